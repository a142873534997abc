// jpeglibrary_amd/csrc/device_batch_resize.cpp -- DeviceBatch: the resize stage (K4, k4_resample.hip).  The setting, the plan of an upload at
// the size that is set (one descriptor per image that was planned without error, one tap table per distinct (input length, output length)
// pair), the launch behind K3, and the accessors of the resized buffer.
#include <hip/hip_runtime.h>

#include <map>
#include <utility>
#include <vector>

#include "device_batch.h"
#include "kernels.h"
#include "resize_tables.h"

namespace jpgpu {

static constexpr int kResizeMaxSide = 65535;

int DeviceBatch::set_resize(int out_width, int out_height, int sample_format) {
    if (out_width == 0 && out_height == 0) {
        resize_ = ResizeSetting();
        resized_fmt_ = -1;  // (what an earlier decode left is withdrawn with it)
        return JPGPU_OK;
    }
    // (a refusal leaves the setting in force as it is)
    if (out_width <= 0 || out_height <= 0) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_resize: the size is two positive numbers, or (0, 0) to withdraw it");
    if (out_width > kResizeMaxSide || out_height > kResizeMaxSide) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_resize: a side is 65535 samples at the most");
    if (!fmt_is_rgb_planes(sample_format))
        return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_resize: the sample format is RGB_PLANAR_U8, RGB_PLANAR_F16 or RGB_PLANAR_F32");
    resize_.width = out_width;
    resize_.height = out_height;
    resize_.format = sample_format;
    return JPGPU_OK;
}

int DeviceBatch::check_resize_format(const char *who) {
    if (resize_.width == 0 || format_ == JPGPU_FMT_RGB_PLANAR_U8) return JPGPU_OK;
    return fail(JPGPU_ERR_ARGUMENT, std::string(who) + ": a resize is set (jpgpu_batch_set_resize), which reads RGB_PLANAR_U8; the upload has another format");
}

// One descriptor per image whose plan holds (the others' slabs stay zero), one table per distinct (input, output) pair of lengths and
// both axes -- equal windows share theirs -- sent to the device.  Made once per upload and size.
int DeviceBatch::plan_resize() {
    if (resize_plan_valid_ && resize_plan_width_ == resize_.width && resize_plan_height_ == resize_.height) return JPGPU_OK;
    const int ow = resize_.width, oh = resize_.height;
    std::vector<ResizeImage> desc;
    std::vector<uint32_t> words;
    std::map<std::pair<int, int>, std::pair<uint32_t, uint32_t>> known;  // (input, output) -> (first word, taps)
    auto table = [&](int in_len, int out_len) {
        auto hit = known.find({in_len, out_len});
        if (hit == known.end()) {
            const ResizeAxis axis = resize_axis(in_len, out_len);
            const uint32_t off = resize_axis_pack(axis, words);
            hit = known.emplace(std::make_pair(in_len, out_len), std::make_pair(off, (uint32_t)axis.max_taps)).first;
        }
        return hit->second;
    };
    for (size_t i = 0; i < images_.size(); i++) {
        const ImagePlan &img = images_[i];
        if (img.status != JPGPU_OK || img.jobs.empty() || img.out_bytes == 0 || img.win.width == 0 || img.win.height == 0) continue;
        const uint64_t planes = one_plane_upload() ? 1u : 3u;  // (a JPGPU_CHANNELS_LUMA upload: ONE tight plane per image, and K4's one-plane form)
        if ((uint64_t)img.win.width * img.win.height * planes != img.out_bytes || img.out_offset + img.out_bytes > out_bytes_) continue;  // (not `planes` tight planes: no entry)
        ResizeImage d;
        d.src_off = img.out_offset;
        d.dst_off = (uint64_t)i * planes * (uint64_t)oh * (uint64_t)ow;
        d.w_in = img.win_oriented.width;  // (the output's size: the window as the caller sees it, turned with the image)
        d.h_in = img.win_oriented.height;
        const auto h = table((int)d.w_in, ow), v = table((int)d.h_in, oh);
        d.h_off = h.first;
        d.h_taps = h.second;
        d.v_off = v.first;
        d.v_taps = v.second;
        desc.push_back(d);
    }
    n_resize_images_ = (int)desc.size();
    if (!desc.empty()) {
        hipError_t e = d_resize_images_.reserve(desc.size() * sizeof(ResizeImage));
        if (e == hipSuccess) e = d_resize_tables_.reserve(words.size() * sizeof(uint32_t));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(resize plan)");
        e = hipMemcpyAsync(d_resize_images_.ptr, desc.data(), desc.size() * sizeof(ResizeImage), hipMemcpyHostToDevice, ctx_->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_resize_tables_.ptr, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx_->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx_->stream);  // `desc` and `words` are local (pageable) vectors
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(resize plan)");
    }
    resize_plan_valid_ = true;
    resize_plan_width_ = ow;
    resize_plan_height_ = oh;
    return JPGPU_OK;
}

int DeviceBatch::run_resize() {
    if (resize_.width == 0) return JPGPU_OK;
    if (const int rc = check_resize_format("jpgpu_batch_run_idct"); rc != JPGPU_OK) return rc;
    if (const int rc = plan_resize(); rc != JPGPU_OK) return rc;
    const int ow = resize_.width, oh = resize_.height;
    const uint64_t planes = one_plane_upload() ? 1u : 3u;
    const uint64_t bytes = (uint64_t)images_.size() * planes * (uint64_t)oh * (uint64_t)ow * (uint64_t)fmt_rgb_plane_sample_bytes(resize_.format);
    resized_fmt_ = -1;
    hipError_t e = d_resized_.reserve((size_t)bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(resized images)");
    for (hipEvent_t &ev : resize_ev_)
        if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) return hip_fail(e, "hipEventCreate(resize)");
    // an image without an entry reads as zeros
    if (bytes != 0 && (e = hipMemsetAsync(d_resized_.ptr, 0, (size_t)bytes, ctx_->stream)) != hipSuccess) return hip_fail(e, "hipMemsetAsync(resized images)");
    if ((e = hipEventRecord(resize_ev_[0], ctx_->stream)) != hipSuccess) return hip_fail(e, "hipEventRecord(resize)");
    e = (one_plane_upload() ? launch_resample_luma : launch_resample)(ctx_->stream, (const uint8_t *)d_out_.ptr, (const ResizeImage *)d_resize_images_.ptr, n_resize_images_,
                                                                (const uint32_t *)d_resize_tables_.ptr, d_resized_.ptr, ow, oh, resize_.format, output_affine_);
    if (e != hipSuccess) return hip_fail(e, "resample_kernel");
    if ((e = hipEventRecord(resize_ev_[1], ctx_->stream)) != hipSuccess) return hip_fail(e, "hipEventRecord(resize)");
    resized_width_ = ow;
    resized_height_ = oh;
    resized_fmt_ = resize_.format;
    resized_images_ = (int)images_.size();
    resized_planes_ = (int)planes;
    return mark_work();
}

int DeviceBatch::resized_device(void **ptr, uint64_t *bytes) const {
    if (!ptr || !bytes) {
        ctx_->last_error = "jpgpu_batch_resized_device: null argument";
        return JPGPU_ERR_ARGUMENT;
    }
    if (resized_fmt_ < 0) {
        ctx_->last_error = "jpgpu_batch_resized_device: no decode with a resize set has run on this upload";
        return JPGPU_ERR_INVALID_OPERATION;
    }
    *ptr = d_resized_.ptr;
    *bytes = (uint64_t)resized_images_ * (uint64_t)resized_planes_ * (uint64_t)resized_height_ * (uint64_t)resized_width_ * (uint64_t)fmt_rgb_plane_sample_bytes(resized_fmt_);
    return JPGPU_OK;
}

int DeviceBatch::download_resized(int i, void *dst, uint64_t bytes) {
    if (resized_fmt_ < 0) return fail(JPGPU_ERR_INVALID_OPERATION, "jpgpu_batch_download_resized: no decode with a resize set has run on this upload");
    if (!dst || i < 0 || i >= resized_images_) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_download_resized: bad argument");
    const uint64_t slab = (uint64_t)resized_planes_ * (uint64_t)resized_height_ * (uint64_t)resized_width_ * (uint64_t)fmt_rgb_plane_sample_bytes(resized_fmt_);
    if (bytes < slab) return fail(JPGPU_ERR_ARGUMENT, "Destination buffer is too small.");
    if (const int rc = sync(); rc != JPGPU_OK) return rc;
    if (resized_fmt_ < 0) return fail(JPGPU_ERR_INVALID_OPERATION, "jpgpu_batch_download_resized: the decode was issued again without its resize");
    hipError_t e = hipMemcpy(dst, (const uint8_t *)d_resized_.ptr + (uint64_t)i * slab, (size_t)slab, hipMemcpyDeviceToHost);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, "hipMemcpy(resized image)");
}

int DeviceBatch::resize_ms(float *ms) {
    if (!ms) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_resize_ms: null argument");
    if (resized_fmt_ < 0) return fail(JPGPU_ERR_INVALID_OPERATION, "jpgpu_batch_resize_ms: no decode with a resize set has run on this upload");
    if (const int rc = sync(); rc != JPGPU_OK) return rc;
    if (hipEventElapsedTime(ms, resize_ev_[0], resize_ev_[1]) != hipSuccess) return fail(JPGPU_ERR_DEVICE, "hipEventElapsedTime failed");
    return JPGPU_OK;
}

}  // namespace jpgpu
