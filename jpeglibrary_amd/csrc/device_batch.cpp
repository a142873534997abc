// jpeglibrary_amd/csrc/device_batch.cpp -- a batch of scan jobs: its buffers and errors, an image's output geometry, the ordering of an upload
// behind unsynchronised work, and the uploads of single scan jobs, progressive frames and scans, and coefficient frames.  (The file is split by role:
// device_batch_ingest.cpp = the uploads of whole files (jpgpu_batch_upload*): host-side plans, staging, the ingest's stages; device_batch_layout.cpp =
// layout_and_upload and the planning stages it calls, which every upload path ends in; device_batch_launch.cpp = the launches of a decode,
// device_batch_result.cpp = results, the partial-flush replay, downloads.)
//
// HBM layout (all offsets 256-byte aligned unless noted):
//   input   : the files' bytes back to back (256-byte slots, 256 bytes of slack before the first and after the last)
//   ends    : uint32 per restart interval: offset of the FF that closes it (written by K1, read by K2)
//   coefs   : int16[total_blocks][64], zig-zag order, blocks in MCU scan order per scan job (K2 -> K3)
//   out     : per image, in the batch's format (INTERLEAVED_U8: W*H*C bytes; PLANAR_*: padded planes)
#include "device_batch.h"

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "kernels.h"
#include "k3r_reduced.h"

namespace jpgpu {

static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

hipError_t DevBuffer::reserve(size_t bytes) {
    if (bytes <= cap && ptr) return hipSuccess;
    if (ptr) {
        hipError_t e = hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        if (e != hipSuccess) return e;
    }
    if (bytes == 0) bytes = 256;
    hipError_t e = hipMalloc(&ptr, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
}
void DevBuffer::release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
}

DeviceBatch::~DeviceBatch() {
    if (ctx_) (void)hipSetDevice(ctx_->device);
    for (DevBuffer *b : {&d_sub_work_, &d_sub_final_work_, &d_sub_scan_ids_, &d_sub_exit_a_, &d_sub_exit_b_, &d_sub_nblk_, &d_sub_first_, &d_sub_entry_, &d_sub_dcsum_, &d_sub_dcentry_, &d_sub_changed_, &d_sub_same_, &d_sub_perm_, &d_k1_desc_, &d_k1_tickets_, &d_k2_tickets_, &d_sr_luts_, &d_sr_set_scan_, &d_k1_order_, &d_prog_snapshot_, &d_dense_, &d_split_ids_, &d_dispose_, &d_verify_, &d_lut_pool_, &d_prog_work_, &d_prog_sync_, &d_planes_, &d_extend_desc_, &d_gather_, &d_heads_, &d_rgb_scratch_, &d_color_images_, &d_orient_images_, &d_fancy_images_, &d_luma_images_, &d_luma_work_, &d_islow_work_, &d_reduced_work_, &d_chunk_work_, &d_chunk_sums_, &d_unstuffed_, &d_ends_u_, &d_input_, &d_scans_, &d_status_, &d_ends_, &d_huff_pool_, &d_quant_pool_, &d_huff_work_, &d_idct_work_, &d_idct_work_halves_, &d_coefs_, &d_out_, &d_resized_, &d_resize_images_, &d_resize_tables_})
        b->release();
    for (hipEvent_t &e : ev_pool_)
        if (e) (void)hipEventDestroy(e);
    if (done_ev_) (void)hipEventDestroy(done_ev_);
    for (hipEvent_t ev : gather_ev_)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : resize_ev_)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : fancy_ev_)
        if (ev) (void)hipEventDestroy(ev);
    if (h_k1_giveup_) (void)hipHostFree(h_k1_giveup_);
}

int DeviceBatch::fail(int status, const std::string &msg) {
    ctx_->last_error = msg;
    return status;
}
int DeviceBatch::hip_fail(hipError_t e, const char *what) {
    return fail(e == hipErrorOutOfMemory ? JPGPU_ERR_OUT_OF_MEMORY : JPGPU_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

bool DeviceBatch::fancy_filtered(int policy, int format, const ImagePlan &img) {
    return policy == JPGPU_UPSAMPLE_FANCY && img.luma == kLumaNone && fmt_is_rgb(format) && img.color_kind == kColorYcbcr && img.num_components == 3 && img.precision == 8 &&
           k3u_ratio_filtered(img.chroma_hs, img.chroma_vs, img.pic_w) && img.scale < 8;  // (libjpeg: no filter where a block yields one sample)
}

jpgpu_rect DeviceBatch::fancy_fetch_rect(const ImagePlan &img) {
    const K3uSpan x = k3u_fetch_span(img.win.x, img.win.x + img.win.width, img.pic_w, img.chroma_hs);
    const K3uSpan y = k3u_fetch_span(img.win.y, img.win.y + img.win.height, img.pic_h, img.chroma_vs);
    return jpgpu_rect{x.lo, y.lo, x.hi - x.lo, y.hi - y.lo};
}

// (16 bytes behind the fetch rectangle stay unused: K3U's 12-byte loads of a line's last pixels end there)
uint64_t DeviceBatch::fancy_staging_offset(const ImagePlan &img) {
    const jpgpu_rect f = fancy_fetch_rect(img);
    return ((uint64_t)f.width * f.height * 3 + 16 + 255) / 256 * 256;
}

uint64_t DeviceBatch::slot_bytes(const ImagePlan &img) {
    if (img.fancy) {  // the fetch rectangle's samples, and behind them the staged window of an image that is turned as well
        const jpgpu_rect f = fancy_fetch_rect(img);
        const uint64_t samples = img.orientation != 1 ? fancy_staging_offset(img) + (uint64_t)img.win.width * img.win.height * 3 : (uint64_t)f.width * f.height * 3;
        return std::max(img.out_bytes, samples);
    }
    const bool through_scratch = color_kind_by_file(img.color_kind) || img.orientation != 1 || img.luma == kLumaScratch || img.islow;
    const uint64_t samples = through_scratch ? (uint64_t)img.win.width * img.win.height * color_kind_sample_bytes(img.color_kind) : 0u;
    return std::max(img.out_bytes, samples);
}

int DeviceBatch::set_color_policy(int policy) {
    if (policy != JPGPU_COLOR_YCC && policy != JPGPU_COLOR_FILE) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_color_policy: unknown policy");
    color_policy_ = policy;
    return JPGPU_OK;
}

int DeviceBatch::image_color(int i, int *kind) const {
    const ImagePlan *img = image(i);
    if (!img || !kind) return JPGPU_ERR_ARGUMENT;
    *kind = img->status == JPGPU_OK ? img->color_kind : kColorYcbcr;  // (include/jpgpu.h: YCBCR for an image that failed at upload, its window's refusal included)
    return JPGPU_OK;
}

int DeviceBatch::set_orientation_policy(int policy) {
    if (policy != JPGPU_ORIENT_STORED && policy != JPGPU_ORIENT_FILE) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_orientation_policy: unknown policy");
    orient_policy_ = policy;
    return JPGPU_OK;
}

int DeviceBatch::set_orientations(const uint8_t *orientations, int n) {
    if (n < 0 || (n > 0 && !orientations)) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_orientations: bad argument");
    for (int i = 0; i < n; i++)
        if (orientations[i] > 8) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_orientations: an orientation is 1..8, or 0 for what the policy gives");
    pending_orientations_.assign(orientations, orientations + n);
    orientations_pending_ = n > 0;
    return JPGPU_OK;
}

int DeviceBatch::set_upsampling_policy(int policy) {
    if (policy != JPGPU_UPSAMPLE_REPLICATE && policy != JPGPU_UPSAMPLE_FANCY) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_upsampling_policy: unknown policy");
    upsample_policy_ = policy;
    return JPGPU_OK;
}

int DeviceBatch::image_upsampling(int i, int *applied) const {
    const ImagePlan *img = image(i);
    if (!img || !applied) return JPGPU_ERR_ARGUMENT;
    *applied = img->status == JPGPU_OK && img->fancy ? 1 : 0;
    return JPGPU_OK;
}

int DeviceBatch::set_channels_policy(int policy) {
    if (policy != JPGPU_CHANNELS_RGB && policy != JPGPU_CHANNELS_LUMA) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_channels_policy: unknown policy");
    channels_policy_ = policy;
    return JPGPU_OK;
}

int DeviceBatch::image_channels(int i, int *channels) const {
    const ImagePlan *img = image(i);
    if (!img || !channels) return JPGPU_ERR_ARGUMENT;
    *channels = img->status == JPGPU_OK && img->luma != kLumaNone ? 1 : 3;
    return JPGPU_OK;
}

int DeviceBatch::luma_work(int32_t counts[2]) const {
    if (!counts) return JPGPU_ERR_ARGUMENT;
    counts[0] = counts[1] = 0;
    for (const ImagePlan &img : images_)
        if (img.status == JPGPU_OK && img.luma != kLumaNone) counts[img.luma == kLumaFast ? 0 : 1]++;
    return JPGPU_OK;
}

bool DeviceBatch::luma_fast(const ImagePlan &img, const std::vector<ScanJob> &jobs, bool keep_canvas) {
    if (img.color_kind != kColorGray && img.color_kind != kColorYcbcr) return false;
    if (img.precision != 8 || img.orientation != 1 || keep_canvas || jobs.size() != 1) return false;
    const ScanJob &job = jobs[0];
    if (job.kind != kScanSequential || job.disabled || job.scan_components != img.num_components) return false;
    if (job.blocks_per_mcu < 1 || job.blocks_per_mcu > kMaxBlocksPerMcu || job.geo.mcus_per_line <= 0 || job.geo.mcus_per_column <= 0) return false;
    // frame component 0 first, at the frame's maxima, and named once (a scan that names it again writes over its blocks: K3's business).
    // (Vertically also ONE block per MCU column under a taller MCU -- (2, 1) luma beside (1, 2) chroma --: K3Y repeats its sample rows as the
    // reference's replication does.  Several blocks that are replicated as well overlap in the reference; those stay K3's.)
    const ResolvedScanComponent &c0 = job.comp[0];
    if (c0.component_index != 0 || c0.hs != 1 || c0.h < 1 || c0.h > 4 || c0.v < 1 || c0.v > 4) return false;
    if (!(c0.vs == 1 || (c0.v == 1 && c0.vs >= 2 && c0.vs <= 4))) return false;
    for (int c = 1; c < job.scan_components; c++)
        if (job.comp[c].component_index == 0) return false;
    // its blocks are the MCU's first, in raster order: slot by * h + bx (what K3Y's index arithmetic assumes)
    const int n0 = c0.h * c0.v;
    if (n0 > job.blocks_per_mcu) return false;
    for (int k = 0; k < n0; k++)
        if (job.blk_comp[k] != 0 || job.blk_x[k] != k % c0.h || job.blk_y[k] != k / c0.h) return false;
    return true;
}

int DeviceBatch::set_arithmetic_policy(int policy) {
    if (policy != JPGPU_ARITHMETIC_REFERENCE && policy != JPGPU_ARITHMETIC_LIBJPEG) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_arithmetic_policy: unknown policy");
    arithmetic_policy_ = policy;
    return JPGPU_OK;
}

int DeviceBatch::image_arithmetic(int i, int *arithmetic) const {
    const ImagePlan *img = image(i);
    if (!img || !arithmetic) return JPGPU_ERR_ARGUMENT;
    *arithmetic = img->status == JPGPU_OK && img->islow ? JPGPU_ARITHMETIC_LIBJPEG : JPGPU_ARITHMETIC_REFERENCE;
    return JPGPU_OK;
}

// libjpeg's jdcolor.c: FIX(1.40200), -FIX(0.71414), FIX(1.77200), -FIX(0.34414) -- the last one is where the reference's differ (-22553)
YccRgbFactors DeviceBatch::color_factors() const {
    if (islow_upload_ && whole_files_) return YccRgbFactors{91881, -46802, 116130, -22554};
    return ycc_rgb_factors();
}

bool DeviceBatch::islow_taken(int policy, int format, const ImagePlan &img, const std::vector<ScanJob> &jobs, bool keep_canvas) {
    if (policy != JPGPU_ARITHMETIC_LIBJPEG || !fmt_is_rgb(format) || img.precision != 8 || keep_canvas || jobs.empty()) return false;
    // (K3J stores color_kind_sample_bytes() bytes per pixel of the scratch slot, one per frame component)
    if (img.num_components < 1 || img.num_components > kMaxScanComponents || img.num_components != color_kind_sample_bytes(img.color_kind)) return false;
    auto pow2 = [](int r) { return r == 1 || r == 2 || r == 4; };
    uint32_t written = 0;  // frame components some sequential scan has written
    for (const ScanJob &job : jobs) {
        if (job.kind == kScanProgressive) continue;  // (an entropy scan of a progressive frame: no transform of its own)
        if (job.kind == kScanFrameOnly && job.dispose_generic) return false;  // the literal Dispose(): the store holds samples when the output stage runs
        if (job.blocks_per_mcu < 1 || job.blocks_per_mcu > kMaxBlocksPerMcu || job.geo.mcus_per_line <= 0 || job.geo.mcus_per_column <= 0) return false;
        if (job.scan_components < 1 || job.scan_components > kMaxScanComponents) return false;
        uint32_t mask = 0;
        for (int c = 0; c < job.scan_components; c++) {
            const ResolvedScanComponent &sc = job.comp[c];
            if (sc.component_index < 0 || sc.component_index >= img.num_components) return false;
            if ((mask >> sc.component_index) & 1u) return false;  // named twice: the later block wins, K3's business
            mask |= 1u << sc.component_index;
            if (!pow2(sc.hs) || !pow2(sc.vs)) return false;
            // several blocks per MCU line or column that are replicated as well overlap in a sequential scan (k3_idct.hip)
            if (job.kind == kScanSequential && ((sc.h > 1 && sc.hs > 1) || (sc.v > 1 && sc.vs > 1))) return false;
        }
        for (int k = 0; k < job.blocks_per_mcu; k++)
            if (job.blk_comp[k] >= job.scan_components) return false;
        if (job.kind == kScanSequential) {
            if (mask & written) return false;  // scans ordered behind each other: K3's levels
            written |= mask;
        }
    }
    return true;
}

int DeviceBatch::set_scale_policy(int denom) {
    if (denom != 1 && denom != 2 && denom != 4 && denom != 8) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_scale_policy: the denominator is 1, 2, 4 or 8");
    scale_policy_ = denom;
    return JPGPU_OK;
}

int DeviceBatch::set_scale_fit(uint32_t min_w, uint32_t min_h) {
    if ((min_w == 0) != (min_h == 0)) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_scale_fit: a least size has two positive sides; (0, 0) switches the rule off");
    scale_fit_w_ = min_w;
    scale_fit_h_ = min_h;
    return JPGPU_OK;
}

int DeviceBatch::image_scale(int i, int *denom) const {
    const ImagePlan *img = image(i);
    if (!img || !denom) return JPGPU_ERR_ARGUMENT;
    *denom = img->status == JPGPU_OK ? img->scale : 1;
    return JPGPU_OK;
}

// Pillow's draft(): the largest of 8, 4, 2 that leaves the oriented frame at least the least size in both directions
int DeviceBatch::scale_wanted(const ImagePlan &img, int orientation) const {
    if (scale_fit_w_ == 0) return scale_policy_;
    const uint32_t ow = orientation_transposes(orientation) ? img.height : img.width, oh = orientation_transposes(orientation) ? img.width : img.height;
    const uint32_t k = std::min(ow / scale_fit_w_, oh / scale_fit_h_);
    return k >= 8 ? 8 : (k >= 4 ? 4 : (k >= 2 ? 2 : 1));
}

// The plan of an image that takes libjpeg's transform, at 1 / denom: the reduced picture's size, and of a three-component image whose
// chroma ratio the frame states (plan_image_geometry) the ratio jdmaster's per-component transform sizes leave in it (k3r_reduced.h).
// The whole picture is its window; apply_window sizes the output by it.
void DeviceBatch::plan_reduced_geometry(ImagePlan &img, const BaselineGeometry &geo, int denom) {
    const uint32_t m = 8u / (uint32_t)denom;
    img.scale = (uint8_t)denom;
    img.pic_w = (uint16_t)(((uint32_t)img.width * m + 7u) / 8u);
    img.pic_h = (uint16_t)(((uint32_t)img.height * m + 7u) / 8u);
    if (img.chroma_hs != 0 && img.chroma_vs != 0) {
        const FrameComponent &c1 = geo.frame.components[1];
        const uint32_t bs = reduced_block_size(m, c1.h, c1.v, (uint32_t)geo.max_h, (uint32_t)geo.max_v);
        img.chroma_hs = (uint8_t)reduced_replication(m, bs, c1.h, (uint32_t)geo.max_h);
        img.chroma_vs = (uint8_t)reduced_replication(m, bs, c1.v, (uint32_t)geo.max_v);
    }
    img.win = img.win_oriented = jpgpu_rect{0, 0, img.pic_w, img.pic_h};
}

int DeviceBatch::upsampling_ms(float *ms) {
    if (!ms) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upsampling_ms: null argument");
    if (!fancy_timed_) return fail(JPGPU_ERR_INVALID_OPERATION, "jpgpu_batch_upsampling_ms: no K3U call of this upload was timed (JPGPU_TIME_UPSAMPLE=1 at the upload, a filtered image, a decode)");
    if (const int rc = sync(); rc != JPGPU_OK) return rc;
    if (hipEventElapsedTime(ms, fancy_ev_[0], fancy_ev_[1]) != hipSuccess) return fail(JPGPU_ERR_DEVICE, "hipEventElapsedTime failed");
    return JPGPU_OK;
}

int DeviceBatch::image_orientation(int i, int *orientation) const {
    const ImagePlan *img = image(i);
    if (!img || !orientation) return JPGPU_ERR_ARGUMENT;
    *orientation = img->status == JPGPU_OK ? img->orientation : 1;  // (include/jpgpu.h: 1 for an image that failed at upload, its window's refusal included)
    return JPGPU_OK;
}

void DeviceBatch::plan_image_geometry(ImagePlan &img, const BaselineGeometry &geo, const ColorMarkers &markers, int exif_orientation) const {
    const FrameHeader &fh = geo.frame;
    img.width = fh.samples_per_line;
    img.height = fh.lines;
    img.precision = fh.precision;
    img.num_components = fh.num_components;
    img.color_kind = fh.num_components == 1 ? kColorGray : kColorYcbcr;
    // (what the frame says about its chroma; whether the image is filtered is apply_window's decision)
    img.chroma_hs = img.chroma_vs = 0;
    img.fancy = false;
    img.luma = kLumaNone;
    img.islow = false;
    img.scale = 1;
    img.pic_w = img.width;
    img.pic_h = img.height;
    if (fh.num_components == 3 && fh.components.size() == 3) {
        const auto &c0 = fh.components[0], &c1 = fh.components[1], &c2 = fh.components[2];
        if (c0.h == geo.max_h && c0.v == geo.max_v && c1.h == c2.h && c1.v == c2.v && c1.h > 0 && c1.v > 0 && geo.max_h % c1.h == 0 && geo.max_v % c1.v == 0) {
            img.chroma_hs = (uint8_t)(geo.max_h / c1.h);
            img.chroma_vs = (uint8_t)(geo.max_v / c1.v);
        }
    }
    img.restart_interval = geo.restart_interval;
    img.mcus_per_line = (uint32_t)geo.mcus_per_line;
    img.mcus_per_column = (uint32_t)geo.mcus_per_column;
    if (fmt_is_sample_bytes(format_)) {
        // the two stock writers it follows (JpegBufferOutputWriterLessThan8Bit / GreaterThan8Bit): at P = 0 ExpandBits never ends,
        // above 16 there is no 16-bit sample to shift -- no behaviour to follow, the image fails by itself
        if (format_ == JPGPU_FMT_INTERLEAVED_U8_SCALED && (fh.precision < 1 || fh.precision > 16))
            throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "INTERLEAVED_U8_SCALED is defined for precisions 1..16 only.", kDetailUnsupportedFrame);
        img.out_bytes = (uint64_t)img.width * img.height * img.num_components;
    } else if (fmt_is_rgb(format_)) {
        if (color_policy_ == JPGPU_COLOR_FILE) {  // the one decision the policy makes (ingest_host.h); what it refuses is refused below, as ever
            uint8_t ids[4] = {0, 0, 0, 0};
            for (size_t c = 0; c < fh.components.size() && c < 4; c++) ids[c] = fh.components[c].identifier;
            const int kind = color_kind_of(fh.precision, fh.num_components, ids, markers);
            if (kind >= 0) img.color_kind = (uint8_t)kind;
        }
        const bool four = img.color_kind == kColorCmyk || img.color_kind == kColorYcck;
        if (fh.num_components != 1 && fh.num_components != 3 && !four)  // apps/JpegDecode/DecodeAction.cs:29-33
            throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "This color space is not supported", kDetailUnsupportedFrame);
        if (fh.precision != 8)
            throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "RGB output is defined for 8-bit precision only (the reference converter assumes 8-bit samples).",
                              kDetailUnsupportedFrame);
        // (the three-plane formats: one, two or four bytes per sample)
        img.out_bytes = (uint64_t)img.width * img.height * (format_ == JPGPU_FMT_RGBA_U8 ? 4 : 3) * fmt_rgb_plane_sample_bytes(format_);
        if (fmt_is_rgb_planes(format_))  // three tight planes R, G, B (a 1-component frame too: R = G = B); offset in bytes, the rest in samples
            for (int c = 0; c < 3; c++)
                img.plane[c] = jpgpu_plane_info{(uint64_t)c * img.width * img.height * fmt_rgb_plane_sample_bytes(format_), img.width, img.height, img.width};
    } else {
        if (fh.num_components > 4)  // jpgpu_plane_info describes four planes; a fifth component would land on plane 0
            throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "The planar output formats describe at most 4 components.", kDetailUnsupportedFrame);
        // the test writer spreads P bits over 16 (JpegExtendingOutputWriter.cs:83-110): at P = 0 its ExpandBits loop never
        // ends, above 16 the shifts leave the 32-bit range -- there is no behaviour to follow, the image fails by itself
        if (format_ == JPGPU_FMT_EXTENDED_U16 && (fh.precision < 1 || fh.precision > 16))
            throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "EXTENDED_U16 is defined for precisions 1..16 only.", kDetailUnsupportedFrame);
        // EXTENDED_U16 is produced from int16 planes (K3's PLANAR_I16 output in a scratch buffer, see run_idct)
        const uint64_t sample_bytes = (format_ == JPGPU_FMT_PLANAR_I16 || format_ == JPGPU_FMT_EXTENDED_U16) ? 2 : 1;
        uint64_t off = 0;
        for (int c = 0; c < fh.num_components && c < 4; c++) {
            jpgpu_plane_info &p = img.plane[c];
            p.width = (uint32_t)geo.mcus_per_line * fh.components[c].h * 8;
            p.height = (uint32_t)geo.mcus_per_column * fh.components[c].v * 8;
            p.pitch = p.width;
            p.offset = off;
            off = align_up(off + (uint64_t)p.pitch * p.height * sample_bytes, 256);
        }
        img.out_bytes = off;
        if (format_ == JPGPU_FMT_EXTENDED_U16) {
            img.planes_bytes = off;
            img.out_bytes = (uint64_t)img.width * img.height * 4 * sizeof(uint16_t);
        }
    }
    img.windowed = false;  // (a window is applied behind the plans, DeviceBatch::apply_window)
    img.win = img.win_oriented = jpgpu_rect{0, 0, img.width, img.height};
    img.exif_orientation = (uint8_t)exif_orientation;  // (what the file says; what the image is planned with is apply_window's decision)
    img.orientation = 1;
    // A frame header is two 16-bit sizes and a component count: a corrupted one can ask for hundreds of gigabytes (the
    // reference's caller would fail allocating the writer's buffer).  Such an image fails BY ITSELF instead of taking the
    // batch's allocation, and every other image, with it (tools/stress_parity.py STRESS_HEADER=1, seed 460).
    if (ctx_ && ctx_->device_bytes != 0 && img.out_bytes + img.planes_bytes > ctx_->device_bytes)
        throw DecodeError(JPGPU_ERR_OUT_OF_MEMORY, "The frame's output (" + std::to_string(img.out_bytes + img.planes_bytes) +
                                                        " bytes) is larger than the device's memory.", kDetailUnsupportedFrame);
}

int DeviceBatch::mark_work() {
    if (!done_ev_) {
        hipError_t e = hipEventCreateWithFlags(&done_ev_, hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreate(done)");
    }
    hipError_t e = hipEventRecord(done_ev_, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord(done)");
    work_in_flight_ = true;
    return JPGPU_OK;
}

// An upload rewrites the batch's inputs, descriptors and work lists on the upload stream; kernels this batch launched on the
// decode stream and nobody waited for may still be reading them.  The upload stream waits for them on the device (the host
// does not block, another batch's decode is not waited for).
int DeviceBatch::order_upload_behind_work() {
    if (!work_in_flight_ || !done_ev_) return JPGPU_OK;
    hipError_t e = hipStreamWaitEvent(ctx_->upload_stream, done_ev_, 0);
    if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent(upload behind decode)");
    return JPGPU_OK;
}

int DeviceBatch::upload_single_job(const ScanJob &job, int format, const void *initial_output, size_t initial_output_bytes) {
    whole_files_ = false;
    device_ingest_ = jpgpu_device_ingest_stats();
    if (format < 0 || format >= kNumOutputFormats) return fail(JPGPU_ERR_ARGUMENT, "unknown format");
    format_ = format;
    images_.assign(1, ImagePlan());
    jobs_.assign(1, job);
    job_image_.assign(1, 0);
    job_entropy_off_.assign(1, 0);
    ImagePlan &img = images_[0];
    img.sof = kSOF0;
    img.file_len = job.entropy_len;
    plan_image_geometry(img, job.geo);
    img.blocks_per_mcu = (uint32_t)job.blocks_per_mcu;
    img.jobs.push_back(0);
    std::vector<const uint8_t *> fp(1, job.entropy);
    std::vector<size_t> fl(1, job.entropy_len);
    keep_canvas_ = initial_output && initial_output_bytes;
    int rc = layout_and_upload(fp, fl);
    keep_canvas_ = false;
    if (rc != JPGPU_OK) return rc;
    if (initial_output && initial_output_bytes) {
        out_clear_.clear();  // the caller's buffer is the canvas: what this scan does not write keeps the caller's samples
        const size_t nbytes = std::min<size_t>(initial_output_bytes, img.out_bytes);
        hipError_t e = hipMemcpyAsync((uint8_t *)d_out_.ptr + img.out_offset, initial_output, nbytes, hipMemcpyHostToDevice, ctx_->upload_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx_->upload_stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(initial output)");
    }
    return JPGPU_OK;
}

int DeviceBatch::upload_progressive_frame(const ProgressiveFrame &frame, const uint8_t *file, size_t file_len, int sof, int format) {
    whole_files_ = false;
    device_ingest_ = jpgpu_device_ingest_stats();
    if (format < 0 || format >= kNumOutputFormats) return fail(JPGPU_ERR_ARGUMENT, "unknown format");
    format_ = format;
    images_.assign(1, ImagePlan());
    jobs_.clear();
    job_image_.clear();
    job_entropy_off_.clear();
    jobs_.push_back(frame.make_frame_job());  // throws DecodeError for scan orders the reference mangles
    for (const ScanJob &j : frame.scans()) jobs_.push_back(j);
    ImagePlan &img = images_[0];
    img.sof = (uint8_t)sof;
    img.file_len = file_len;
    plan_image_geometry(img, jobs_[0].geo);
    img.blocks_per_mcu = (uint32_t)jobs_[0].blocks_per_mcu;
    for (size_t j = 0; j < jobs_.size(); j++) {
        img.jobs.push_back((int)j);
        job_image_.push_back(0);
        job_entropy_off_.push_back(jobs_[j].entropy ? (uint64_t)(jobs_[j].entropy - file) : 0u);
    }
    std::vector<const uint8_t *> fp(1, file);
    std::vector<size_t> fl(1, file_len);
    const int rc = layout_and_upload(fp, fl);
    replay_possible_ = rc == JPGPU_OK;  // (a scan that fails: the frame is issued again in file order up to the throw, like a file of a batch)
    return rc;
}

int DeviceBatch::upload_progressive_scan(const ProgressiveFrame &frame, int scan_index, bool first_scan) {
    whole_files_ = false;
    device_ingest_ = jpgpu_device_ingest_stats();
    if (scan_index < 0 || scan_index >= (int)frame.scans().size()) return fail(JPGPU_ERR_ARGUMENT, "progressive scan index out of range");
    format_ = JPGPU_FMT_INTERLEAVED_U8;  // no samples are produced by a scan; the smallest output layout
    images_.assign(1, ImagePlan());
    jobs_.clear();
    job_image_.clear();
    job_entropy_off_.clear();
    jobs_.push_back(frame.make_frame_job());  // the store's geometry (and position: block 0 of the coefficient buffer)
    jobs_.push_back(frame.scans()[(size_t)scan_index]);
    ScanJob &scan = jobs_.back();
    // the scans this one depends on ran in earlier calls: nothing to wait for inside the launch
    scan.n_deps = 0;
    scan.deps[0] = scan.deps[1] = scan.deps[2] = -1;
    scan.ordinal = 0;
    scan.has_consumers = false;
    ImagePlan &img = images_[0];
    img.sof = kSOF2;
    img.file_len = scan.entropy_len;
    plan_image_geometry(img, jobs_[0].geo);
    img.blocks_per_mcu = (uint32_t)jobs_[0].blocks_per_mcu;
    for (size_t j = 0; j < jobs_.size(); j++) {
        img.jobs.push_back((int)j);
        job_image_.push_back(0);
        job_entropy_off_.push_back(0);
    }
    std::vector<const uint8_t *> fp(1, scan.entropy);
    std::vector<size_t> fl(1, scan.entropy_len);
    const int rc = layout_and_upload(fp, fl);
    keep_progressive_store_ = !first_scan;
    defer_refusal_ = true;
    return rc;
}

int DeviceBatch::snapshot_progressive_store() {
    prog_snapshot_blocks_ = 0;
    if (prog_clear_.empty() || !d_coefs_.ptr) return JPGPU_OK;
    const uint64_t first = prog_clear_[0].first, blocks = prog_clear_[0].second;
    hipError_t e = d_prog_snapshot_.reserve((size_t)blocks * 128 + 256);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(store snapshot)");
    e = hipMemcpyAsync(d_prog_snapshot_.ptr, (const int16_t *)d_coefs_.ptr + first * 64, (size_t)blocks * 128, hipMemcpyDeviceToDevice, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(store snapshot)");
    prog_snapshot_blocks_ = blocks;
    return JPGPU_OK;
}

int DeviceBatch::rerun_failed_progressive_scan(bool first_scan) {
    if (jobs_.size() != 2 || jobs_[1].kind != kScanProgressive || h_status_.size() != 2 || h_status_[1].first_error == kNoError) return JPGPU_OK;
    if (jobs_[1].force_lane) return JPGPU_OK;  // (this WAS the exact kernel)
    jobs_[1].force_lane = true;
    jobs_[1].last_interval = h_status_[1].first_error >> 8;  // the lowest failing restart interval: the reference never got behind it
    std::vector<const uint8_t *> fp(1, nullptr);
    std::vector<size_t> fl(1, images_[0].file_len);
    int rc = layout_and_upload(fp, fl, true);  // (the scan's bytes are in HBM already)
    if (rc != JPGPU_OK) return rc;
    if (first_scan || prog_snapshot_blocks_ == 0 || prog_clear_.empty()) {
        keep_progressive_store_ = false;  // run_progressive() clears the store like JpegBlockAllocator.Allocate
    } else {
        keep_progressive_store_ = true;
        const uint64_t blocks = std::min<uint64_t>(prog_snapshot_blocks_, prog_clear_[0].second);
        hipError_t e = hipMemcpyAsync((int16_t *)d_coefs_.ptr + prog_clear_[0].first * 64, d_prog_snapshot_.ptr, (size_t)blocks * 128, hipMemcpyDeviceToDevice, ctx_->stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(store restore)");
    }
    defer_refusal_ = true;
    if ((rc = run_marker_index()) != JPGPU_OK) return rc;
    if ((rc = run_huffman()) != JPGPU_OK) return rc;
    rc = sync();
    keep_progressive_store_ = true;  // whatever comes next works on this store
    return rc;
}

int DeviceBatch::upload_progressive_dispose(const ProgressiveFrame &frame, int format) {
    whole_files_ = false;
    device_ingest_ = jpgpu_device_ingest_stats();
    if (format < 0 || format >= kNumOutputFormats) return fail(JPGPU_ERR_ARGUMENT, "unknown format");
    format_ = format;
    images_.assign(1, ImagePlan());
    jobs_.clear();
    job_image_.clear();
    job_entropy_off_.clear();
    jobs_.push_back(frame.make_frame_job());
    ImagePlan &img = images_[0];
    img.sof = kSOF2;
    plan_image_geometry(img, jobs_[0].geo);
    img.blocks_per_mcu = (uint32_t)jobs_[0].blocks_per_mcu;
    img.jobs.push_back(0);
    job_image_.push_back(0);
    job_entropy_off_.push_back(0);
    std::vector<const uint8_t *> fp(1, nullptr);
    std::vector<size_t> fl(1, 0);
    const bool store_holds_samples = dispose_done_;  // an earlier Dispose() of this session has transformed the store in place
    const int rc = layout_and_upload(fp, fl);
    dispose_done_ = store_holds_samples && !dispose_jobs_.empty();
    keep_progressive_store_ = true;
    defer_refusal_ = false;
    return rc;
}

int DeviceBatch::upload_frames(const jpgpu_frame *frames, const uint16_t *qt, int n, int format) {
    whole_files_ = false;
    luma_upload_ = false;  // (frames decode to three planes whatever the channels policy)
    islow_upload_ = false;  // (... and with the reference's arithmetic whatever the arithmetic policy)
    device_ingest_ = jpgpu_device_ingest_stats();
    if (windows_pending_ || orientations_pending_) {  // (both are for uploads of whole files: consumed and refused, the batch left empty)
        const bool windows = windows_pending_;
        pending_windows_.clear();
        pending_orientations_.clear();
        windows_pending_ = orientations_pending_ = replay_possible_ = false;
        forget_batch();
        return fail(JPGPU_ERR_ARGUMENT, windows ? "jpgpu_batch_upload_frames: windows are pending (jpgpu_batch_set_windows), and frames take none"
                                                : "jpgpu_batch_upload_frames: orientations are pending (jpgpu_batch_set_orientations), and frames take none");
    }
    windows_.clear();
    orientations_.clear();
    if (n < 0 || (n > 0 && (!frames || !qt))) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload_frames: null argument");
    if (format < 0 || format >= kNumOutputFormats) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload_frames: unknown format");
    format_ = format;
    images_.assign((size_t)n, ImagePlan());
    jobs_.clear();
    job_image_.clear();
    job_entropy_off_.clear();
    std::vector<const uint8_t *> fp((size_t)n, nullptr);
    std::vector<size_t> fl((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        ImagePlan &img = images_[i];
        try {
            const jpgpu_frame &f = frames[i];
            if (f.num_components == 0 || f.num_components > 4) throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "1..4 components are supported.", kDetailUnsupportedFrame);
            HostDecoder dec;
            FrameHeader fh;
            fh.precision = f.precision;
            fh.lines = f.height;
            fh.samples_per_line = f.width;
            fh.num_components = f.num_components;
            ScanHeader sh;
            sh.num_components = f.num_components;
            sh.se = 63;
            for (int c = 0; c < f.num_components; c++) {
                fh.components.push_back({f.comp[c].identifier, f.comp[c].h, f.comp[c].v, f.comp[c].tq});
                sh.components.push_back({f.comp[c].identifier, 0, 0});
                if (f.comp[c].tq > 3) throw DecodeError(JPGPU_ERR_ARGUMENT, "quantisation table selector out of range");
                QuantTable q;
                q.identifier = f.comp[c].tq;
                memcpy(q.elements, qt + ((size_t)i * 4 + f.comp[c].tq) * 64, sizeof q.elements);
                dec.set_quantization_table(q);
            }
            // the IDCT stage needs no Huffman tables; a placeholder keeps the scan-job builder's checks satisfied
            HuffTable dummy;
            const uint8_t bits[16] = {0, 1};
            const uint8_t vals[1] = {0};
            HuffTable::from_bits_values(0, 0, bits, vals, 1, &dummy);
            dec.set_huffman_table(dummy);
            dummy.table_class = 1;
            dec.set_huffman_table(dummy);
            dec.set_frame_header(fh);
            img.sof = f.sof;
            const BaselineGeometry geo = BaselineGeometry::latch(dec, fh);
            jobs_.push_back(make_scan_job(dec, geo, sh, nullptr, 0));
            plan_image_geometry(img, geo);
            img.blocks_per_mcu = (uint32_t)jobs_.back().blocks_per_mcu;
            img.jobs.push_back((int)jobs_.size() - 1);
            job_image_.push_back(i);
            job_entropy_off_.push_back(0);
        } catch (const DecodeError &e) {
            img.status = e.status;
            img.detail = e.detail;
            img.error = e.what();
        }
    }
    return layout_and_upload(fp, fl);
}

}  // namespace jpgpu
