// jpeglibrary_amd/csrc/device_batch.h -- device-resident batch of scan jobs: HBM layout, uploads, kernel launches.  (DeviceBatch is implemented in
// device_batch.cpp, device_batch_ingest.cpp, device_batch_layout.cpp, device_batch_launch.cpp, device_batch_result.cpp and device_batch_resize.cpp, by role.)
#pragma once
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "../../include/jpgpu.h"
#include "common.h"
#include "host.h"
#include "k3u_taps.h"
#include "kernels.h"

namespace jpgpu {
// Crew size when the caller did not choose one: the CPUs this process may really use (affinity mask, cgroup v2 / v1 quota),
// capped at 16; JPGPU_HOST_THREADS overrides.  granted_host_cpus() is the same figure without the cap and the override.
int default_host_threads();
int granted_host_cpus();
// Caller memory a kernel is about to read (jpgpu_encoder_upload_device, jpgpu_batch_upload_device): 0 = [p, p + bytes) is device
// memory of `device` inside one allocation; 1 = hipPointerGetAttributes does not report p as device memory of that device (host,
// pinned host and managed memory among them); 2 = the bytes do not lie inside one allocation (hipMemGetAddressRange).
int check_device_range(int device, const void *p, size_t bytes);
}  // namespace jpgpu

// Pinned staging ring of a context: the caller's (pageable) file bytes are copied into it by the host crew and leave it
// as few large DMAs on the context's upload stream (ref input contract: caller-owned, possibly multi-segment
// ReadOnlySequence<byte>, apps/JpegDecode/MemoryPoolBufferWriter.cs:166-174 -- "the shim linearises into pinned memory").
struct StagingRing {
    static constexpr int kMaxSlots = 16;
    int n_slots = 8;                  // JPGPU_STAGING_SLOTS (8 x 32 MiB: profiles/r02_ingest_sweep.jsonl)
    size_t slot_bytes = 32u << 20;    // JPGPU_STAGING_SLOT_MB; fixed once the first slot exists
    uint8_t *slot[kMaxSlots] = {};
    hipEvent_t drained[kMaxSlots] = {};  // recorded behind the DMA that reads the slot
    uint32_t *verdict = nullptr;      // pinned: per-file results of the ingest verification kernel
    size_t verdict_cap = 0;
    uint8_t *heads = nullptr;         // pinned: the packed heads of the files of a device upload (jpgpu_batch_upload_device)
    size_t heads_cap = 0;
};

struct jpgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;         // kernels of jpgpu_batch_decode and friends
    hipStream_t stream2 = nullptr;        // second half of a large batch in jpgpu_batch_decode (DeviceBatch::decode)
    hipStream_t upload_stream = nullptr;  // H2D of jpgpu_batch_upload: runs beside another batch's decode on `stream`
    // progressive batches too large for one resident launch: the DC scans and every component's AC scans form chains that never
    // touch the same coefficients; each chain's launches go to a stream of its own (DeviceBatch::run_progressive)
    static constexpr int kProgChains = 5;
    hipStream_t prog_stream[kProgChains] = {};
    hipEvent_t prog_ev[kProgChains + 1] = {};
    StagingRing staging;
    int host_threads = 0;                 // crew size of jpgpu_batch_upload; 0 = min(CPUs granted to the process, 16)
    std::string last_error;
    int num_cus = 0;
    uint64_t device_bytes = 0;            // the device's memory: a frame whose output alone is beyond it fails by itself (status 7)
};

namespace jpgpu {

// grow-only device allocation
struct DevBuffer {
    void *ptr = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes);
    void release();
};
// One line of an upload's reservations: `buf` grows to max(bytes, reserve) and, where there are any, takes `bytes` from `src` on the stream.
struct DevUpload {
    DevBuffer *buf;
    const void *src;
    size_t bytes, reserve;
};
// ... and the list of them, in order; *copying says which of the two calls the error is of
template <size_t N>
hipError_t reserve_and_copy(const DevUpload (&ups)[N], hipStream_t stream, bool *copying) {
    for (const DevUpload &u : ups) {
        *copying = false;
        hipError_t e = u.buf->reserve(u.bytes > u.reserve ? u.bytes : u.reserve);
        if (e != hipSuccess) return e;
        *copying = true;
        if (u.bytes && (e = hipMemcpyAsync(u.buf->ptr, u.src, u.bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// What the last jpgpu_batch_upload did (jpgpu_batch_ingest_stats).
struct IngestStats {
    int threads = 0;
    int n_header_only = 0;  // files whose plan came from their headers alone, confirmed by the device
    int n_full_walk = 0;    // files that took the full Identify + Decode marker walks on the host
    float parse_ms = 0, copy_ms = 0, full_walk_ms = 0, layout_ms = 0, total_ms = 0;
    int n_pinned_dma = 0;   // segments DMA'd straight from the caller's page-locked memory
    int n_linearised = 0;   // multi-segment files gathered as a whole on the host
};

enum LumaRoad : uint8_t { kLumaNone = 0, kLumaFast = 1, kLumaScratch = 2 };

struct ImagePlan {
    int status = JPGPU_OK;
    int detail = 0;
    std::string error;
    // a failure of the marker walk BEHIND a scan that was already handed to the scan decoder: the reference only meets it
    // if that scan itself decodes (Decode() runs ProcessScan before it reads the next marker), so it is reported after the
    // device-side status of the scans recorded before it
    int late_status = JPGPU_OK, late_detail = 0;
    bool replay_skip = false;  // replay of the failed progressive frames (replay_failed_progressive): this image is left as it was decoded
    std::string late_error;
    // what the walk ends in instead when scan job `swallow_job` (the file's last sequential scan) leaves exactly one whole
    // byte unread: the reference's reader then resumes one byte INTO the terminating marker (plan_swallowed_terminator)
    int swallow_job = -1, swallow_status = JPGPU_OK, swallow_detail = 0;
    std::string swallow_error;
    uint16_t width = 0, height = 0;
    uint8_t precision = 0, num_components = 0, sof = 0;
    uint32_t restart_interval = 0;
    uint32_t mcus_per_line = 0, mcus_per_column = 0, blocks_per_mcu = 0;
    uint64_t total_blocks = 0;
    uint64_t out_offset = 0, out_bytes = 0;
    uint64_t planes_offset = 0, planes_bytes = 0;  // EXTENDED_U16: the int16 planes K3 writes, in DeviceBatch::d_planes_
    uint64_t coef_offset = 0;
    jpgpu_plane_info plane[4] = {};
    std::vector<int> jobs;     // indices into DeviceBatch::jobs_
    uint64_t file_offset = 0;  // position of the file inside the device input buffer
    size_t file_len = 0;
    // the window the image is decoded through (jpgpu_batch_set_windows): out_bytes and plane[] describe it, width / height stay the frame's.
    // windowed = false: the whole frame (win = {0, 0, width, height}), planned and decoded exactly as without windows
    bool windowed = false;
    jpgpu_rect win = {0, 0, 0, 0};
    // what the image's samples are (common.h: ColorKind): kColorGray / kColorYcbcr unless the batch's colour policy is JPGPU_COLOR_FILE, the
    // format reads it and the file declares otherwise; an image of the other three kinds takes K3's generic class and the K3C launch
    uint8_t color_kind = kColorYcbcr;
    // how the image is turned on its way out (include/jpgpu.h, "Orientation"): 1 = as stored.  exif_orientation is what the file's Exif block
    // says, orientation what the image was planned with (apply_window: the caller's list, the policy, the format).  `win` stays in pixels of
    // the STORED frame, which is what K3 decodes; win_oriented is the same rectangle in the oriented frame, as the caller gave and sees it
    // (equal to win under orientation 1).  An image whose orientation is not 1 takes K3's generic class and the K3O launch.
    uint8_t exif_orientation = 1, orientation = 1;
    jpgpu_rect win_oriented = {0, 0, 0, 0};
    // chroma upsampling (include/jpgpu.h, "Chroma upsampling"): chroma_hs / chroma_vs are what the frame says -- the ratio of components 1 and 2
    // to component 0 where component 0 carries the maximal factors and the two agree, else 0 --, `fancy` what the image was planned with
    // (fancy_filtered: the policy, the format, the kind, the ratio, the width).  A filtered image takes K3's generic class over its FETCH
    // RECTANGLE (fancy_fetch_rect) and the K3U launch; if it is turned as well, K3U leaves its samples in a staging slot for K3O.
    uint8_t chroma_hs = 0, chroma_vs = 0;
    bool fancy = false;
    // grey output (include/jpgpu.h, "Grey output"): kLumaNone = three planes, as ever; under JPGPU_CHANNELS_LUMA and an RGB_PLANAR_* format the
    // image has ONE plane and takes the fast road (kLumaFast: DeviceBatch::luma_fast holds; K3Y's luma_idct_kernel reads its scan's store, and
    // no K3 list names it) or the scratch road (kLumaScratch: planned like an oriented image, K3's generic class, then K3Y's luma_plane_kernel)
    uint8_t luma = kLumaNone;
    // arithmetic (include/jpgpu.h, "Arithmetic"): the image takes libjpeg's integer transform (DeviceBatch::islow_taken holds): planned like a
    // filtered image -- scratch road, dense hand-off --, its scans in K3J's work list and in none of K3's; never on K3Y's fast road
    bool islow = false;
    // scaled decode (include/jpgpu.h, "Scaled decode"): the denominator the image was planned with -- 1, or 2, 4, 8 for an image that takes
    // libjpeg's transform under a scale policy or the fit rule (apply_window) -- and the picture the output stage works on: the frame itself at
    // scale 1, else the reduced picture of ceil(width * m / 8) x ceil(height * m / 8) pixels, m = 8 / scale.  win, win_oriented, out_bytes and
    // plane[] are in pixels of that picture, chroma_hs / chroma_vs the ratio that is LEFT in it (jdmaster's per-component sizes), and the
    // image's scans are in K3R's work list in place of K3J's.  width / height stay the frame's.
    uint8_t scale = 1;
    uint16_t pic_w = 0, pic_h = 0;
};

class WorkCrew;
struct FilePlan;  // device_batch_ingest.cpp
struct FileSegs;  // ingest_host.h

class DeviceBatch {
  public:
    const IngestStats &ingest_stats() const { return ingest_; }
    void plan_stats(jpgpu_plan_stats *st) const;  // jpgpu_batch_plan_stats: the entropy stage's work lists and pools
    void progressive_plan(jpgpu_progressive_plan *p) const;  // jpgpu_batch_progressive_plan
    void idct_work(int32_t counts[kNumIdctLayoutClasses]) const;  // jpgpu_batch_idct_work: K3 work entries per layout class
    void idct_split_work(int32_t counts[kNumIdctLayoutClasses]) const;  // jpgpu_batch_idct_split_work: those of scans handed over as half-line planes
    explicit DeviceBatch(jpgpu_ctx *ctx) : ctx_(ctx) {}
    ~DeviceBatch();

    // Whole files: host parse (Identify + Decode's marker loop) -> plans/jobs -> HBM.
    int upload_files(const uint8_t *const *jpeg, const size_t *len, int n, int format);
    // (the planner of a one-file batch: sequential scans, by ordinal, that leave their reader one byte into the terminating marker)
    void set_forced_swallow(const std::vector<int> &ordinals) { forced_swallow_ = ordinals; }
    // The same for files handed over as lists of segments (the ReadOnlySequence<byte> a reference caller passes to SetInput,
    // JpegDecoder.cs:56-62; multi-segment: apps/JpegDecode/MemoryPoolBufferWriter.cs:166-174): file i is the next
    // segments_per_file[i] entries of `segments`.  flags & JPGPU_UPLOAD_PINNED: every segment lies in page-locked memory
    // (jpgpu_host_alloc / jpgpu_host_register) and is DMA'd to HBM from where it lies -- no staging copy, no crew time.
    int upload_segments(const jpgpu_segment *segments, const int *segments_per_file, int n, int format, unsigned flags);
    // ... and for whole files in device memory of the context's device (jpgpu_batch_upload_device): copied into the input buffer
    // on the device; the host sees their heads, and whole only the files that need the full marker walks.
    int upload_device(const void *const *device_jpeg, const size_t *len, int n, int format);
    const jpgpu_device_ingest_stats &device_ingest_stats() const { return device_ingest_; }
    // The windows of the NEXT upload of whole files (jpgpu_batch_set_windows): consumed by it, accepted or refused.
    int set_windows(const jpgpu_rect *windows, int n);
    int image_window(int i, jpgpu_rect *window) const;
    // The colour policy (jpgpu_batch_set_color_policy): state of the batch, read by every later upload under an RGB format.
    int set_color_policy(int policy);
    int image_color(int i, int *kind) const;
    // The orientation policy (jpgpu_batch_set_orientation_policy): state of the batch like the colour policy; and the orientations of the NEXT
    // upload of whole files (jpgpu_batch_set_orientations): consumed by it like windows.
    int set_orientation_policy(int policy);
    int set_orientations(const uint8_t *orientations, int n);
    int image_orientation(int i, int *orientation) const;
    // The upsampling policy (jpgpu_batch_set_upsampling_policy): state of the batch like the colour policy, read by every later upload of whole
    // files under an RGB format.
    int set_upsampling_policy(int policy);
    int image_upsampling(int i, int *applied) const;
    int upsampling_ms(float *ms);  // jpgpu_batch_upsampling_ms
    // The channels policy (jpgpu_batch_set_channels_policy): state of the batch like the colour policy, read by every later upload of whole
    // files under RGB_PLANAR_U8 / _F16 / _F32.
    int set_channels_policy(int policy);
    int image_channels(int i, int *channels) const;
    int luma_work(int32_t counts[2]) const;  // jpgpu_batch_luma_work
    // The arithmetic policy (jpgpu_batch_set_arithmetic_policy): state of the batch like the colour policy, read by every later upload of whole
    // files under an RGB format.
    int set_arithmetic_policy(int policy);
    int image_arithmetic(int i, int *arithmetic) const;
    // Scaled decode (jpgpu_batch_set_scale_policy / _set_scale_fit / _image_scale): state of the batch like the arithmetic policy.  An image
    // takes a denominator above 1 exactly where it takes libjpeg's transform (islow_taken).
    int set_scale_policy(int denom);
    int set_scale_fit(uint32_t min_w, uint32_t min_h);
    int image_scale(int i, int *denom) const;
    uint64_t idct_listed_mcus() const { return idct_listed_mcus_; }
    // One progressive frame collected by the JpegDecoder mirror: its entropy scans + the Dispose() pass.
    int upload_progressive_frame(const ProgressiveFrame &frame, const uint8_t *file, size_t file_len, int sof, int format);
    // The per-scan boundary (jpgpu_progressive_*): ONE entropy scan of the frame (index into frame.scans()) accumulating into
    // the frame's coefficient store, which lives in d_coefs_ and persists from call to call (same frame, same layout, the
    // buffers only grow); first_scan clears it like JpegBlockAllocator.Allocate does.  Then run_marker_index + run_huffman.
    int upload_progressive_scan(const ProgressiveFrame &frame, int scan_index, bool first_scan);
    // The store as it is now, kept aside (a device copy): what rerun_failed_progressive_scan() starts again from.
    int snapshot_progressive_store();
    // The scan of the last upload_progressive_scan() failed on the device.  The reference's ProcessScan threw at one coefficient
    // and left the store exactly there (JpegHuffmanProgressiveScanDecoder.cs:92-419; Decode()'s finally then disposes it,
    // JpegDecoder.cs:545-549): the store is put back (the snapshot; zero behind a first scan) and the scan issued once more on
    // the kernel that walks and stores coefficient by coefficient, up to the restart interval it failed in.
    int rerun_failed_progressive_scan(bool first_scan);
    // ... and the Dispose() pass alone over that store: the frame job without entropy scans; then run_idct.
    int upload_progressive_dispose(const ProgressiveFrame &frame, int format);
    // One pre-built scan job whose entropy bytes are `entropy` (level-2 API and the JpegDecoder mirror).
    int upload_single_job(const ScanJob &job, int format, const void *initial_output, size_t initial_output_bytes);
    // Coefficient hand-off (progressive / config 5): images described by frame geometry + quantisation tables only.
    int upload_frames(const jpgpu_frame *frames, const uint16_t *qt /*[n][4][64]*/, int n, int format);

    int run_marker_index();
    int run_huffman();
    int run_subseq_sync(const uint32_t **final_state, const uint32_t **first_block);  // K2S rounds + prefix sums only
    int run_idct(bool with_resize = true);  // with_resize = false: decode()'s, which issues K4 behind its last stage event itself
    int run_progressive();     // entropy scans of progressive frames (K2P), ordinal by ordinal
    int decode();  // marker index + the selected pipeline, with stage events
    int sync();    // waits for THIS batch's device work (an event behind its last launch), not for the whole stream

    int size() const { return (int)images_.size(); }
    const ImagePlan *image(int i) const { return (i >= 0 && i < (int)images_.size()) ? &images_[i] : nullptr; }
    int result(int i, jpgpu_image_result *res);
    void *output_device(uint64_t *total) const {
        if (total) *total = out_bytes_;
        return d_out_.ptr;
    }
    void *coefs_device(uint64_t *total_blocks);  // dense int16[blocks][64], whatever form K2 handed the scans over in
    long long debug_split_flags(int i, uint64_t *dst, size_t cap_words);  // tests: the flag words K2 left for image i (-1: not split)
    // tests: what K1 left for scan job k of image i (tests/test_marker_index_gpu.py); -1: the image failed at upload or has no such job
    long long debug_marker_index(int i, int k, uint32_t head[10], uint32_t *ends, uint32_t *ends_u, size_t cap_ends, uint8_t *udata, size_t cap_udata);
    bool debug_k1_onepass() const { return k1_onepass_; }
    int download_output(int i, void *dst, size_t cap);
    int download_coefficients(int i, int16_t *dst, size_t cap_blocks);
    int upload_coefficients(int i, const int16_t *src, size_t nblocks);
    int stage_ms(float ms[4]);
    void totals(uint64_t *compressed, uint64_t *blocks, uint64_t *pixels, uint64_t *out_bytes) const;
    int format() const { return format_; }
    // RGB_PLANAR_F16 / _F32: the constants of the output stage's affine step (common.h: OutputAffine).  Launch state, not part of the plan:
    // they hold from the next decode() / run_idct() on, whatever was uploaded before or is uploaded after.  No other format reads them.
    void set_output_affine(const OutputAffine &a) { output_affine_ = a; }
    // The resize stage (K4, device_batch_resize.cpp): launch state like the constants above.  While one is set, every decode() / run_idct() of an
    // RGB_PLANAR_U8 upload is followed by one launch that resamples every image (its window, if it has one) to out_width x out_height samples
    // of sample_format into one dense [N][3][out_height][out_width] buffer; an upload of another format is refused before anything is enqueued.
    // (0, 0, any format) withdraws it.
    int set_resize(int out_width, int out_height, int sample_format);
    int resized_device(void **ptr, uint64_t *bytes) const;
    int download_resized(int i, void *dst, uint64_t bytes);
    int resize_ms(float *ms);
    void note_entropy_only_request() { in_decode_request_ = false; }
    int last_subseq_rounds() const { return last_subseq_rounds_; }
    int progressive_fallbacks() const { return prog_fallbacks_; }
    int subseq_fallbacks() const { return k2s_fallbacks_; }
    int marker_fallbacks() const { return k1_fallbacks_; }
    int progressive_replays() const { return prog_replays_; }
    void set_partial_flush(bool on) { partial_flush_ = on; }
    // the optimizer path only needs the files, the scan descriptors and the marker index: no coefficient / sample buffers
    void set_entropy_only(bool on) { entropy_only_ = on; }
    void set_preset_restart_intervals(std::vector<int> v) { preset_dri_ = std::move(v); }
    void set_preset_no_subseq(std::vector<uint8_t> v) { preset_no_subseq_ = std::move(v); }

  private:
    friend class OptimizeBatch;
    bool entropy_only_ = false;
    std::vector<int> preset_dri_;  // entropy-only mode: restart interval in force at each file's scan
    std::vector<uint8_t> preset_no_subseq_;  // entropy-only mode: files whose DRI = 0 scan stays on the interval kernel
    int fail(int status, const std::string &msg);
    int hip_fail(hipError_t e, const char *what);
    // files_resident: the files are in d_input_ already (staged by the ingest, or by the upload this one lays out again)
    int layout_and_upload(const std::vector<const uint8_t *> &file_ptr, const std::vector<size_t> &file_len, bool files_resident = false);
    // its stages, in the order they run (device_batch_layout.cpp); UploadPlan is what one stage hands the next
    struct UploadPlan;
    void reset_upload_state(const UploadPlan &p);
    void choose_batch_shapes(UploadPlan &p);
    uint16_t huff_index(UploadPlan &p, const HuffTable &t);
    uint16_t quant_index(const QuantTable &t);
    void plan_image(UploadPlan &p, size_t ii, const std::vector<size_t> &file_len);  // per scan job: the five below
    void fill_scan(UploadPlan &p, size_t ii, int j, size_t file_len);
    void plan_dispose_job(int j, bool listed);
    void plan_progressive_scan(UploadPlan &p, const ImagePlan &img, int j);
    void plan_entropy_work(UploadPlan &p, size_t ii, int j);
    void plan_idct_work(UploadPlan &p, size_t ii, int j, bool overlapping_scans);
    void list_rgb_convert(size_t ii);
    void resolve_offsets(UploadPlan &p);
    void pool_huffman_runs(UploadPlan &p);
    void plan_subseq_lists(UploadPlan &p);
    void assemble_progressive_lists(UploadPlan &p);
    void plan_output_clears();
    void assemble_idct_lists(UploadPlan &p);
    void plan_overlap_halves(UploadPlan &p);
    void init_status();
    int upload_plan(const UploadPlan &p, const std::vector<const uint8_t *> &file_ptr, const std::vector<size_t> &file_len);
    // markers: what the file's headers declare about its colour (none seen: frames, single jobs)
    // exif_orientation: what its Exif block says (1: none seen); recorded here, decided on in apply_window
    void plan_image_geometry(ImagePlan &img, const BaselineGeometry &geo, const ColorMarkers &markers = ColorMarkers(), int exif_orientation = 1) const;
    // bytes an image takes in the output buffer AND in the scratch image, which mirrors its offsets: out_bytes, or the 4 bytes per pixel a
    // CMYK / YCCK image's samples need where that is more (RGB_U8, RGB_PLANAR_U8); an oriented image of any kind passes through the scratch
    // image too, with 1, 3 or 4 bytes per pixel by the same rule
    static uint64_t slot_bytes(const ImagePlan &img);
    // The one decision of the upsampling policy: is this image filtered (its kind, precision, ratio and width; k3u_taps.h has the ratio rule)
    static bool fancy_filtered(int policy, int format, const ImagePlan &img);
    // What K3 leaves in the scratch image of a filtered image: its stored window widened to every tap (k3u_taps.h: k3u_fetch_span), in pixels
    // of the stored frame; and where, behind those samples in the image's slot, K3U stages the samples of an image K3O turns afterwards
    static jpgpu_rect fancy_fetch_rect(const ImagePlan &img);
    static uint64_t fancy_staging_offset(const ImagePlan &img);
    void plan_color_convert();
    void plan_orient_convert();
    void plan_fancy_convert();
    // The one decision between the two roads of a grey image: can K3Y transform component 0's blocks straight from the scan's store (its kind,
    // precision and orientation; ONE sequential scan that names every frame component once, component 0 first and at the frame's maximal
    // factors, its blocks the MCU's first in raster order; no caller's canvas).  jobs: the scan jobs of the image's file plan.
    static bool luma_fast(const ImagePlan &img, const std::vector<ScanJob> &jobs, bool keep_canvas);
    void plan_luma_work(size_t ii, int j);
    // The one decision of the arithmetic policy: does this image take libjpeg's integer transform (K3J) -- the policy, the format, its
    // precision and components, and of every scan job of its file plan: the blocks per MCU, replication by 1, 2 or 4, no component written twice,
    // no overlapping blocks, no literal Dispose(); no caller's canvas.  include/jpgpu.h states the rule.
    static bool islow_taken(int policy, int format, const ImagePlan &img, const std::vector<ScanJob> &jobs, bool keep_canvas);
    void plan_islow_work(size_t ii, int j);
    // The denominator an image that takes libjpeg's transform is decoded with: the fit rule over its oriented frame where one is set, else
    // the policy.  plan_reduced_geometry then turns the image's plan into the reduced picture's (pic_w / pic_h, the residual chroma ratio).
    int scale_wanted(const ImagePlan &img, int orientation) const;
    static void plan_reduced_geometry(ImagePlan &img, const BaselineGeometry &geo, int denom);
    void plan_luma_convert();
    // ingest (jpgpu_batch_upload*), see device_batch_ingest.cpp
    void plan_file_headers(const uint8_t *file, size_t len, FilePlan &fp) const;
    void plan_file_full(const uint8_t *file, size_t len, int index, FilePlan &fp) const;
    void plan_swallowed_terminator(FilePlan &fp, const uint8_t *file, size_t len, bool identify_is_clean) const;
    int begin_ingest(int n, int format);
    int take_windows(int n, int format, const char *what);  // pending windows -> this upload's, or the whole call's refusal
    void apply_window(size_t i, const std::vector<ScanJob> &jobs);                            // image i of merge_plans: its window's verdict and geometry
    void forget_batch();  // no images, no jobs
    int ingest_files(std::vector<FileSegs> &files, unsigned flags, std::chrono::steady_clock::time_point t_begin);
    // its stages, in the order they run (a device source stages in front of plan_heads); IngestRun is what one stage hands the next
    struct IngestRun;
    int plan_heads(IngestRun &r);
    void find_arena_span(IngestRun &r) const;
    int place_files(IngestRun &r);
    int stage_pageable(IngestRun &r);
    int stage_pinned_arena(IngestRun &r);
    int stage_pinned_segments(IngestRun &r);
    int stage_device_gather(IngestRun &r);
    int stage_device_heads(IngestRun &r);
    int confirm_plans(IngestRun &r);
    int verify_plans(const IngestRun &r, const std::vector<int> &spec, std::vector<uint32_t> &first, std::vector<uint32_t> *bytes);
    void demote_unclosed_plans(IngestRun &r) const;
    int finish_plans(IngestRun &r);
    void merge_plans(IngestRun &r);
    int fetch_device_files(std::vector<FileSegs> &files, const std::vector<int> &which);
    // device work of this batch issued since its last sync(): uploads are ordered behind it (an upload right
    // after an un-synced decode must not overwrite what that decode's kernels still read)
    int mark_work();
    int order_upload_behind_work();
    hipEvent_t done_ev_ = nullptr;
    bool work_in_flight_ = false;
    bool whole_files_ = false;     // the last upload was whole files (upload_files / upload_segments): d_input_ holds them as they came
    IngestStats ingest_;
    jpgpu_device_ingest_stats device_ingest_ = {};
    hipEvent_t gather_ev_[2] = {};  // around the gather of a device upload (device_ingest_.gather_ms)
    DevBuffer d_verify_;
    int fetch_status();
    int clear_partial_outputs();
    bool keep_progressive_store_ = false;  // run_progressive: the store holds earlier scans' coefficients (per-scan boundary)
    bool defer_refusal_ = false;           // result(): a frame job's `refuse` is the Dispose() pass's business, not a scan's
    bool keep_canvas_ = false;  // layout of a single scan job over the caller's samples: nothing the scan does not write is touched
    struct OutClear {
        uint64_t first, second;              // (offset, bytes) in the output buffer; the scratch image's slot is slot_bytes long
        uint64_t planes_first, planes_bytes; // EXTENDED_U16: the image's int16 planes
        uint64_t slot_bytes;
    };
    std::vector<OutClear> out_clear_;  // images whose scans leave frame components unwritten

    jpgpu_ctx *ctx_;
    int format_ = JPGPU_FMT_INTERLEAVED_U8;
    OutputAffine output_affine_ = kOutputAffineIdentity;
    // the resize stage: what is set (width 0 = none), the plan made for this upload at that size (descriptors and tap tables, on the device),
    // and what the last launch left in d_resized_ (resized_fmt_ < 0: nothing; cleared by an upload and by a withdrawal)
    struct ResizeSetting {
        int width = 0, height = 0, format = 0;
    } resize_;
    int check_resize_format(const char *who);  // a resize is set and the upload is not RGB_PLANAR_U8: ArgumentException, nothing enqueued
    int run_resize();                          // behind everything K3 has enqueued on the context's stream
    int plan_resize();
    bool resize_plan_valid_ = false;
    int resize_plan_width_ = 0, resize_plan_height_ = 0, n_resize_images_ = 0;
    int resized_width_ = 0, resized_height_ = 0, resized_fmt_ = -1, resized_images_ = 0, resized_planes_ = 3;
    DevBuffer d_resized_, d_resize_images_, d_resize_tables_;
    hipEvent_t resize_ev_[2] = {};
    std::vector<ImagePlan> images_;
    std::vector<ScanJob> jobs_;
    std::vector<int> job_image_;
    std::vector<uint64_t> job_entropy_off_;  // offset of the job's entropy segment inside its file
    std::vector<DevScan> h_scans_;
    std::vector<DevScanStatus> h_status_;
    bool status_valid_ = false;
    std::vector<DevHuffTable> huff_pool_;
    std::vector<DevQuantTable> quant_pool_;
    int n_huff_slots_ = 1;
    // A MIDDLE sequential scan that left one whole byte unread (round 6): the reference resumes its marker walk one byte into the
    // terminating marker, so WHICH scans exist behind it depends on the decode.  The file is planned again with that knowledge and decoded
    // by a batch of its own; its output and result replace the image's (redo_swallowed; cached per image).
    int redo_swallowed(int i, int job, jpgpu_image_result *res);
    std::vector<int> forced_swallow_;
    struct Redo {
        jpgpu_image_result res;
        std::string error;
    };
    std::map<int, Redo> redo_;
    std::vector<SubseqPool> k2_pools_;          // pooled runs of K2 (round 6): entries of d_huff_work_ behind the first n_huff_work_
    uint32_t k2_ticket_base_[kK2MaxPools] = {};  // tickets the earlier launches of this upload drew from each pool's counter (d_k2_tickets_)
    uint32_t k2_tab_bytes_ = 0;  // LDS of the largest table set a sequential scan of the upload stages (K2, the K2S final pass)
    int n_huff_work_ = 0, n_idct_work_ = 0;
    int idct_class_begin_[kNumIdctLayoutClasses + 1] = {};
    std::vector<int> idct_later_begin_;  // d_idct_work_ behind the classes: [k], [k + 1]) = the k-th ordered launch (run_idct)
    // Sequential scans with restart intervals are handed from K2 to K3 as half-line planes (common.h: kScanSplitHandoff; the planner
    // decides per scan, JPGPU_DENSE_HANDOFF=1 keeps every scan dense).  Everything else that reads coefficients wants dense blocks:
    // dense_coefs() expands the split scans into d_dense_ (same offsets; lazily, once per entropy stage).  A caller that uploads
    // coefficients makes the dense copy the batch's store and every scan dense until the next upload of files.
    std::vector<uint32_t> split_scans_;
    uint32_t split_max_blocks_ = 0;
    uint64_t coef_store_blocks_ = 0;  // the coefficient buffer's blocks: total_blocks_ + the padding of split scans
    int idct_split_begin_class_[kNumIdctLayoutClasses] = {};  // d_idct_work_: where the split scans' entries of each class begin
    // The work of windowed images is listed apart (launch_idct_window): d_idct_work_ behind the whole-frame classes, class by class; and every
    // ordered launch [idct_later_begin_[k], [k + 1]) is of one kind, idct_later_win_[k] saying which.
    int idct_win_class_begin_[kNumIdctLayoutClasses + 1] = {};
    std::vector<uint8_t> idct_later_win_;
    uint64_t idct_listed_mcus_ = 0;
    bool windows_pending_ = false;
    std::vector<jpgpu_rect> pending_windows_, windows_;  // set_windows' / the running upload's (empty: whole frames)
    bool dense_valid_ = false, dense_override_ = false;
    DevBuffer d_dense_, d_split_ids_;
    int dense_coefs(const int16_t **ptr);
    int make_store_dense();
    uint64_t total_blocks_ = 0, out_bytes_ = 0, planes_bytes_ = 0, input_bytes_ = 0, compressed_bytes_ = 0, total_pixels_ = 0;
    DevBuffer d_planes_;  // EXTENDED_U16: K3's PLANAR_I16 output, converted by extend_u16_kernel
    DevBuffer d_extend_desc_;
    DevBuffer d_gather_;  // JPGPU_UPLOAD_PINNED: the piece list of gather_pinned_kernel; a device upload: its pieces, files and head lengths
    DevBuffer d_heads_;   // a device upload: the packed heads
    bool in_decode_request_ = false;  // the last entropy stage was issued by decode() (fetch_status's fallback re-issues the same thing)
    uint32_t total_ends_ = 0;

    // DRI = 0 scans: self-synchronising subsequence decode (K2S)
    DevBuffer d_lut_pool_;  // fused lookups of every pool table (K2S round kernel)
    DevBuffer d_sub_work_, d_sub_scan_ids_, d_sub_exit_a_, d_sub_exit_b_, d_sub_nblk_, d_sub_first_, d_sub_entry_, d_sub_dcsum_, d_sub_dcentry_, d_sub_changed_, d_sub_same_, d_sub_perm_;
    DevBuffer d_prog_snapshot_;  // per-scan session: the frame's store in front of the current scan
    uint64_t prog_snapshot_blocks_ = 0;
    DevBuffer d_dispose_;  // DisposeJob per frame that takes the generic Dispose() pass
    std::vector<DisposeJob> dispose_jobs_;
    uint32_t dispose_max_blocks_ = 0;
    int run_dispose_passes(hipStream_t stream);
    // dispose_pass_kernel transforms the stores of the generic-Dispose frames IN PLACE: it runs once per entropy stage / store
    // clear / coefficient upload, a second jpgpu_batch_run_idct (or Dispose of a session) only flushes again
    bool dispose_done_ = false;
    int replay_failed_progressive();
    bool replay_done_ = false, replay_possible_ = false, prog_by_scan_ = false;
    bool replay_layout_active_ = false, in_replay_ = false;  // the work lists are the replay's (failed frames only): the next decode() restores the batch's own
    bool partial_flush_ = true;                               // JPGPU_NO_PARTIAL_FLUSH / jpgpu_batch_set_partial_flush: throughput callers may leave the replay out
    std::vector<std::pair<size_t, ScanJob>> replay_saved_jobs_;  // the jobs the replay rewrote, as they were
    int restore_after_replay();
    int prog_replays_ = 0;
  public:
    int clear_progressive_stores();
  private:
    // K1 in one pass (launch_marker_onepass): the look-back descriptors (tagged, never cleared between decodes), a ticket counter
    // per scan job + the device's give-up word behind them, the host's give-up word in page-locked memory
    DevBuffer d_k1_desc_, d_k1_tickets_, d_k1_order_;
    int n_k1_groups_ = 0;
    uint32_t *h_k1_giveup_ = nullptr;
    uint32_t k1_epoch_ = 0, k1_tag_ = 0;
    bool k1_onepass_ = true;
    int k1_fallbacks_ = 0;
    bool sub_same_valid_ = false;  // d_sub_same_ holds the twins of this upload's subsequences (subseq_same_kernel)
    int n_sub_work_ = 0, n_sub_gather_ = 0, n_sub_scans_ = 0, n_sub_final_work_ = 0, sub_final_spl_ = 2;
    int n_sr_sets_ = 0;  // distinct table sets among the DRI = 0 scans (the K2S round kernel's lookups)
    DevBuffer d_sub_final_work_;
    std::vector<SubseqPool> sub_pools_;  // pooled runs of the final pass: entries of d_sub_final_work_ behind the first n_sub_final_work_
    uint32_t total_subs_ = 0, max_subs_per_scan_ = 0;
    int sub_shift_used_ = 0;  // the subsequence shift of the upload's K2S scans (0 without any): plan_stats
    std::vector<uint32_t> sub_scan_ids_;
    int last_subseq_rounds_ = 0;
    // Device-driven K2S rounds (launch_subseq_sync): the host enqueues a budget of rounds and reads the counts when it next
    // waits for the batch (sync()).  k2s_budget_: rounds the last checked decode of this upload used (0 = not known yet: the
    // first decode takes kSubseqFirstBudget); k2s_unchecked_: such a decode is in flight; k2s_idct_behind_: the output stage
    // was issued behind it (the fallback repeats it too); k2s_host_checked_: the rounds did not suffice once (or
    // JPGPU_SUBSEQ_HOST_CHECK): this upload's decodes take the host-checked loop.
    int k2s_budget_ = 0, k2s_issued_ = 0, k2s_fallbacks_ = 0;
    bool k2s_unchecked_ = false, k2s_idct_behind_ = false, k2s_host_checked_ = false;
    int check_subseq_rounds();
    // progressive frames: work of scan ordinal k is prog_work[prog_begin_[k] .. prog_begin_[k + 1])
    DevBuffer d_prog_work_, d_prog_sync_;  // d_prog_sync_: workgroups of the pipelined launch that have started
    std::vector<int> prog_begin_;
    // ... and the scans with few, long intervals (one wave per interval): prog_work[prog_stream_begin_[k] .. [k + 1])
    std::vector<int> prog_stream_begin_;
    // ... and the pipelined launch's own list: one entry per WAVE (a scan that only follows one cheap scan runs behind it in
    // that scan's wave, DevScan::wave_next): prog_work[prog_pipe_begin_ .. prog_pipe_begin_ + prog_pipe_count_)
    int prog_pipe_begin_ = 0, prog_pipe_count_ = 0;
    // ... and the same stream work once more, grouped by chain (0 = DC scans, 1 + c = the AC scans of frame component c) and by
    // the scan's ordinal inside its frame's chain: prog_work[prog_chain_begin_[x][j] .. [x][j + 1])
    std::vector<int> prog_chain_begin_[jpgpu_ctx::kProgChains];
    bool prog_chains_ok_ = false;
    bool prog_pipelined_ = false;  // all progressive scans are single streams with <= 3 direct dependencies: one launch
    uint32_t prog_spin_budget_ = 1u << 22;  // polls a follower scan may spend in the pipelined launch (JPGPU_PROG_SPIN_BUDGET)
    // what jpgpu_batch_progressive_plan reports beside the lists above: scans planned, the most direct producers of one scan,
    // scans that share their producer's wave, scans per chain; and the launches run_progressive() last took (JPGPU_PROG_LAUNCH_*)
    int prog_scans_ = 0, prog_max_deps_ = 0, prog_wave_tails_ = 0, prog_launch_form_ = 0;
    int prog_chain_scans_[jpgpu_ctx::kProgChains] = {};
    int prog_fallbacks_ = 0;                // times the pipelined launch timed out and the step was re-issued level by level
    std::vector<std::pair<uint64_t, uint64_t>> prog_clear_;  // (first block, blocks) of every progressive frame's store
    // RGB / RGBA output for layouts without a fused conversion: INTERLEAVED_U8 samples in a scratch image first
    struct RgbConvert {
        uint32_t image;
        uint64_t out_offset, pixels;
        int components;
    };
    std::vector<RgbConvert> rgb_convert_;
    DevBuffer d_rgb_scratch_;
    // ... and the images of kind RGB, CMYK and YCCK among them, listed apart: one K3C launch converts them all (plan_color_convert)
    std::vector<RgbConvert> color_convert_;
    std::vector<ColorImage> color_images_;
    uint64_t color_max_pixels_ = 0;
    DevBuffer d_color_images_;
    int color_policy_ = JPGPU_COLOR_YCC;
    // ... and the images whose orientation is not 1, of every kind, in a third list: one K3O launch turns and converts them all (plan_orient_convert)
    std::vector<RgbConvert> orient_convert_;
    std::vector<OrientImage> orient_images_;
    uint32_t orient_max_tiles_ = 0;
    DevBuffer d_orient_images_;
    int orient_policy_ = JPGPU_ORIENT_STORED;
    bool orientations_pending_ = false;
    std::vector<uint8_t> pending_orientations_, orientations_;  // set_orientations' / the running upload's (empty: every image by the policy)
    // ... and the images that are filtered under JPGPU_UPSAMPLE_FANCY, in a fourth list: one K3U call filters and converts them all
    // (plan_fancy_convert); one that is turned as well is in orient_convert_ too, and K3O reads what K3U staged for it
    std::vector<RgbConvert> fancy_convert_;
    std::vector<FancyImage> fancy_images_;
    uint32_t fancy_max_tiles_ = 0;
    int n_fancy_staged_ = 0;
    DevBuffer d_fancy_images_;
    int upsample_policy_ = JPGPU_UPSAMPLE_REPLICATE;
    // JPGPU_TIME_UPSAMPLE=1 (read per upload): an event pair around the K3U call, for jpgpu_batch_upsampling_ms; fancy_timed_: one was recorded
    bool fancy_time_wanted_ = false, fancy_timed_ = false;
    hipEvent_t fancy_ev_[2] = {};
    // ... and the images that have ONE plane under JPGPU_CHANNELS_LUMA: those on the scratch road, of every kind and orientation, in a fifth
    // list of their own and in none of the four above -- one K3Y launch forms and turns them all (plan_luma_convert) --, those on the fast
    // road in K3Y's own work list and in no K3 list (plan_luma_work)
    std::vector<RgbConvert> luma_convert_;
    std::vector<LumaImage> luma_images_;
    std::vector<LumaWork> luma_work_;
    uint32_t luma_max_tiles_ = 0;
    int n_luma_fast_ = 0;
    bool luma_work_windowed_ = false;
    DevBuffer d_luma_images_, d_luma_work_;
    // ... and the scans of the images that take libjpeg's integer transform under JPGPU_ARITHMETIC_LIBJPEG: K3J's own work list, one launch
    // behind K3's (plan_islow_work); the images themselves are in the conversion lists like every image of the scratch road
    std::vector<IslowWork> islow_work_;
    DevBuffer d_islow_work_;
    // ... and those of the images decoded at a reduced size: K3R's work list, one launch behind K3J's
    std::vector<ReducedWork> reduced_work_;
    DevBuffer d_reduced_work_;
    int scale_policy_ = 1;
    uint32_t scale_fit_w_ = 0, scale_fit_h_ = 0;  // the fit rule's least size (0, 0: off)
    int arithmetic_policy_ = JPGPU_ARITHMETIC_REFERENCE;
    bool islow_upload_ = false;  // the last upload of whole files was made under JPGPU_ARITHMETIC_LIBJPEG and an RGB format: libjpeg's colour constants
    YccRgbFactors color_factors() const;  // of this upload's YCbCr -> RGB steps: the reference's, or libjpeg's (islow_upload_)
    int channels_policy_ = JPGPU_CHANNELS_RGB;
    bool luma_upload_ = false;  // the last upload of whole files was made under JPGPU_CHANNELS_LUMA and an RGB_PLANAR_* format: one plane per image
    bool one_plane_upload() const { return luma_upload_ && whole_files_; }  // (what the resize stage sizes its slabs by)
    DevBuffer d_chunk_work_, d_chunk_sums_;
    int n_chunk_work_ = 0;
    DevBuffer d_unstuffed_, d_ends_u_;  // K1 output: entropy data as the bit reader sees it + interval ends in it
    DevBuffer d_input_, d_scans_, d_status_, d_ends_, d_huff_pool_, d_quant_pool_, d_huff_work_, d_idct_work_, d_coefs_, d_out_, d_k2_tickets_;
    DevBuffer d_sr_luts_, d_sr_set_scan_;  // K2S round kernel: its lookups per distinct set of tables (kSrLutSetBytes each), and a scan that stages each set
    // stage events of every decode() since the last stage_ms() query (4 events per decode)
    std::vector<hipEvent_t> ev_pool_;
    size_t ev_used_ = 0;
    std::vector<bool> ev_serial_;  // per decode(): issued serially with stage events (true) or as two overlapped halves
    // decode() in two halves (K2 of the second beside K3 of the first)
    static constexpr int kSerialEvery = 8;
    bool overlap_ok_ = false;
    int decodes_since_query_ = 0;
    int huff_half_ = 0;  // d_huff_work_: where the second half's entries begin
    int idct_half_begin_[2][kNumIdctLayoutClasses + 1] = {};  // d_idct_work_halves_: the classes of each half
    DevBuffer d_idct_work_halves_;
};

}  // namespace jpgpu
