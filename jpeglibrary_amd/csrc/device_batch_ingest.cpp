// jpeglibrary_amd/csrc/device_batch_ingest.cpp -- jpgpu_batch_upload*, the front door of every decode: the host-side plans of a file
// (header-only / full marker walks), the crew's size, the upload entries for files in pageable, page-locked and device memory, and
// DeviceBatch::ingest_files, a list of stages around an IngestRun, which ends in layout_and_upload (device_batch_layout.cpp).
// (One file with device_batch.cpp until the ingest was cut into stages; ingest_host.h has what needs no device.)
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

#include "device_batch.h"
#include "host_pool.h"
#include "ingest_host.h"
#include "kernels.h"

namespace jpgpu {

static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// The largest file the ingest takes: a larger one is refused by the full path before it reads a byte, and gets no slot.
constexpr size_t kMaxFileBytes = 0x7FFFFFF0u;

// Planner: what JpegScanDecoder.Create / ProcessScan become while the batch is being laid out.
namespace {

class PlanHandler final : public ScanHandler {
  public:
    explicit PlanHandler(std::vector<ScanJob> *jobs, bool first_scan_only = false, const std::vector<int> *forced = nullptr)
        : jobs_(jobs), first_scan_only_(first_scan_only), forced_(forced) {}
    // Second walk of a file whose sequential scans are already planned (`ends` = where each one's data stops): nothing is
    // recorded, and scan number `swallow` leaves the reader ONE byte into its terminating marker.  That is where the
    // reference's reader stands when exactly one whole byte was left in the bit reader behind the last block: the marker
    // has been pulled into the bit reader, TryPeekMarker() only shows it once the buffer is empty, so the two bytes are
    // not given back (ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:167-176, JpegBitReader.cs:152-155).
    PlanHandler(const std::vector<size_t> *ends, int swallow) : jobs_(nullptr), replay_ends_(ends), swallow_(swallow) {}
    const std::vector<size_t> &sequential_ends() const { return ends_; }
    void on_frame(HostDecoder &dec, int sof) override {
        sof_ = sof;
        baseline_ = false;
        flush_progressive();  // a second SOF replaces the scan decoder: the old one is disposed first (JpegDecoder.cs:568)
        if (sof == kSOF0 || sof == kSOF1) {
            geo_ = BaselineGeometry::latch(dec, dec.frame_header());  // DRI latched at SOF time
            baseline_ = true;
        } else if (sof == kSOF2) {
            prog_.begin(dec, dec.frame_header());
        }
    }
    void on_scan(HostDecoder &dec, MarkerReader &reader, const ScanHeader &scan) override {
        const uint8_t *entropy = reader.remaining_bytes();
        const size_t len = (size_t)reader.remaining_byte_count();
        if (prog_.active()) {
            prog_.add_scan(dec, scan, entropy, len);  // the reference leaves the outer reader where it is
            return;
        }
        if (!baseline_)
            throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "Only Huffman DCT frames (SOF0, SOF1, SOF2) run on this path.", kDetailUnsupportedFrame);
        if (scan.num_components == 0) {
            // A scan header that names no component: ProcessScan walks the MCUs without reading a bit (:99-136).  With a
            // restart interval the first restart check finds the bit buffer full and no marker (:139-154); without one
            // the reader is left where it is and the outer walk skips the entropy data as fill.
            const uint64_t mcus = (uint64_t)geo_.mcus_per_line * (uint64_t)geo_.mcus_per_column;
            if (geo_.restart_interval != 0 && mcus >= geo_.restart_interval && len != 0 &&
                !(len >= 2 && entropy[0] == 0xFF && entropy[1] != 0x00 && entropy[1] != 0xFF))
                throw DecodeError(JPGPU_ERR_INVALID_OPERATION, "Expect restart marker.", kDetailExpectRestart);
            if (first_scan_only_)
                throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "A scan without components is not supported by the optimizer path.", kDetailUnsupportedFrame);
            if (geo_.restart_interval != 0 && mcus >= geo_.restart_interval)
                throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "A scan without components in front of restart markers is not supported.", kDetailUnsupportedFrame);
            reader.try_advance((int)find_scan_end(entropy, len));
            return;
        }
        if (replay_ends_) {
            const int k = replayed_++;
            if (k > swallow_ || k >= (int)replay_ends_->size())
                throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "A scan behind a scan that left one byte unread is not supported.", kDetailUnsupportedFrame);
            reader.try_advance((int)(*replay_ends_)[k] + (k == swallow_ ? 1 : 0));
            return;
        }
        jobs_->push_back(make_scan_job(dec, geo_, scan, entropy, len, first_scan_only_));
        if (!first_scan_only_) {
            // (a scan KNOWN to leave one whole byte unread -- the device said so in the batch this plan is made for -- hands the
            // reader back one byte into its terminating marker, the way the reference's does: DeviceBatch::redo_swallowed)
            const bool forced = forced_ != nullptr && std::find(forced_->begin(), forced_->end(), (int)ends_.size()) != forced_->end();
            ends_.push_back(find_scan_end(entropy, len));
            jobs_->back().forced_swallow = forced && ends_.back() < len;
            reader.try_advance((int)ends_.back() + (jobs_->back().forced_swallow ? 1 : 0));
            return;
        }
        // leave the reader just before the next non-RST marker, like ProcessScan does (:167-176); the optimizer path only
        // wants the scan resolved (what follows it is its own marker walk's business): nothing is left to read
        reader.try_advance(first_scan_only_ ? (int)len : (int)find_scan_end(entropy, len));
    }
    void on_dispose(HostDecoder &) override { flush_progressive(); }
    const BaselineGeometry &geo() const { return prog_geo_valid_ ? prog_geo_ : geo_; }
    int sof() const { return sof_; }

  private:
    // Dispose() of the progressive scan decoder: the frame's IDCT pass, then its entropy scans in file order
    void flush_progressive() {
        if (!prog_.active()) return;
        if (jobs_) {  // (also without a single recorded scan: Dispose() still flushes the allocator's blocks)
            jobs_->push_back(prog_.make_frame_job());
            for (ScanJob &j : prog_.scans()) jobs_->push_back(std::move(j));
            prog_geo_ = prog_.geo();
            prog_geo_valid_ = true;
        }
        prog_.reset();
    }
    std::vector<ScanJob> *jobs_;
    std::vector<size_t> ends_;
    const std::vector<size_t> *replay_ends_ = nullptr;
    int swallow_ = -1, replayed_ = 0;
    bool first_scan_only_ = false;
    const std::vector<int> *forced_ = nullptr;  // sequential scans (by ordinal) known to leave one byte unread: DeviceBatch::redo_swallowed
    BaselineGeometry geo_, prog_geo_;
    bool prog_geo_valid_ = false;
    ProgressiveFrame prog_;
    bool baseline_ = false;
    int sof_ = 0;
};
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- ingest
//
// jpgpu_batch_upload = SetInput + Identify + Decode's marker loop for n files (ref: JpegDecoder.cs:75-162, 509-617), without
// the host ever walking entropy-coded bytes in the common case:
//   1. header-only plan, one file per crew thread: Identify's walk up to the first SOS header, then Decode's walk up to the
//      same point; the file is planned as "this one sequential scan, its data closed by EOI" (FastPlanHandler);
//   2. the files go to HBM through the context's pinned staging ring: the crew copies the caller's bytes into 32 MiB slots,
//      every full slot leaves as one DMA on the upload stream while the next ones are being filled;
//   3. the device reads the bytes behind each SOS header once (first_marker_kernel) and reports the first marker that is
//      not RSTn: where that is EOI, Identify and Decode would have seen nothing else either (neither looks behind EOI) and
//      the plan stands -- including Identify's "last DRI in the file" (every DRI lay in front of the SOS);
//   4. every other file (several scans, progressive, tables or garbage behind the scan, truncated data, a Decode-walk
//      failure that a later Identify failure would pre-empt) takes the full walk of both loops, also on the crew.

namespace {
struct NeedFullWalk {};  // the header-only planner met something that is not "headers, one sequential scan"

class FastPlanHandler final : public ScanHandler {
  public:
    explicit FastPlanHandler(std::vector<ScanJob> *jobs) : jobs_(jobs) {}
    void on_frame(HostDecoder &dec, int sof) override {
        if (sof != kSOF0 && sof != kSOF1) throw NeedFullWalk{};
        geo_ = BaselineGeometry::latch(dec, dec.frame_header());  // DRI latched at SOF time
    }
    void on_scan(HostDecoder &dec, MarkerReader &reader, const ScanHeader &scan) override {
        if (scan.num_components == 0) throw NeedFullWalk{};
        const uint8_t *entropy = reader.remaining_bytes();
        const size_t len = (size_t)reader.remaining_byte_count();
        jobs_->push_back(make_scan_job(dec, geo_, scan, entropy, len, false));
        reader.try_advance((int)len);  // the plan: nothing but this scan's data and an EOI follow (checked on the device)
    }
    void on_dispose(HostDecoder &) override {}

  private:
    std::vector<ScanJob> *jobs_;
    BaselineGeometry geo_;
};
}  // namespace

struct FilePlan {
    ImagePlan img;
    std::vector<ScanJob> jobs;
    std::vector<size_t> seq_ends;  // where each sequential scan's data stops (offset from the scan's first entropy byte)
    bool speculative = false;      // header-only plan, waiting for the device's verdict
    bool need_full = false;
    size_t scan_data_pos = 0;      // offset of the first entropy byte in the file (speculative plans)
};

// Identify + Decode's marker loop over the whole file (both walk the entropy bytes): the general path.
void DeviceBatch::plan_file_full(const uint8_t *file, size_t len, int index, FilePlan &fp) const {
    fp.jobs.clear();
    fp.seq_ends.clear();
    fp.speculative = false;
    fp.img = ImagePlan();
    ImagePlan &img = fp.img;
    img.file_len = len;
    bool decoding = false;  // Identify() is over, Decode()'s marker loop is running
    HostDecoder dec;
    PlanHandler handler(&fp.jobs, entropy_only_, forced_swallow_.empty() ? nullptr : &forced_swallow_);
    try {
        if (len > kMaxFileBytes) throw DecodeError(JPGPU_ERR_NOT_SUPPORTED, "JPEG streams of 2 GiB or more are not supported.");
        dec.set_input(file, len);
        if (entropy_only_) {
            // optimizer path: JpegOptimizer.Scan() runs no Identify(); the restart interval is the one in force at the
            // scan (OptimizeBatch::plan_file found it) unless a DRI segment in front of the frame header says otherwise
            if ((size_t)index < preset_dri_.size()) dec.set_restart_interval(preset_dri_[index]);
        } else {
            dec.identify(false);  // every reference caller runs Identify before Decode; it latches the LAST DRI (F4)
        }
        img.sof = (uint8_t)dec.start_of_frame();
        decoding = true;
        try {
            dec.decode(handler, true);
        } catch (...) {
            fp.seq_ends = handler.sequential_ends();
            throw;
        }
        decoding = false;
        if (entropy_only_) img.sof = (uint8_t)dec.start_of_frame();
        if (fp.jobs.empty()) {
            // no scan: Decode() succeeds without writing anything; keep the frame geometry for the caller
            if (img.sof == kSOF0 || img.sof == kSOF1 || img.sof == kSOF2) plan_image_geometry(img, BaselineGeometry::latch(dec, dec.frame_header()), dec.color_markers(), dec.exif_orientation());
        } else {
            plan_image_geometry(img, fp.jobs[0].geo, dec.color_markers(), dec.exif_orientation());
            img.blocks_per_mcu = (uint32_t)fp.jobs[0].blocks_per_mcu;
        }
        fp.seq_ends = handler.sequential_ends();
    } catch (const DecodeError &e) {
        // the scans of a progressive frame recorded before the walk failed ran in the reference too (each ProcessScan
        // decodes its scan on the spot): they are kept so that their own failures come first
        if (decoding && e.status != JPGPU_ERR_NOT_SUPPORTED) {
            try {
                handler.on_dispose(dec);
            } catch (const DecodeError &) {
            }
        }
        const bool keep = decoding && !fp.jobs.empty() && e.status != JPGPU_ERR_NOT_SUPPORTED;
        if (keep) {
            // scans handed to the scan decoder before the walk failed: they run, the failure is reported behind them
            img.late_status = e.status;
            img.late_detail = e.detail;
            img.late_error = e.what();
            try {
                plan_image_geometry(img, fp.jobs[0].geo, dec.color_markers(), dec.exif_orientation());
                img.blocks_per_mcu = (uint32_t)fp.jobs[0].blocks_per_mcu;
            } catch (const DecodeError &e2) {
                fp.jobs.clear();
                img.status = e2.status;
                img.detail = e2.detail;
                img.error = e2.what();
            }
        } else {
            fp.jobs.clear();
            img.status = e.status;
            img.detail = e.detail;
            img.error = e.what();
        }
    }
    if (!entropy_only_ && img.status == JPGPU_OK) plan_swallowed_terminator(fp, file, len, false);
}

// Headers only: both marker loops up to the first SOS header, the scan planned as the file's only one.
void DeviceBatch::plan_file_headers(const uint8_t *file, size_t len, FilePlan &fp) const {
    fp.jobs.clear();
    fp.seq_ends.clear();
    fp.speculative = fp.need_full = false;
    fp.img = ImagePlan();
    ImagePlan &img = fp.img;
    img.file_len = len;
    if (entropy_only_ || len > kMaxFileBytes || !forced_swallow_.empty()) {
        fp.need_full = true;  // optimizer walks have rules of their own; oversize files are refused by the full path; a re-plan walks the file
        return;
    }
    HostDecoder dec;
    try {
        dec.set_input(file, len);
        if (!dec.identify_until_scan(false, &fp.scan_data_pos)) {
            fp.need_full = true;  // no scan in the file: the walk just done WAS the whole Identify; let the general path plan it
            return;
        }
        if (!dec.has_frame_header()) {
            fp.need_full = true;  // SOS in front of any SOF: Identify's verdict depends on what follows the scan
            return;
        }
    } catch (const DecodeError &e) {
        // Identify fails in front of the first scan: that is what the caller sees, whatever follows
        img.status = e.status;
        img.detail = e.detail;
        img.error = e.what();
        return;
    }
    img.sof = (uint8_t)dec.start_of_frame();
    try {
        FastPlanHandler handler(&fp.jobs);
        dec.decode(handler, true);
        if (fp.jobs.size() != 1) throw NeedFullWalk{};
        plan_image_geometry(img, fp.jobs[0].geo, dec.color_markers(), dec.exif_orientation());
        img.blocks_per_mcu = (uint32_t)fp.jobs[0].blocks_per_mcu;
        fp.speculative = true;
    } catch (const NeedFullWalk &) {
        fp.need_full = true;
    } catch (const DecodeError &) {
        // Decode's loop fails before the scan is planned -- but Identify walks the WHOLE file first, and a failure of
        // its own behind the scan would be the one the caller sees: only the full walk can tell
        fp.need_full = true;
    }
    if (fp.need_full) fp.jobs.clear();
}

// What Decode() ends in when the LAST sequential scan of the file leaves its reader one byte into the terminating marker.
// identify_is_clean: the header-only path already knows that Identify() succeeds (and what it latched lies in front of
// the first SOS): its walk over the entropy data is not repeated.
void DeviceBatch::plan_swallowed_terminator(FilePlan &fp, const uint8_t *file, size_t len, bool identify_is_clean) const {
    ImagePlan &img = fp.img;
    img.swallow_status = JPGPU_OK;
    img.swallow_detail = 0;
    img.swallow_error.clear();
    img.swallow_job = -1;
    const std::vector<size_t> &ends = fp.seq_ends;
    if (ends.empty() || fp.jobs.empty()) return;
    int last = -1, n_seq = 0;
    for (size_t j = 0; j < fp.jobs.size(); j++)
        if (fp.jobs[j].kind == kScanSequential) {
            last = (int)j;
            n_seq++;
        }
    if (last < 0 || n_seq != (int)ends.size() || ends.back() >= fp.jobs[last].entropy_len) return;  // no marker behind it
    img.swallow_job = last;  // index into fp.jobs; upload_files turns it into a batch job index
    if (identify_is_clean && n_seq == 1 && (size_t)(fp.jobs[last].entropy - file) + ends.back() + 2 == len) {
        // The EOI closes the file (every clean file): the replayed walk would step over the scan to one byte into the
        // marker, find a single byte left and fail in TryReadMarker (JpegDecoder.cs:533-537).  Written down directly: a
        // thousand exceptions thrown from a crew of threads serialise on the unwinder's lock.
        img.swallow_status = JPGPU_ERR_INVALID_DATA;
        img.swallow_detail = kDetailBadHeader;
        img.swallow_error = "Failed to decode JPEG data at offset " + std::to_string(len - 1) + ". No marker found.";
        return;
    }
    try {
        HostDecoder dec;
        dec.set_input(file, len);
        if (identify_is_clean) {
            size_t pos;
            (void)dec.identify_until_scan(false, &pos);
        } else {
            dec.identify(false);
        }
        PlanHandler replay(&ends, n_seq - 1);
        dec.decode(replay, true);
    } catch (const DecodeError &e) {
        img.swallow_status = e.status;
        img.swallow_detail = e.detail;
        img.swallow_error = e.what();
    }
}

// Crew size when the caller did not choose one: the CPUs this process may really use -- the affinity mask and the cgroup
// CPU quota (v2 cpu.max, v1 cpu.cfs_quota_us) both bound it (a container often reports the machine's 256 threads and is
// granted 16) -- capped at 16.
int granted_host_cpus() {
    unsigned cpus = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) cpus = std::min(cpus, (unsigned)CPU_COUNT(&set));
    bool have_quota = false;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
        char q[32] = {0};
        long period = 0;
        if (fscanf(f, "%31s %ld", q, &period) == 2 && period > 0) {
            have_quota = true;
            if (strcmp(q, "max") != 0) {
                const long quota = atol(q);
                if (quota > 0) cpus = std::min(cpus, (unsigned)std::max(1L, (quota + period - 1) / period));
            }
        }
        fclose(f);
    }
    if (!have_quota) {  // cgroup v1: cpu.cfs_quota_us (-1 = unlimited) / cpu.cfs_period_us
        long quota = -1, period = 0;
        if (FILE *f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
            if (fscanf(f, "%ld", &quota) != 1) quota = -1;
            fclose(f);
        }
        if (FILE *f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (fscanf(f, "%ld", &period) != 1) period = 0;
            fclose(f);
        }
        if (quota > 0 && period > 0) cpus = std::min(cpus, (unsigned)std::max(1L, (quota + period - 1) / period));
    }
    return (int)cpus;
}
int default_host_threads() {
    if (const char *ev = getenv("JPGPU_HOST_THREADS")) return std::max(1, atoi(ev));
    return std::min(16, granted_host_cpus());  // a handful of threads already keep the host link busy (profiles/r02_ingest_sweep.jsonl)
}

// jpgpu_batch_set_windows: the windows of the next upload of whole files
int DeviceBatch::set_windows(const jpgpu_rect *windows, int n) {
    if (n < 0 || (n > 0 && !windows)) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_set_windows: bad argument");
    pending_windows_.assign(windows, windows + n);
    windows_pending_ = n > 0;
    return JPGPU_OK;
}

int DeviceBatch::image_window(int i, jpgpu_rect *window) const {
    const ImagePlan *img = image(i);
    if (!img || !window) return JPGPU_ERR_ARGUMENT;
    *window = img->win_oriented;  // (as the caller gave it: in pixels of the oriented frame)
    return JPGPU_OK;
}

// What every upload of whole files starts with: the pending windows become this upload's and nobody else's.  The refusals of the whole
// call, decided before anything is enqueued; they leave the batch empty.
int DeviceBatch::take_windows(int n, int format, const char *what) {
    luma_upload_ = channels_policy_ == JPGPU_CHANNELS_LUMA && fmt_is_rgb_planes(format);  // (this upload's images have one plane each)
    islow_upload_ = arithmetic_policy_ == JPGPU_ARITHMETIC_LIBJPEG && fmt_is_rgb(format);  // (this upload's colour steps take libjpeg's constants)
    windows_.clear();
    orientations_.clear();
    if (!windows_pending_ && !orientations_pending_) return JPGPU_OK;
    const bool with_windows = windows_pending_, with_orientations = orientations_pending_;
    windows_.swap(pending_windows_);
    orientations_.swap(pending_orientations_);
    pending_windows_.clear();
    pending_orientations_.clear();
    windows_pending_ = orientations_pending_ = false;
    const char *why = nullptr;
    if (with_windows && (int)windows_.size() != n) why = ": the upload's n differs from the windows' n (jpgpu_batch_set_windows)";
    else if (with_windows && (format < 0 || format >= kNumOutputFormats || !fmt_is_interleaved(format)))
        why = ": windows (jpgpu_batch_set_windows) need a whole-pixel format; PLANAR_U8, PLANAR_I16 and EXTENDED_U16 have none";
    else if (with_orientations && (int)orientations_.size() != n) why = ": the upload's n differs from the orientations' n (jpgpu_batch_set_orientations)";
    else if (with_orientations && (format < 0 || format >= kNumOutputFormats || !fmt_is_rgb(format)))
        why = ": orientations (jpgpu_batch_set_orientations) need an RGB format; the sample and the planar formats decode as stored";
    if (!with_windows) windows_.clear();
    if (!with_orientations) orientations_.clear();
    if (!why) return JPGPU_OK;
    windows_.clear();
    orientations_.clear();
    forget_batch();
    whole_files_ = replay_possible_ = false;
    return fail(JPGPU_ERR_ARGUMENT, std::string(what) + why);
}

// Image i behind its plan: its orientation -- the caller's value, else what the policy makes of the file's, and 1 under a format that does
// not read it -- then the verdict on its window, which is given in pixels of the ORIENTED frame, and the geometry of the output in place of
// the stored frame's; and whether it is filtered under the upsampling policy.  A window that is the whole frame is no window.  An image that failed keeps its status; an image of orientation 1
// without a window leaves here exactly as its plan made it.
// Under JPGPU_CHANNELS_LUMA and an RGB_PLANAR_* format the image has one plane, and `jobs` (the scan jobs of its file plan) decide its road.
void DeviceBatch::apply_window(size_t i, const std::vector<ScanJob> &jobs) {
    ImagePlan &img = images_[i];
    if (img.status != JPGPU_OK) return;
    int o = 1;
    if (fmt_is_rgb(format_)) {
        const int given = orientations_.empty() ? 0 : orientations_[i];
        o = given != 0 ? given : (orient_policy_ == JPGPU_ORIENT_FILE ? img.exif_orientation : 1);
    }
    img.orientation = (uint8_t)o;
    const bool one_plane = channels_policy_ == JPGPU_CHANNELS_LUMA && fmt_is_rgb_planes(format_);
    // (an image that takes libjpeg's transform is never on K3Y's fast road, which runs K3's: its grey plane comes from the scratch slot K3J fills)
    img.islow = islow_taken(arithmetic_policy_, format_, img, jobs, keep_canvas_ || entropy_only_);
    img.luma = !one_plane ? kLumaNone : (!img.islow && luma_fast(img, jobs, keep_canvas_) ? kLumaFast : kLumaScratch);
    // (... and it alone is decoded at a reduced size: from here on the picture is the reduced one, include/jpgpu.h "Scaled decode")
    if (const int denom = img.islow ? scale_wanted(img, o) : 1; denom > 1) plan_reduced_geometry(img, jobs.front().geo, denom);
    img.fancy = fancy_filtered(upsample_policy_, format_, img);  // (the window only decides which of its pixels come out; never a grey image)
    const uint32_t ow = orientation_transposes(o) ? img.pic_h : img.pic_w, oh = orientation_transposes(o) ? img.pic_w : img.pic_h;  // the oriented frame
    jpgpu_rect w = windows_.empty() ? jpgpu_rect{0, 0, 0, 0} : windows_[i];
    bool whole = w.x == 0 && w.y == 0 && w.width == 0 && w.height == 0;
    if (!whole) {
        const bool inside = (uint64_t)w.x + w.width <= ow && (uint64_t)w.y + w.height <= oh;
        if (!inside || w.width == 0 || w.height == 0) {  // (outside the frame, or no pixels: this image alone fails)
            img.status = JPGPU_ERR_ARGUMENT;
            img.detail = kDetailNone;
            img.error = "The window {" + std::to_string(w.x) + ", " + std::to_string(w.y) + ", " + std::to_string(w.width) + ", " + std::to_string(w.height) +
                        "} does not lie inside the " + std::to_string(ow) + " x " + std::to_string(oh) + " frame, or is empty.";
            img.out_bytes = 0;
            memset(img.plane, 0, sizeof img.plane);
            return;
        }
        whole = w.x == 0 && w.y == 0 && w.width == ow && w.height == oh;
    }
    if (whole) w = jpgpu_rect{0, 0, ow, oh};
    img.win_oriented = w;
    if (whole && o == 1 && !one_plane && img.scale == 1) return;
    if (!whole) {
        img.windowed = true;
        img.win = orientation_stored_rect(o, w, img.pic_w, img.pic_h);  // what K3 decodes
    }
    const uint64_t pixels = (uint64_t)w.width * w.height;
    if (fmt_is_sample_bytes(format_)) {
        img.out_bytes = pixels * img.num_components;
    } else if (one_plane) {  // ONE tight plane of the oriented frame or of its window
        img.out_bytes = pixels * fmt_rgb_plane_sample_bytes(format_);
        memset(img.plane, 0, sizeof img.plane);
        img.plane[0] = jpgpu_plane_info{0, w.width, w.height, w.width};
    } else {  // (the RGB formats: take_windows admits nothing else)
        img.out_bytes = pixels * (format_ == JPGPU_FMT_RGBA_U8 ? 4 : 3) * fmt_rgb_plane_sample_bytes(format_);
        if (fmt_is_rgb_planes(format_))
            for (int c = 0; c < 3; c++) img.plane[c] = jpgpu_plane_info{(uint64_t)c * pixels * fmt_rgb_plane_sample_bytes(format_), w.width, w.height, w.width};
    }
}

int DeviceBatch::upload_files(const uint8_t *const *jpeg, const size_t *len, int n, int format) {
    if (n < 0 || (n > 0 && (!jpeg || !len))) {
        pending_windows_.clear();  // (consumed by this upload, refused as it is)
        pending_orientations_.clear();
        windows_pending_ = orientations_pending_ = false;
        return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload: null argument");
    }
    std::vector<jpgpu_segment> segs((size_t)n);
    std::vector<int> per((size_t)n, 1);
    for (int i = 0; i < n; i++) segs[(size_t)i] = {jpeg[i], len[i]};
    return upload_segments(segs.data(), per.data(), n, format, 0);
}

int DeviceBatch::upload_segments(const jpgpu_segment *segments, const int *segments_per_file, int n, int format, unsigned flags) {
    if (const int wrc = take_windows(n, format, "jpgpu_batch_upload"); wrc != JPGPU_OK) return wrc;
    if (n < 0 || (n > 0 && (!segments || !segments_per_file))) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload: null argument");
    if (format < 0 || format >= kNumOutputFormats) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload: unknown format");
    if (flags & ~(JPGPU_UPLOAD_PINNED | JPGPU_UPLOAD_PINNED_ARENA)) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload_segments: unknown flag");
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    int rc = begin_ingest(n, format);
    if (rc != JPGPU_OK) return rc;
    std::vector<FileSegs> files((size_t)n);
    {
        const jpgpu_segment *sp = segments;
        for (int i = 0; i < n; i++) {
            FileSegs &f = files[(size_t)i];
            if (segments_per_file[i] < 0) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload_segments: negative segment count");
            f.seg = sp;
            f.n = segments_per_file[i];
            sp += f.n;
            for (int k = 0; k < f.n; k++) {
                if (f.seg[k].len && !f.seg[k].data) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload: null segment");
                f.len += f.seg[k].len;
            }
            if (f.n == 1) {
                f.base = f.seg[0].data;
                f.base_len = f.len;
            }
        }
    }
    return ingest_files(files, flags, t_begin);
}

// What every upload of whole files starts with: the batch forgets its images and jobs, the upload stream waits for the batch's
// unsynchronised device work.
int DeviceBatch::begin_ingest(int n, int format) {
    ingest_ = IngestStats();
    device_ingest_ = jpgpu_device_ingest_stats();
    hipError_t e = hipSetDevice(ctx_->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    int rc = order_upload_behind_work();
    if (rc != JPGPU_OK) return rc;
    format_ = format;
    forget_batch();
    images_.assign((size_t)n, ImagePlan());
    return JPGPU_OK;
}

void DeviceBatch::forget_batch() {
    images_.clear();
    jobs_.clear();
    job_image_.clear();
    job_entropy_off_.clear();
}

// jpgpu_batch_upload for whole files that lie in device memory of the context's device (include/jpgpu.h, 1b).
int DeviceBatch::upload_device(const void *const *device_jpeg, const size_t *len, int n, int format) {
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    if (const int wrc = take_windows(n, format, "jpgpu_batch_upload_device"); wrc != JPGPU_OK) {
        device_ingest_ = jpgpu_device_ingest_stats();
        return wrc;
    }
    auto refuse = [&](const std::string &why) {
        forget_batch();
        whole_files_ = replay_possible_ = false;
        device_ingest_ = jpgpu_device_ingest_stats();
        return fail(JPGPU_ERR_ARGUMENT, "jpgpu_batch_upload_device: " + why);
    };
    if (n < 0 || (n > 0 && (!device_jpeg || !len))) return refuse("null argument");
    if (format < 0 || format >= kNumOutputFormats) return refuse("unknown format");
    hipError_t e = hipSetDevice(ctx_->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    std::vector<FileSegs> files((size_t)n);
    for (int i = 0; i < n; i++) {
        FileSegs &f = files[(size_t)i];
        f.device = true;
        f.len = len[i];
        if (f.len == 0) continue;  // the empty file: its pointer is not looked at
        f.dev = (const uint8_t *)device_jpeg[i];
        const std::string which = "file " + std::to_string(i);
        if (!f.dev) return refuse(which + ": null pointer");
        const int where = check_device_range(ctx_->device, f.dev, f.len);
        if (where == 1) return refuse(which + " is not in device memory of the context's device");
        if (where == 2) return refuse(which + ": " + std::to_string(f.len) + " bytes do not lie inside one device allocation");
    }
    const int rc = begin_ingest(n, format);
    if (rc != JPGPU_OK) return rc;
    return ingest_files(files, 0, t_begin);
}

int check_device_range(int device, const void *p, size_t bytes) {
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof attr);
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) (void)hipGetLastError();  // (host memory the runtime has never seen: an error of this query, not of the stream)
    if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != device) return 1;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p);
    if (e != hipSuccess) (void)hipGetLastError();
    const uintptr_t lo = (uintptr_t)base, at = (uintptr_t)p;
    if (e != hipSuccess || at < lo || at - lo > size || bytes > size - (at - lo)) return 2;
    return 0;
}

// What the stages of ingest_files hand one another: the files and their plans, the crew, what the flags ask for, and the clock.
// (What the decode and the results read afterwards is a member of DeviceBatch.)
struct DeviceBatch::IngestRun {
    using clk = std::chrono::steady_clock;
    std::vector<FileSegs> &files;
    std::vector<FilePlan> plans;
    const int n;
    const unsigned flags;
    const bool device, pinned;  // the source: device memory; page-locked host memory (scattered, or one arena)
    const uint64_t total_bytes;
    WorkCrew crew;
    std::pair<const uint8_t *, size_t> arena_span = {nullptr, 0};  // JPGPU_UPLOAD_PINNED_ARENA: the span the device copy mirrors
    std::atomic<int> n_linearised{0};
    // a device source, between the two halves of its staging: what the first left in d_gather_ and brought back of it
    const DeviceFile *d_files = nullptr;
    uint64_t *d_head_off = nullptr;
    uint32_t *d_head_len = nullptr;
    std::vector<uint64_t> head_off;  // [n + 1]: where each head lies in the packed heads; [n] = their total
    std::vector<uint32_t> head_len;
    float device_stage_ms = 0;
    std::vector<const uint8_t *> file_ptr;  // merge_plans: what layout_and_upload is given
    std::vector<size_t> file_len;
    clk::time_point t0;

    IngestRun(std::vector<FileSegs> &f, unsigned fl, int want_threads)
        : files(f), plans(f.size()), n((int)f.size()), flags(fl), device(!f.empty() && f[0].device),
          pinned((fl & (JPGPU_UPLOAD_PINNED | JPGPU_UPLOAD_PINNED_ARENA)) != 0), total_bytes(sum_of_lengths(f)),
          crew(size_crew(want_threads, n, total_bytes)) {}
    static uint64_t sum_of_lengths(const std::vector<FileSegs> &f) {
        uint64_t total = 0;
        for (const FileSegs &s : f) total += s.len;
        return total;
    }
    // no more threads than there is work for: one per 8 files or per 2 MiB, whichever asks for more
    static int size_crew(int want, int n, uint64_t total_bytes) {
        const int useful = (int)std::max<uint64_t>((uint64_t)(n + 7) / 8, total_bytes >> 21);
        return std::max(1, std::min(want, useful));
    }
    static float ms_since(clk::time_point t) { return (float)std::chrono::duration<double, std::milli>(clk::now() - t).count(); }
    void mark() { t0 = clk::now(); }
    float lap() {  // the time since the last mark, which it moves to now
        const float ms = ms_since(t0);
        mark();
        return ms;
    }
};

// The ingest proper, for files in host memory (segments) and in device memory alike.  The two sources differ in how a file's
// head is obtained (host: it is there, or gathered from the segments; device: the files are staged FIRST, the device says how
// long each head is and delivers them packed), how a whole file is obtained (host: gathered from the segments by the crew
// thread that needs it; device: the files that need it are fetched back from their slots together, one synchronisation) and
// how the two bytes at the verdict are read (FileSegs::at).  Everything else is one body: the stages below, in this order.
int DeviceBatch::ingest_files(std::vector<FileSegs> &files, unsigned flags, std::chrono::steady_clock::time_point t_begin) {
    IngestRun r(files, flags, ctx_->host_threads > 0 ? ctx_->host_threads : default_host_threads());
    ingest_.threads = r.crew.threads();
    int rc = JPGPU_OK;
    r.mark();
    if (r.device) {
        // (a device source: step 2 comes first -- the heads are read from the batch's own copy of the files)
        if ((rc = place_files(r)) != JPGPU_OK || (rc = stage_device_gather(r)) != JPGPU_OK || (rc = stage_device_heads(r)) != JPGPU_OK) return rc;
        r.device_stage_ms = r.lap();
        if ((rc = plan_heads(r)) != JPGPU_OK) return rc;
        ingest_.parse_ms = r.lap();
    } else {
        if ((rc = plan_heads(r)) != JPGPU_OK) return rc;
        ingest_.parse_ms = r.lap();
        find_arena_span(r);
        if ((rc = place_files(r)) != JPGPU_OK) return rc;
        rc = r.arena_span.first ? stage_pinned_arena(r) : r.pinned ? stage_pinned_segments(r) : stage_pageable(r);
        if (rc != JPGPU_OK) return rc;
    }
    if ((rc = confirm_plans(r)) != JPGPU_OK) return rc;
    work_in_flight_ = false;  // the upload stream waited for this batch's earlier device work, and has been drained
    ingest_.copy_ms = r.lap() + r.device_stage_ms;
    demote_unclosed_plans(r);
    if ((rc = finish_plans(r)) != JPGPU_OK) return rc;
    ingest_.full_walk_ms = r.lap();
    ingest_.n_linearised = r.n_linearised.load();
    merge_plans(r);
    rc = layout_and_upload(r.file_ptr, r.file_len, true);
    replay_possible_ = rc == JPGPU_OK && !entropy_only_;
    whole_files_ = rc == JPGPU_OK;  // (redo_swallowed: the files are in d_input_ as they came)
    ingest_.layout_ms = IngestRun::ms_since(r.t0);
    ingest_.total_ms = IngestRun::ms_since(t_begin);
    return rc;
}

// ---- 1. header-only plans (a multi-segment file: over its first 64 KiB, gathered; should its first scan start behind
//         them, or the plan not be "headers + one sequential scan", the whole file is gathered for the full walks)
int DeviceBatch::plan_heads(IngestRun &r) {
    std::vector<uint8_t> want_whole((size_t)(r.device ? r.n : 0), 0);
    r.crew.run((size_t)r.n, [&](size_t i, int) {
        FileSegs &f = r.files[i];
        FilePlan &fp = r.plans[i];
        if (f.len > kMaxFileBytes) {
            fp.img.file_len = f.len;
            fp.need_full = true;  // refused by the full path before it reads a byte
            return;
        }
        if (f.n > 1) f.gather(FileSegs::kHeadBytes);
        plan_file_headers(f.base, f.base_len, fp);
        if (!f.whole()) {
            if (fp.speculative) {
                fp.jobs[0].entropy_len = f.len - fp.scan_data_pos;
            } else if (f.device) {
                want_whole[i] = 1;
            } else {
                f.gather(f.len);
                r.n_linearised.fetch_add(1, std::memory_order_relaxed);
                plan_file_headers(f.base, f.base_len, fp);
            }
        }
        fp.img.file_len = f.len;
    });
    std::vector<int> fetch;  // device files whose head did not do: fetched whole, together, and planned again
    for (size_t i = 0; i < want_whole.size(); i++)
        if (want_whole[i]) fetch.push_back((int)i);
    if (fetch.empty()) return JPGPU_OK;
    const int rc = fetch_device_files(r.files, fetch);
    if (rc != JPGPU_OK) return rc;
    r.crew.run(fetch.size(), [&](size_t k, int) {
        FileSegs &f = r.files[(size_t)fetch[k]];
        FilePlan &fp = r.plans[(size_t)fetch[k]];
        plan_file_headers(f.base, f.base_len, fp);
        fp.img.file_len = f.len;
    });
    return JPGPU_OK;
}

// One page-locked arena (JPGPU_UPLOAD_PINNED_ARENA): the device copy keeps the arena's own layout -- file i lies where it
// lies in the arena, relative to the lowest address -- so the whole span travels as a few large DMAs instead of one per
// file (1 MiB copies reach ~36 GB/s on this link, 32 MiB ones 56).  Needs every file contiguous in memory and a span
// that is mostly payload; otherwise the files go one DMA per segment.
void DeviceBatch::find_arena_span(IngestRun &r) const {
    if (!(r.flags & JPGPU_UPLOAD_PINNED_ARENA) || r.n == 0) return;
    const uint8_t *lo = nullptr, *hi = nullptr;
    bool contiguous = true;
    for (int i = 0; i < r.n && contiguous; i++) {
        const FileSegs &f = r.files[(size_t)i];
        if (f.len == 0) continue;
        if (f.len > kMaxFileBytes) contiguous = false;
        const uint8_t *expect = nullptr;
        for (int k = 0; k < f.n; k++) {
            if (!f.seg[k].len) continue;
            if (expect && f.seg[k].data != expect) contiguous = false;
            if (!lo || f.seg[k].data < lo) lo = f.seg[k].data;
            if (!hi || f.seg[k].data + f.seg[k].len > hi) hi = f.seg[k].data + f.seg[k].len;
            expect = f.seg[k].data + f.seg[k].len;
        }
    }
    if (contiguous && lo && (uint64_t)(hi - lo) <= 2 * r.total_bytes + (1u << 20)) r.arena_span = {lo, (size_t)(hi - lo)};
}

// ---- 2. the files -> HBM (every file gets its slot, whatever became of its plan: the layout does not wait for plans)
// Where every file lies in the input buffer (FileSegs::slot), how large that buffer is, and the buffer itself: the files back to back
// in 256-byte slots whatever their source, or where they lie in the arena; 256 bytes of slack in front and behind either way.
int DeviceBatch::place_files(IngestRun &r) {
    uint64_t in_off = 256;
    if (r.arena_span.first) {
        for (FileSegs &f : r.files) {
            const uint8_t *first = nullptr;
            for (int k = 0; k < f.n && !first; k++)
                if (f.seg[k].len) first = f.seg[k].data;
            f.slot = 256 + (first ? (uint64_t)(first - r.arena_span.first) : 0u);
        }
        in_off = align_up(256 + r.arena_span.second, 256);
    } else {
        for (FileSegs &f : r.files) {
            f.slot = in_off;
            if (f.len <= kMaxFileBytes) in_off = align_up(in_off + f.len, 256);
        }
    }
    input_bytes_ = in_off + 256;
    const hipError_t e = d_input_.reserve((size_t)input_bytes_);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(input)");
    return JPGPU_OK;
}

// Step 2 of the ingest: caller memory -> HBM.
//  - pageable input: through the pinned staging ring.  The input buffer is cut into pieces that never cross a 32 MiB slot;
//    the crew copies pieces in buffer order, whoever completes a slot sends it off (one DMA per slot) and records the event
//    that frees the slot for the chunk n_slots later;
//  - page-locked input (JPGPU_UPLOAD_PINNED): one DMA per segment from where the caller's bytes lie; the slack between the
//    files is zeroed by one fill of the whole input buffer in front of the copies (~0.3 ms per GB, on the device).
int DeviceBatch::stage_pinned_arena(IngestRun &r) {
    hipStream_t up = ctx_->upload_stream;
    uint8_t *d_in = (uint8_t *)d_input_.ptr;
    // the slack in front of the span and behind it is read by the kernels' wide loads: defined (zero); what lies between
    // the files inside the span are the arena's own bytes (nothing a result depends on: every read is bounded by a length)
    hipError_t e = hipMemsetAsync(d_in, 0, 256, up);
    const uint64_t tail = 256 + r.arena_span.second;
    if (e == hipSuccess) e = hipMemsetAsync(d_in + tail, 0, (size_t)(input_bytes_ - tail), up);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(input slack)");
    constexpr size_t kChunk = 32u << 20;
    for (size_t off = 0; off < r.arena_span.second; off += kChunk) {
        const size_t m = std::min(kChunk, r.arena_span.second - off);
        e = hipMemcpyAsync(d_in + 256 + off, r.arena_span.first + off, m, hipMemcpyHostToDevice, up);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(pinned arena)");
        ingest_.n_pinned_dma++;
    }
    return JPGPU_OK;
}

int DeviceBatch::stage_pinned_segments(IngestRun &r) {
    hipStream_t up = ctx_->upload_stream;
    uint8_t *d_in = (uint8_t *)d_input_.ptr;
    // segments scattered in page-locked memory: the device pulls them itself (gather_pinned_kernel, 32 KiB pieces) -- one
    // launch instead of one hipMemcpyAsync per segment
    hipError_t e = hipMemsetAsync(d_in, 0, (size_t)input_bytes_, up);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(input)");
    constexpr uint32_t kPiece = 32u << 10;
    std::vector<GatherPiece> gp;
    for (const FileSegs &f : r.files) {
        if (f.len > kMaxFileBytes || f.len == 0) continue;
        uint64_t off = f.slot;
        for (int k = 0; k < f.n; k++) {
            if (!f.seg[k].len) continue;
            for (size_t at = 0; at < f.seg[k].len; at += kPiece)
                gp.push_back({(uint64_t)(uintptr_t)(f.seg[k].data + at), off + at, (uint32_t)std::min<size_t>(kPiece, f.seg[k].len - at), 0u});
            off += f.seg[k].len;
            ingest_.n_pinned_dma++;
        }
    }
    if (!gp.empty()) {
        e = d_gather_.reserve(gp.size() * sizeof(GatherPiece));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(gather list)");
        e = hipMemcpyAsync(d_gather_.ptr, gp.data(), gp.size() * sizeof(GatherPiece), hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipStreamSynchronize(up);  // `gp` is a local (pageable) vector
        if (e == hipSuccess) e = launch_gather_pinned(up, (const GatherPiece *)d_gather_.ptr, (int)gp.size(), d_in);
        if (e != hipSuccess) return hip_fail(e, "gather_pinned_kernel");
    }
    return JPGPU_OK;
}

int DeviceBatch::stage_pageable(IngestRun &r) {
    hipError_t e = hipSuccess;
    hipStream_t up = ctx_->upload_stream;
    uint8_t *d_in = (uint8_t *)d_input_.ptr;
    StagingRing &ring = ctx_->staging;
    const uint64_t kSlot = ring.slot_bytes;
    const size_t n_slots = (size_t)ring.n_slots;
    std::vector<StagePiece> pieces;
    uint64_t pos = 0;
    for (const FileSegs &f : r.files) {
        uint64_t off = f.slot;
        if (f.len > kMaxFileBytes || f.len == 0) continue;
        if (off > pos) cut_stage_pieces(pieces, nullptr, pos, off - pos, kSlot);
        for (int k = 0; k < f.n; k++) {
            if (!f.seg[k].len) continue;
            cut_stage_pieces(pieces, f.seg[k].data, off, f.seg[k].len, kSlot);
            off += f.seg[k].len;
        }
        pos = off;
    }
    if (input_bytes_ > pos) cut_stage_pieces(pieces, nullptr, pos, input_bytes_ - pos, kSlot);

    const size_t n_chunks = (size_t)((input_bytes_ + kSlot - 1) / kSlot);
    std::vector<std::atomic<int>> remaining(n_chunks);
    std::vector<std::atomic<int>> state(n_chunks);  // 0 = being filled, 1 = DMA issued (event recorded), 2 = slot known drained
    for (size_t c = 0; c < n_chunks; c++) {
        remaining[c].store(0, std::memory_order_relaxed);
        state[c].store(0, std::memory_order_relaxed);
    }
    for (const StagePiece &p : pieces) remaining[p.dst / kSlot].fetch_add(1, std::memory_order_relaxed);
    for (size_t c = 0; c < std::min<size_t>(n_chunks, n_slots); c++) {
        if (!ring.slot[c]) {
            e = hipHostMalloc((void **)&ring.slot[c], kSlot, hipHostMallocDefault);
            if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(staging)");
        }
        if (!ring.drained[c]) {
            e = hipEventCreateWithFlags(&ring.drained[c], hipEventDisableTiming | hipEventBlockingSync);
            if (e != hipSuccess) return hip_fail(e, "hipEventCreate(staging)");
        }
    }
    std::atomic<int> hip_error{(int)hipSuccess};
    const int device = ctx_->device;
    const uint64_t total = input_bytes_;
    r.crew.run(pieces.size(), [&](size_t k, int) {
        const StagePiece &p = pieces[k];
        const size_t c = (size_t)(p.dst / kSlot);
        const int slot = (int)(c % n_slots);
        if (hip_error.load(std::memory_order_relaxed) != (int)hipSuccess) return;
        (void)hipSetDevice(device);
        if (c >= n_slots) {
            // the slot still holds chunk c - n_slots until that chunk's DMA has read it
            std::atomic<int> &prev = state[c - n_slots];
            while (prev.load(std::memory_order_acquire) == 0) {
                if (hip_error.load(std::memory_order_relaxed) != (int)hipSuccess) return;
                std::this_thread::yield();
            }
            if (prev.load(std::memory_order_acquire) == 1) {
                const hipError_t es = hipEventSynchronize(ring.drained[slot]);
                if (es != hipSuccess) {
                    hip_error.store((int)es);
                    return;
                }
                prev.store(2, std::memory_order_release);
            }
        }
        uint8_t *dst = ring.slot[slot] + (p.dst - (uint64_t)c * kSlot);
        if (p.src) memcpy(dst, p.src, p.n);
        else memset(dst, 0, p.n);
        if (remaining[c].fetch_sub(1, std::memory_order_acq_rel) == 1) {
            const uint64_t base = (uint64_t)c * kSlot;
            const size_t bytes = (size_t)std::min<uint64_t>(kSlot, total - base);
            hipError_t ec = hipMemcpyAsync(d_in + base, ring.slot[slot], bytes, hipMemcpyHostToDevice, up);
            if (ec == hipSuccess) ec = hipEventRecord(ring.drained[slot], up);
            if (ec != hipSuccess) hip_error.store((int)ec);
            state[c].store(1, std::memory_order_release);
        }
    });
    if (hip_error.load() != (int)hipSuccess) {
        (void)hipStreamSynchronize(up);
        return hip_fail((hipError_t)hip_error.load(), "staged H2D");
    }
    return JPGPU_OK;
}

namespace {
// the context's page-locked buffers for what the device reports per file (the ingest verdicts and the head lengths; the packed heads):
// grown when `n` elements do not fit, never shrunk, never smaller than `at_least`
template <typename T>
hipError_t reserve_pinned(T *&buf, size_t &cap, size_t n, size_t at_least) {
    if (cap >= n) return hipSuccess;
    if (buf) (void)hipHostFree(buf);
    buf = nullptr;
    cap = 0;
    const size_t want = std::max(n, at_least);
    const hipError_t e = hipHostMalloc((void **)&buf, want * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
}
}  // namespace

// Step 2 of the ingest for a device source, and how its heads are obtained: the caller's device memory -> the input buffer
// (gather_device_kernel: the slots of upload_segments' layout, every byte of slack written as zero), then the head the host
// parser needs of every file: head_walk_kernel says how long it is, head_scan_kernel where it goes, head_pack_kernel packs them.
// Two small H2D (the pieces, the files), four launches, one D2H of the lengths, offsets and total and a synchronisation -- from
// there on no kernel reads the caller's memory any more --, then one D2H of the packed heads and a second synchronisation (the host
// has to know the total before it can ask for the bytes), whatever the number of files.
// The first half: the gather, the head lengths, the first synchronisation.
int DeviceBatch::stage_device_gather(IngestRun &r) {
    const std::vector<FileSegs> &files = r.files;
    const size_t n = files.size();
    std::vector<GatherPiece> gp;
    std::vector<DeviceFile> df(n);
    gp.push_back({0u, 0u, 0u, 256u});  // the slack in front of the first file ...
    for (size_t i = 0; i < n; i++) {
        const FileSegs &f = files[i];
        df[i] = {0u, 0u, 0u};
        if (f.len == 0 || f.len > kMaxFileBytes) continue;
        df[i] = {f.slot, (uint32_t)f.len, 0u};
        for (size_t at = 0; at < f.len; at += kGatherPieceBytes) {
            const uint32_t m = (uint32_t)std::min<size_t>(kGatherPieceBytes, f.len - at);
            const uint32_t pad = at + m == f.len ? (uint32_t)(align_up(f.len, 256) - f.len) : 0u;  // (the last piece: up to the slot's end)
            gp.push_back({(uint64_t)(uintptr_t)(f.dev + at), f.slot + at, m, pad});
        }
        device_ingest_.files_gathered++;
        device_ingest_.bytes_gathered += f.len;
    }
    gp.push_back({0u, input_bytes_ - 256, 0u, 256u});  // ... and behind the last
    // one device buffer: the pieces, the files, then what comes back in one copy: head_off[n + 1] (64-bit; [n] = the total), head_len[n]
    const size_t files_at = align_up(gp.size() * sizeof(GatherPiece), 256), off_at = align_up(files_at + n * sizeof(DeviceFile), 256);
    const size_t len_at = off_at + (n + 1) * sizeof(uint64_t), back_words = 2 * (n + 1) + n;
    hipError_t e = d_gather_.reserve(len_at + n * sizeof(uint32_t) + 256);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(gather list)");
    StagingRing &ring = ctx_->staging;
    e = reserve_pinned(ring.verdict, ring.verdict_cap, back_words, 4096);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(verdict)");
    hipStream_t up = ctx_->upload_stream;
    uint8_t *d_in = (uint8_t *)d_input_.ptr, *d_list = (uint8_t *)d_gather_.ptr;
    r.d_files = (const DeviceFile *)(d_list + files_at);
    r.d_head_off = (uint64_t *)(d_list + off_at);
    r.d_head_len = (uint32_t *)(d_list + len_at);
    e = hipMemcpyAsync(d_list, gp.data(), gp.size() * sizeof(GatherPiece), hipMemcpyHostToDevice, up);
    if (e == hipSuccess && n) e = hipMemcpyAsync(d_list + files_at, df.data(), n * sizeof(DeviceFile), hipMemcpyHostToDevice, up);
    for (hipEvent_t &ev : gather_ev_)
        if (e == hipSuccess && !ev) e = hipEventCreate(&ev);
    if (e == hipSuccess) e = hipEventRecord(gather_ev_[0], up);
    if (e == hipSuccess) e = launch_gather_device(up, (const GatherPiece *)d_list, (int)gp.size(), d_in);
    if (e == hipSuccess) e = hipEventRecord(gather_ev_[1], up);
    if (e == hipSuccess) e = launch_head_walk(up, d_in, r.d_files, (int)n, r.d_head_len);
    if (e == hipSuccess) e = launch_head_scan(up, r.d_head_len, (int)n, r.d_head_off);
    if (e == hipSuccess && n) e = hipMemcpyAsync(ring.verdict, r.d_head_off, back_words * sizeof(uint32_t), hipMemcpyDeviceToHost, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);  // (`gp` and `df` are local, pageable vectors; the caller's memory is free from here)
    if (e == hipSuccess) e = hipEventElapsedTime(&device_ingest_.gather_ms, gather_ev_[0], gather_ev_[1]);
    if (e != hipSuccess) return hip_fail(e, "gather of device files");
    if (n == 0) return JPGPU_OK;
    r.head_off.resize(n + 1);
    memcpy(r.head_off.data(), ring.verdict, (n + 1) * sizeof(uint64_t));
    r.head_len.assign(ring.verdict + 2 * (n + 1), ring.verdict + back_words);
    for (size_t i = 0; i < n; i++)
        if (r.head_len[i] & kHeadGaveUp) device_ingest_.walker_giveups++;
    device_ingest_.head_bytes = r.head_off[n];
    return JPGPU_OK;
}

// The second half: the packed heads, the second synchronisation; every file's `base` is its head from here on.
int DeviceBatch::stage_device_heads(IngestRun &r) {
    const size_t n = r.files.size();
    const uint64_t total = n ? r.head_off[n] : 0;
    if (total == 0) return JPGPU_OK;
    StagingRing &ring = ctx_->staging;
    hipStream_t up = ctx_->upload_stream;
    hipError_t e = reserve_pinned(ring.heads, ring.heads_cap, (size_t)total, 4u << 20);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(heads)");
    e = d_heads_.reserve((size_t)total + 256);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(heads)");
    e = launch_head_pack(up, (const uint8_t *)d_input_.ptr, r.d_files, (int)n, r.d_head_len, r.d_head_off, (uint8_t *)d_heads_.ptr);
    if (e == hipSuccess) e = hipMemcpyAsync(ring.heads, d_heads_.ptr, (size_t)total, hipMemcpyDeviceToHost, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);
    if (e != hipSuccess) return hip_fail(e, "heads of device files");
    for (size_t i = 0; i < n; i++) {
        FileSegs &f = r.files[i];
        if (f.len > kMaxFileBytes) continue;
        f.base = ring.heads + r.head_off[i];
        // (a hint: what the host reads of it is bounded by the file here too)
        f.base_len = std::min<size_t>(r.head_len[i] & ~kHeadGaveUp, std::min<size_t>(f.len, kDeviceHeadMax));
    }
    return JPGPU_OK;
}

// ---- 3. the device's verdict on the header-only plans
int DeviceBatch::confirm_plans(IngestRun &r) {
    std::vector<int> spec;
    for (int i = 0; i < r.n; i++)
        if (r.plans[(size_t)i].speculative) spec.push_back(i);
    if (spec.empty()) {
        const hipError_t e = hipStreamSynchronize(ctx_->upload_stream);  // the caller's buffers may be released after upload returns
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(upload)");
        return JPGPU_OK;
    }
    std::vector<uint32_t> first, bytes;
    const int rc = verify_plans(r, spec, first, r.device ? &bytes : nullptr);
    if (rc != JPGPU_OK) return rc;
    for (size_t k = 0; k < spec.size(); k++) {
        FilePlan &fp = r.plans[(size_t)spec[k]];
        FileSegs &f = r.files[(size_t)spec[k]];
        const size_t dlen = f.len - fp.scan_data_pos;
        const uint32_t pos = first[k];
        if (r.device) {
            f.verdict_at = fp.scan_data_pos + pos;
            f.verdict = bytes[k];
        }
        // classify16 only calls FF xx a marker when xx exists: pos + 1 < dlen
        if (pos != 0xFFFFFFFFu && (size_t)pos + 1 < dlen && f.at(fp.scan_data_pos + pos) == 0xFF && f.at(fp.scan_data_pos + pos + 1) == kEOI) {
            fp.seq_ends.assign(1, (size_t)pos);
        } else {
            fp.speculative = false;
            fp.need_full = true;
            fp.jobs.clear();
        }
    }
    return JPGPU_OK;
}

// A file the host does not hold whole -- a multi-segment file planned from its gathered head, a device file planned from the head
// the device delivered -- keeps its header-only plan when the EOI closes the file: the direct verdict (plan_swallowed_terminator)
// needs nothing but offsets then.  Anything else replays the walk over the whole file, i.e. takes the general path.
void DeviceBatch::demote_unclosed_plans(IngestRun &r) const {
    for (int i = 0; i < r.n; i++) {
        FilePlan &fp = r.plans[(size_t)i];
        const FileSegs &f = r.files[(size_t)i];
        if (fp.speculative && !f.whole() && fp.scan_data_pos + fp.seq_ends[0] + 2 != f.len) {
            fp.speculative = false;
            fp.need_full = true;
        }
    }
}

// ---- 4. the rest: "one byte into the terminator" verdicts of the confirmed plans, full walks of everything else
int DeviceBatch::finish_plans(IngestRun &r) {
    if (r.device) {
        // the device files that take the general path and are not on the host yet are fetched together
        std::vector<int> fetch;
        for (int i = 0; i < r.n; i++) {
            const FileSegs &f = r.files[(size_t)i];
            if (r.plans[(size_t)i].need_full && !f.whole() && f.len <= kMaxFileBytes) fetch.push_back(i);
        }
        const int rc = fetch_device_files(r.files, fetch);
        if (rc != JPGPU_OK) return rc;
    }
    r.crew.run((size_t)r.n, [&](size_t i, int) {
        FilePlan &fp = r.plans[i];
        FileSegs &f = r.files[i];
        if (fp.speculative) {
            plan_swallowed_terminator(fp, f.base, f.len, true);
        } else if (fp.need_full) {
            if (!f.whole() && f.len <= kMaxFileBytes) {
                f.gather(f.len);
                r.n_linearised.fetch_add(1, std::memory_order_relaxed);
            }
            plan_file_full(f.base, f.len, (int)i, fp);
        }
    });
    return JPGPU_OK;
}

// ---- 5. merge into the batch's job list (file order)
void DeviceBatch::merge_plans(IngestRun &r) {
    r.file_ptr.resize((size_t)r.n);
    r.file_len.resize((size_t)r.n);
    for (int i = 0; i < r.n; i++) {
        FilePlan &fp = r.plans[(size_t)i];
        const FileSegs &f = r.files[(size_t)i];
        r.file_ptr[(size_t)i] = f.base;
        r.file_len[(size_t)i] = f.len;
        const size_t first_job = jobs_.size();
        if (fp.speculative) ingest_.n_header_only++;
        else if (fp.need_full) ingest_.n_full_walk++;
        images_[i] = std::move(fp.img);
        ImagePlan &img = images_[i];
        img.file_len = f.len;
        img.file_offset = f.slot;
        img.jobs.clear();
        apply_window((size_t)i, fp.jobs);
        if (img.status != JPGPU_OK) continue;
        for (size_t j = 0; j < fp.jobs.size(); j++) {
            img.jobs.push_back((int)(first_job + j));
            job_image_.push_back(i);
            job_entropy_off_.push_back(fp.jobs[j].entropy ? (uint64_t)(fp.jobs[j].entropy - f.base) : 0u);
            jobs_.push_back(std::move(fp.jobs[j]));
        }
        if (img.swallow_job >= 0) img.swallow_job += (int)first_job;
    }
    r.plans.clear();
}

// Step 3 of the ingest: first marker that is not RSTn behind every planned SOS header (first_marker_kernel); synchronises
// the upload stream, so the caller's buffers are free once this returns.
// bytes (a device source): the two bytes at each reported position too, low byte first (verdict_bytes_kernel behind the verdict;
// the same D2H carries them).
int DeviceBatch::verify_plans(const IngestRun &r, const std::vector<int> &spec, std::vector<uint32_t> &first, std::vector<uint32_t> *bytes) {
    const size_t n = spec.size();
    std::vector<uint32_t> host(3 * n);  // {offset lo, length} pairs, then offset hi
    uint32_t max_len = 0;
    for (size_t k = 0; k < n; k++) {
        const FilePlan &fp = r.plans[(size_t)spec[k]];
        const uint64_t off = r.files[(size_t)spec[k]].slot + fp.scan_data_pos;
        const uint32_t dlen = (uint32_t)(fp.img.file_len - fp.scan_data_pos);
        host[2 * k] = (uint32_t)off;
        host[2 * k + 1] = dlen;
        host[2 * n + k] = (uint32_t)(off >> 32);
        max_len = std::max(max_len, dlen);
    }
    const size_t n_out = bytes ? 2 * n : n;
    hipError_t e = d_verify_.reserve((3 * n + n_out) * sizeof(uint32_t) + 256);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(verify)");
    StagingRing &ring = ctx_->staging;
    e = reserve_pinned(ring.verdict, ring.verdict_cap, n_out, 4096);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(verdict)");
    hipStream_t up = ctx_->upload_stream;
    uint32_t *d = (uint32_t *)d_verify_.ptr;
    e = hipMemcpyAsync(d, host.data(), 3 * n * sizeof(uint32_t), hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipMemsetAsync(d + 3 * n, 0xFF, n * sizeof(uint32_t), up);
    if (e == hipSuccess) e = launch_first_marker(up, (const uint8_t *)d_input_.ptr, d, d + 2 * n, (int)n, max_len, d + 3 * n);
    if (e == hipSuccess && bytes) e = launch_verdict_bytes(up, (const uint8_t *)d_input_.ptr, d, d + 2 * n, d + 3 * n, (int)n, d + 4 * n);
    if (e == hipSuccess) e = hipMemcpyAsync(ring.verdict, d + 3 * n, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);
    if (e != hipSuccess) return hip_fail(e, "ingest verification");
    first.assign(ring.verdict, ring.verdict + n);
    if (bytes) bytes->assign(ring.verdict + n, ring.verdict + 2 * n);
    return JPGPU_OK;
}

// How a whole device file is obtained: from its slot in the input buffer, one D2H per listed file, issued together, one
// synchronisation.  The ingest calls it at most twice: behind the header-only plans (heads that did not do) and in front of step 4
// (plans the device did not confirm, or whose EOI does not close the file).
int DeviceBatch::fetch_device_files(std::vector<FileSegs> &files, const std::vector<int> &which) {
    if (which.empty()) return JPGPU_OK;
    hipStream_t up = ctx_->upload_stream;
    for (int i : which) {
        FileSegs &f = files[(size_t)i];
        f.gathered.resize(f.len);
        const hipError_t e = hipMemcpyAsync(f.gathered.data(), (const uint8_t *)d_input_.ptr + f.slot, f.len, hipMemcpyDeviceToHost, up);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(up);
            return hip_fail(e, "hipMemcpyAsync(device file to the host)");
        }
        device_ingest_.files_downloaded++;
        device_ingest_.bytes_downloaded += f.len;
    }
    const hipError_t e = hipStreamSynchronize(up);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(device files to the host)");
    for (int i : which) {
        FileSegs &f = files[(size_t)i];
        f.base = f.gathered.data();
        f.base_len = f.len;
    }
    return JPGPU_OK;
}

}  // namespace jpgpu
