// jpeglibrary_amd/csrc/device_batch_layout.cpp -- DeviceBatch::layout_and_upload, a list of stages: the HBM layout of an upload (device_batch.cpp
// has the layout's description), the scan descriptors, the table pools and every kernel's work list; the device copies.  The stages hand one another
// an UploadPlan; read_layout_switches alone reads the JPGPU_* switches.  (One file with device_batch.cpp until round 6; the launches are in
// device_batch_launch.cpp, results and the partial-flush replay in device_batch_result.cpp.)
#include "device_batch.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "k3_quant_order.h"
#include "kernels.h"

namespace jpgpu {

static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

namespace {
// Workgroup i of a launch runs on XCD i % 8 (round-robin dispatch), each XCD behind its own L2.  Work lists are built in
// memory order; interleaving them gives every XCD one contiguous run, so that neighbouring work items -- which share the
// cache lines at their common boundary -- meet in one L2 instead of writing two halves of a line from two.
template <typename T>
void xcd_interleave(std::vector<T> &w, int xcds) {
    if (xcds <= 1 || w.size() < (size_t)xcds * 8) return;
    const size_t n = w.size(), per = (n + xcds - 1) / xcds;
    std::vector<T> m;
    m.reserve(n);
    for (size_t i = 0; m.size() < n; i++) {
        const size_t src = (i % xcds) * per + i / xcds;
        if (src < n) m.push_back(w[src]);
    }
    w.swap(m);
}

// Every JPGPU_* switch of the layout.  Read once per upload (not per scan job; not once per process: tests set them between calls),
// but for the three marked "process", which are read once per process.
struct LayoutSwitches {
    int dbg_delay_scan = -1, dbg_delay_ms = 0;  // JPGPU_DEBUG_DELAY_SCAN="k:ms" (test hook, see plan_progressive_scan)
    bool dbg_status = false, prog_no_pipeline = false, no_subseq = false;  // JPGPU_DEBUG_STATUS, JPGPU_PROG_NO_PIPELINE, JPGPU_NO_SUBSEQ
    uint32_t subseq_shift = 0;                  // JPGPU_SUBSEQ_SHIFT, 8..14; 0 = unset
    // subsequences in the batch from which a lane of the K2S final pass takes two (test hook: 1 = always, so a small batch reaches
    // the form the planner otherwise keeps for kSubFinalFewSubs and more)
    uint64_t subseq_two_per_lane_from = kSubFinalFewSubs;  // JPGPU_SUBSEQ_TWO_PER_LANE_FROM
    // a scan with fewer restart intervals than this gets one WAVE per interval (progressive_stream_kernel)
    uint32_t stream_max_intervals = 16;         // JPGPU_PROG_STREAM_MAX_INTERVALS
    // polls (~2-3 us each) a follower scan of the pipelined launch may spend before it gives up: ~0.3 s by default (a fully
    // resident grid -- the only kind that takes the pipelined launch by default -- makes progress within microseconds)
    uint32_t prog_spin_budget = 1u << 17;       // JPGPU_PROG_SPIN_BUDGET
    bool subseq_host_check = false;             // JPGPU_SUBSEQ_HOST_CHECK (A/B switch: the host reads the counts between rounds)
    // JPGPU_DENSE_HANDOFF: 1 = every scan dense, 0 = split wherever K3 has the form, unset = ... and the content promises a gain
    bool handoff_set = false, handoff_dense = false;
    bool tile_align = true;                     // JPGPU_TILE_ALIGN=0 turns it off (A/B switch, default on)
    bool overlap = false;                       // JPGPU_OVERLAP: the opt-in two-stream issue order (plan_overlap_halves)
    bool time_upsample = false;                 // JPGPU_TIME_UPSAMPLE: an event pair around the K3U call (jpgpu_batch_upsampling_ms; measuring aid)
    int xcds = 8;                               // JPGPU_XCD_MAP.  MI355X: 8 XCDs; 0 / 1 = memory order (A/B switch)
    // process: JPGPU_PROG_BY_SCAN, JPGPU_PROG_NO_WAVE_CHAINS, JPGPU_K1_THREE_PASS (A/B switch: count + prefix + write kernels)
    bool prog_by_scan = false, no_wave_chains = false, k1_three_pass = false;
};

LayoutSwitches read_layout_switches() {
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    static const bool by_scan = set("JPGPU_PROG_BY_SCAN"), no_wave_chains = set("JPGPU_PROG_NO_WAVE_CHAINS"), three_pass = set("JPGPU_K1_THREE_PASS");
    LayoutSwitches sw;
    const char *dd = getenv("JPGPU_DEBUG_DELAY_SCAN");
    if (dd && sscanf(dd, "%d:%d", &sw.dbg_delay_scan, &sw.dbg_delay_ms) != 2) sw.dbg_delay_scan = -1;
    sw.dbg_status = set("JPGPU_DEBUG_STATUS");
    if (const char *ev = getenv("JPGPU_SUBSEQ_SHIFT")) sw.subseq_shift = (uint32_t)std::min(14, std::max(8, atoi(ev)));
    if (const char *ev = getenv("JPGPU_SUBSEQ_TWO_PER_LANE_FROM")) sw.subseq_two_per_lane_from = strtoull(ev, nullptr, 10);
    if (const char *ev = getenv("JPGPU_PROG_STREAM_MAX_INTERVALS")) sw.stream_max_intervals = (uint32_t)atoi(ev);
    sw.prog_no_pipeline = set("JPGPU_PROG_NO_PIPELINE");
    if (const char *ev = getenv("JPGPU_PROG_SPIN_BUDGET")) sw.prog_spin_budget = (uint32_t)strtoul(ev, nullptr, 10);
    sw.subseq_host_check = set("JPGPU_SUBSEQ_HOST_CHECK");
    if (const char *ev = getenv("JPGPU_DENSE_HANDOFF")) sw.handoff_set = true, sw.handoff_dense = atoi(ev) != 0;
    if (const char *ev = getenv("JPGPU_TILE_ALIGN")) sw.tile_align = atoi(ev) != 0;
    sw.no_subseq = set("JPGPU_NO_SUBSEQ");
    if (const char *ev = getenv("JPGPU_OVERLAP")) sw.overlap = atoi(ev) != 0;
    if (const char *ev = getenv("JPGPU_XCD_MAP")) sw.xcds = atoi(ev);
    if (const char *ev = getenv("JPGPU_TIME_UPSAMPLE")) sw.time_upsample = atoi(ev) != 0;
    sw.prog_by_scan = by_scan, sw.no_wave_chains = no_wave_chains, sw.k1_three_pass = three_pass;
    return sw;
}

// bit mask of the frame components a scan writes
uint32_t component_mask(const ScanJob &job) {
    uint32_t mask = 0;
    for (int c = 0; c < job.scan_components; c++) mask |= 1u << (job.comp[c].component_index & 31);
    return mask;
}
// chain of a progressive scan: DC scans (interleaved, or Ss = 0) touch coefficient 0 only, an AC scan the band of ONE
// component (what it may write beyond its header stays inside that component's AC coefficients)
int progressive_chain(const ScanJob &job) { return (job.scan_components != 1 || job.ss == 0) ? 0 : 1 + std::min(3, job.comp[0].component_index); }
// two scans stage the same tables in the same slots
bool same_tables(const DevScan &a, const DevScan &b) {
    return memcmp(a.huff_pool, b.huff_pool, sizeof a.huff_pool) == 0 && a.scan_components == b.scan_components &&
           a.blocks_per_mcu == b.blocks_per_mcu && memcmp(a.blk_comp, b.blk_comp, sizeof a.blk_comp) == 0 &&
           memcmp(a.comp, b.comp, sizeof a.comp) == 0;
}
// [i, the return value): the run of consecutive entries from i on whose scans (scan_of(entry index)) stage the same tables
template <typename ScanOf>
size_t same_tables_run(const std::vector<DevScan> &scans, size_t i, size_t n, ScanOf scan_of) {
    size_t k = i + 1;
    while (k < n && same_tables(scans[scan_of(i)], scans[scan_of(k)])) k++;
    return k;
}
}  // namespace

// What the stages of layout_and_upload hand one another: the switches, the batch-wide shapes, the running offsets and every kernel's
// work list while it grows.  (What the launches and the results read afterwards is a member of DeviceBatch.)
struct DeviceBatch::UploadPlan {
    LayoutSwitches sw;
    bool files_resident = false;  // the files are in d_input_ already: no input layout, no copy of them (upload_plan)
    uint32_t subseq_shift = 10, idct_tiles_per_wg = (uint32_t)kIdctTilesPerWg, huff_intervals_per_wg = 0;  // choose_batch_shapes
    uint64_t out_off = 0, coef_off = 0, planes_off = 0, real_blocks = 0, flag_words = 0;
    uint32_t ends_off = 0, total_chunks = 0;
    std::vector<const HuffTable *> huff_keys;  // the table (one of jobs_) that every entry of huff_pool_ was built from
    std::vector<HuffWork> huff_work, sub_work, sub_final_work, prog_work;
    std::vector<ChunkWork> chunk_work, k1_order;  // k1_order: the one-pass marker index: (scan, first chunk) per group of kMarkerGroupChunks chunks, by (group, scan)
    std::vector<std::vector<HuffWork>> prog_work_by_ordinal, prog_streams_by_ordinal;
    std::vector<std::vector<HuffWork>> prog_chain_work[jpgpu_ctx::kProgChains];  // [chain][ordinal in the frame's chain]
    std::vector<IdctWork> idct_work, idct_work_halves;
    std::vector<IdctWork> idct_work_by_class[kNumIdctLayoutClasses];
    std::vector<IdctWork> idct_split_by_class[kNumIdctLayoutClasses];  // scans handed over as half-line planes: the split form of K3
    std::vector<IdctWork> idct_win_by_class[kNumIdctLayoutClasses];    // scans of windowed images: the window form of K3 (MCUs of the cover)
    std::vector<std::vector<IdctWork>> idct_later_levels;  // scans ordered behind earlier scans of their image: one launch per level
    std::vector<std::vector<IdctWork>> idct_later_win_levels;  // ... those of windowed images, a launch of their own per level
    std::vector<IdctWork> idct_partial;                     // "the MCU the scan failed in", bytewise (the caller's canvas)
    std::vector<int> scan_level;
    std::vector<uint32_t> sr_set_scan;  // a scan that stages each distinct set of tables among the DRI = 0 scans
};

int DeviceBatch::layout_and_upload(const std::vector<const uint8_t *> &file_ptr, const std::vector<size_t> &file_len, bool files_resident) {
    UploadPlan p;
    p.files_resident = files_resident;
    p.sw = read_layout_switches();
    p.scan_level.assign(jobs_.size(), 0);
    reset_upload_state(p);
    hipError_t e = hipSetDevice(ctx_->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    if (const int rc = order_upload_behind_work(); rc != JPGPU_OK) return rc;
    // ---- input layout (jpgpu_batch_upload has laid the files out and sent them already: files_resident)
    if (!files_resident) {
        uint64_t in_off = 256;
        for (size_t i = 0; i < images_.size(); i++) {
            images_[i].file_offset = in_off;
            if (images_[i].status == JPGPU_OK && !images_[i].jobs.empty()) in_off = align_up(in_off + file_len[i], 256);
        }
        input_bytes_ = in_off + 256;
    }
    // ---- per-image output / coefficient layout, scan descriptors, pools, work lists
    choose_batch_shapes(p);
    for (size_t ii = 0; ii < images_.size(); ii++) plan_image(p, ii, file_len);
    resolve_offsets(p);
    pool_huffman_runs(p);
    plan_subseq_lists(p);
    assemble_progressive_lists(p);
    plan_output_clears();
    plan_color_convert();
    plan_orient_convert();
    plan_fancy_convert();
    plan_luma_convert();
    assemble_idct_lists(p);
    plan_overlap_halves(p);
    init_status();
    // ---- allocate + H2D
    return upload_plan(p, file_ptr, file_len);
}

void DeviceBatch::reset_upload_state(const UploadPlan &p) {
    dispose_done_ = false;
    if (!in_replay_) {
        // every upload path starts from the batch's own launch modes (the replay's flags used to be reset by
        // upload_segments alone); upload_segments says afterwards whether a partial flush can become necessary
        replay_done_ = replay_possible_ = prog_by_scan_ = replay_layout_active_ = false;
        replay_saved_jobs_.clear();
        for (ImagePlan &img : images_) img.replay_skip = false;
        // jpgpu_batch_subseq_rounds is the last decode's, 0 = not used: an upload without DRI = 0 scans used to report the rounds of the
        // last upload that had some.  (The replay keeps the first pass's count: its own decode has the failed progressive frames alone.)
        last_subseq_rounds_ = 0;
    }
    status_valid_ = keep_progressive_store_ = defer_refusal_ = false;
    resize_plan_valid_ = false;  // (the images' sizes and places are this upload's)
    resized_fmt_ = -1;
    ev_used_ = 0;
    huff_pool_.clear();
    quant_pool_.clear();
    h_scans_.assign(jobs_.size(), DevScan());
    prog_chains_ok_ = true;
    prog_scans_ = prog_max_deps_ = prog_wave_tails_ = prog_launch_form_ = prog_fallbacks_ = 0;
    for (int &n : prog_chain_scans_) n = 0;
    prog_clear_.clear();
    prog_pipelined_ = !p.sw.prog_no_pipeline;
    prog_spin_budget_ = p.sw.prog_spin_budget;
    rgb_convert_.clear();
    color_convert_.clear();
    orient_convert_.clear();
    fancy_convert_.clear();
    luma_convert_.clear();
    luma_work_.clear();
    islow_work_.clear();
    reduced_work_.clear();
    n_luma_fast_ = 0;
    luma_work_windowed_ = false;
    fancy_timed_ = false;
    fancy_time_wanted_ = p.sw.time_upsample;
    sub_scan_ids_.clear();
    total_subs_ = max_subs_per_scan_ = 0;
    sub_shift_used_ = 0;
    k2s_budget_ = 0;
    sub_same_valid_ = k2s_unchecked_ = k2s_idct_behind_ = false;
    // (A/B switch: the host reads the counts between rounds.  Always so over a CALLER'S CANVAS: the device-driven rounds let the
    // output stage run before anybody knows whether they sufficed, and what that stage writes from unconverged states a second,
    // correct pass does not take back where it leaves the canvas alone -- tests/golden/stress/baseline_failing_422_canvas_54.jpg)
    k2s_host_checked_ = p.sw.subseq_host_check || keep_canvas_;
    dispose_jobs_.clear();
    split_scans_.clear();
    dispose_max_blocks_ = split_max_blocks_ = 0;
    dense_valid_ = dense_override_ = false;
    compressed_bytes_ = total_pixels_ = 0;
    for (uint32_t &b : k2_ticket_base_) b = 0;
    decodes_since_query_ = 0;
}

void DeviceBatch::choose_batch_shapes(UploadPlan &p) {
    // DRI = 0 scans are cut into subsequences of 1024 bits; when that gives more lanes than the machine can use anyway the
    // subsequences grow (2048, 4096 bits): a longer one re-synchronises inside itself more often, so fewer rounds
    uint64_t dri0_bits = 0;
    for (size_t j = 0; j < jobs_.size(); j++)
        if (jobs_[j].kind == kScanSequential && jobs_[j].geo.restart_interval == 0) dri0_bits += (uint64_t)jobs_[j].entropy_len * 8;
    while (p.subseq_shift < 12 && (dri0_bits >> p.subseq_shift) >= 500000u) p.subseq_shift++;
    // ... and shrink when the batch is ONE small image (round 6: the reference's callers decode one image per call): a round and the
    // final pass last as long as one lane's subsequence, and 1024-bit lanes of a 48 KB scan fill six waves of a 256-CU machine.
    // (512 bits, not 256: the 6-block MCU phase of a 4:2:0 stream re-synchronises over a few hundred bits, and every subsequence
    // it spans is another round -- a 640 x 368 image took 27 rounds of 256-bit lanes, 9 of 512-bit ones)
    while (p.subseq_shift > 9 && (dri0_bits >> p.subseq_shift) < 4096u) p.subseq_shift--;
    if (p.sw.subseq_shift) p.subseq_shift = p.sw.subseq_shift;
    // K3 walks runs of consecutive tiles per workgroup (the next tile's coefficients fetched under the current one's transform).
    // A batch of few tiles -- one image per call -- is cut into shorter runs: every CU gets work at once (round 6).
    uint64_t blocks = 0;
    for (const ScanJob &job : jobs_)
        if (job.kind != kScanProgressive) blocks += (uint64_t)job.geo.mcus_per_line * job.geo.mcus_per_column * (uint64_t)std::max(1, job.blocks_per_mcu);
    const uint64_t tiles = blocks / (uint64_t)kIdctBlocksPerWg + 1, want_wgs = 3ull * (uint64_t)(ctx_->num_cus > 0 ? ctx_->num_cus : 256);
    while (p.idct_tiles_per_wg > 1 && tiles / p.idct_tiles_per_wg < want_wgs) p.idct_tiles_per_wg /= 2;
    // (known before any work list is cut: the Huffman workgroup's size -- intervals per work entry -- follows from it)
    n_huff_slots_ = 1;
    for (const ScanJob &job : jobs_) n_huff_slots_ = std::max(n_huff_slots_, job.n_huff);
    // LDS the K2 family stages its tables in: the largest set among the sequential scans (an AC table 9 040 bytes, a DC table
    // 2 896: kernels.h); the waves per workgroup are what it leaves room for
    k2_tab_bytes_ = kK2AcTabBytes + kK2DcTabBytes;
    for (const ScanJob &job : jobs_) {
        if (job.kind != kScanSequential) continue;
        uint32_t bytes = 0;
        for (int k = 0; k < job.n_huff; k++) {
            bool is_dc = false;
            for (int c = 0; c < job.scan_components; c++) is_dc |= job.dc_slot[c] == k;
            bytes += is_dc ? kK2DcTabBytes : kK2AcTabBytes;
        }
        k2_tab_bytes_ = std::max(k2_tab_bytes_, bytes);
    }
    p.huff_intervals_per_wg = 64u * (uint32_t)huffman_waves(k2_tab_bytes_);
}

// The table pools.  The order of the calls defines the pool indices: a scan's own tables in slot order, a Dispose job's behind them.
uint16_t DeviceBatch::huff_index(UploadPlan &p, const HuffTable &t) {
    // the device image of a table depends on BITS / HUFFVAL alone: look those up before building it (a batch of
    // camera files carries the same four tables a thousand times)
    for (size_t i = 0; i < p.huff_keys.size(); i++)
        if (p.huff_keys[i]->num_values == t.num_values && memcmp(p.huff_keys[i]->bits, t.bits, 16) == 0 &&
            memcmp(p.huff_keys[i]->values, t.values, t.num_values) == 0)
            return (uint16_t)i;
    DevHuffTable d;
    t.to_device(&d);
    p.huff_keys.push_back(&t);
    huff_pool_.push_back(d);
    return (uint16_t)(huff_pool_.size() - 1);
}
uint16_t DeviceBatch::quant_index(const QuantTable &t) {
    DevQuantTable d;
    memcpy(d.q, t.elements, sizeof d.q);
    k3_quant_pair_floats(d.q, d.qf);
    for (size_t i = 0; i < quant_pool_.size(); i++)
        if (memcmp(&quant_pool_[i], &d, sizeof d) == 0) return (uint16_t)i;
    quant_pool_.push_back(d);
    return (uint16_t)(quant_pool_.size() - 1);
}

// One image: its place in every buffer, then its scan jobs.  The `continue`s decide what a scan has contributed: a progressive scan --
// planned or not -- has its descriptor, interval ends and K1 work and takes no store; a replay-skipped image keeps its place and gets no work.
void DeviceBatch::plan_image(UploadPlan &p, size_t ii, const std::vector<size_t> &file_len) {
    ImagePlan &img = images_[ii];
    img.out_offset = p.out_off;
    img.planes_offset = p.planes_off;
    img.coef_offset = p.coef_off;
    img.total_blocks = 0;
    if (img.status != JPGPU_OK) return;
    p.out_off = align_up(p.out_off + slot_bytes(img), 256);  // (the scratch image mirrors these offsets: the slot holds the larger of the two)
    p.planes_off = align_up(p.planes_off + img.planes_bytes, 256);
    if (!img.jobs.empty()) total_pixels_ += (uint64_t)img.width * img.height;
    // sequential scans of this image that write a component an earlier scan of it has written (ordered launches, see plan_idct_work)
    bool overlapping_scans = false;
    uint32_t seen = 0;
    for (int j : img.jobs) {
        const ScanJob &job = jobs_[j];
        if (job.kind != kScanSequential || job.disabled) continue;
        overlapping_scans |= (component_mask(job) & seen) != 0;
        seen |= component_mask(job);
    }
    for (int j : img.jobs) {
        const ScanJob &job = jobs_[j];
        fill_scan(p, ii, j, file_len[ii]);
        if (job.kind == kScanFrameOnly && job.dispose_generic) plan_dispose_job(j, !img.replay_skip);
        if (job.kind == kScanProgressive) {
            // (disabled -- replay of a failed file: the reference never got to this scan; K1 still indexes it)
            if (!job.disabled && !img.replay_skip) plan_progressive_scan(p, img, j);
            continue;  // no store of its own, no IDCT work
        }
        plan_entropy_work(p, ii, j);
        if (img.replay_skip) continue;  // (its samples are in the output buffer already)
        if (h_scans_[j].blocks_per_mcu == 0) continue;  // cannot happen for a resolved scan (sampling factors are checked); no blocks, no work
        plan_idct_work(p, ii, j, overlapping_scans);
    }
}

// The DevScan of scan job j from its ScanJob; its interval ends and its chunks (K1's work) take their places.
void DeviceBatch::fill_scan(UploadPlan &p, size_t ii, int j, size_t file_len) {
    const ImagePlan &img = images_[ii];
    const ScanJob &job = jobs_[j];
    DevScan &s = h_scans_[j];
    memset(&s, 0, sizeof s);
    const BaselineGeometry &g = job.geo;
    s.kind = (uint8_t)job.kind;
    s.last_interval = job.last_interval;
    s.data_off = img.file_offset + job_entropy_off_[j];
    s.data_len = (uint32_t)(file_len - job_entropy_off_[j]);
    if (job.kind == kScanFrameOnly) s.data_len = 0;
    if (job.kind == kScanProgressive) {
        // the segment ends at the next marker that is not RSTn; K1 only has to see that marker
        const size_t end = find_scan_end(job.entropy, job.entropy_len);
        s.data_len = (uint32_t)std::min<size_t>(end + 2, job.entropy_len);
    }
    // progressive entropy scans accumulate into their frame's store (the frame job precedes them)
    s.coef_off = job.kind == kScanProgressive ? h_scans_[img.jobs[0]].coef_off : p.coef_off;
    s.out_off = format_ == JPGPU_FMT_EXTENDED_U16 ? img.planes_offset : img.out_offset;
    s.dri = job.kind == kScanProgressive ? job.scan_dri : g.restart_interval;
    s.mcus_per_line = (uint32_t)g.mcus_per_line;
    s.mcus_per_column = (uint32_t)g.mcus_per_column;
    s.total_mcus = job.kind == kScanProgressive ? job.total_units : s.mcus_per_line * s.mcus_per_column;
    s.n_intervals = s.dri ? (s.total_mcus + s.dri - 1) / s.dri : 1;
    if (s.total_mcus == 0 || job.kind == kScanFrameOnly) s.n_intervals = 0;
    s.ss = job.ss;
    s.se = job.se;
    s.ah = job.ah;
    s.al = job.al;
    s.frame_bpm = job.frame_bpm;
    s.units_per_line = job.units_per_line;
    for (int c = 0; c < kMaxScanComponents; c++) {
        s.fblk_base[c] = job.fblk_base[c];
        s.hblocks[c] = job.hblocks[c];
        s.vblocks[c] = job.vblocks[c];
    }
    s.ends_off = p.ends_off;
    p.ends_off += s.n_intervals;
    s.chunk_off = p.total_chunks;
    s.n_chunks = (uint32_t)(((uint64_t)s.data_len + (s.data_off & 15u) + kMarkerChunkBytes - 1) / kMarkerChunkBytes);
    if (s.n_chunks == 0) s.n_chunks = 1;
    if (job.kind == kScanFrameOnly) s.n_chunks = 0;  // no entropy data: K1 / K2 skip the job
    // (replay_skip: an image the replay of failed progressive frames leaves alone keeps its place in every buffer and gets no work)
    for (uint32_t c = 0; c < s.n_chunks && !img.replay_skip; c += kMarkerChunksPerWg) p.chunk_work.push_back({(uint32_t)j, c});
    for (uint32_t c = 0; c < s.n_chunks && !img.replay_skip; c += kMarkerGroupChunks) p.k1_order.push_back({(uint32_t)j, c});
    p.total_chunks += s.n_chunks;
    s.image_index = (uint32_t)ii;
    s.first_scan = (uint32_t)img.jobs.front();
    s.level_shift = (uint32_t)g.level_shift;
    s.width = g.frame.samples_per_line;
    s.height = g.frame.lines;
    s.precision = g.frame.precision;
    s.frame_components = g.frame.num_components;
    s.scan_components = (uint8_t)job.scan_components;
    s.max_h = (uint8_t)g.max_h;
    s.max_v = (uint8_t)g.max_v;
    s.blocks_per_mcu = (uint8_t)job.blocks_per_mcu;
    s.restart_check_at_end = (s.dri != 0 && s.total_mcus % s.dri == 0) ? 1 : 0;
    for (int k = 0; k < kMaxHuffSlots; k++) s.huff_pool[k] = 0xFFFF;
    for (int k = 0; k < job.n_huff; k++) s.huff_pool[k] = huff_index(p, job.huff_copy[k]);
    for (int c = 0; c < job.scan_components; c++) {
        DevScanComponent &dc = s.comp[c];
        dc.component_index = (uint8_t)job.comp[c].component_index;
        dc.h = job.comp[c].h;
        dc.v = job.comp[c].v;
        dc.hs = (uint8_t)job.comp[c].hs;
        dc.vs = (uint8_t)job.comp[c].vs;
        dc.quant_slot = (uint8_t)c;
        dc.dc_slot = job.dc_slot[c];
        dc.ac_slot = job.ac_slot[c];
        s.quant_pool[c] = quant_index(job.quant_copy[c]);
        const int fc = job.comp[c].component_index;
        if (fc < 4) {
            s.plane_off[c] = img.plane[fc].offset;
            s.plane_pitch[c] = img.plane[fc].pitch;
        }
    }
    // the window and the MCUs K3 walks for it (a whole frame: everything; only the window forms of K3 read these).  MCU (mx, my) of a scan
    // that walks the frame's MCUs holds the pixels [mx * 8 max_h, +8 max_h) x [my * 8 max_v, +8 max_v) and no others: an interleaved
    // sequential scan (a block lies at (mx * max_h + bx) * 8 and is hs * 8 wide, bx + hs <= max_h), a one-component frame, and the frame
    // pass of a progressive frame whose sampling factors all divide the maxima (JpegBlockAllocator.Flush places block bx of the MCU at
    // (mx * h + bx) * hs * 8).  The cover is then the MCUs the window touches; any other scan keeps the whole grid, clipped all the same.
    // (a filtered image, JPGPU_UPSAMPLE_FANCY: K3 decodes its fetch rectangle, the window widened to every tap of K3U -- the whole frame without one)
    const jpgpu_rect win = img.fancy ? fancy_fetch_rect(img) : img.win;
    s.win_x = (uint16_t)win.x;
    s.win_y = (uint16_t)win.y;
    // (an image decoded at a reduced size, include/jpgpu.h "Scaled decode": its window -- the whole reduced picture without one -- and its
    // cover are in pixels and MCUs of that picture, whose MCU is max_h * 8 / scale x max_v * 8 / scale pixels; only K3R reads them)
    const bool reduced = img.scale > 1;
    s.win_w = img.windowed || reduced ? (uint16_t)win.width : s.width;
    s.win_h = img.windowed || reduced ? (uint16_t)win.height : s.height;
    s.cov_cols = (uint16_t)s.mcus_per_line;
    s.cov_rows = (uint16_t)s.mcus_per_column;
    bool mcu_boxes = job.kind != kScanProgressive && g.max_h > 0 && g.max_v > 0 && (job.scan_components > 1 || g.frame.num_components == 1);
    if (job.kind == kScanFrameOnly)
        for (int c = 0; c < job.scan_components; c++) mcu_boxes &= job.comp[c].h * job.comp[c].hs == g.max_h && job.comp[c].v * job.comp[c].vs == g.max_v;
    if (img.windowed && mcu_boxes && win.width != 0 && win.height != 0) {
        const uint32_t mw = 8u / img.scale * (uint32_t)g.max_h, mh = 8u / img.scale * (uint32_t)g.max_v;
        const uint32_t c0 = win.x / mw, c1 = (win.x + win.width + mw - 1) / mw, r0 = win.y / mh, r1 = (win.y + win.height + mh - 1) / mh;
        if (c1 <= s.mcus_per_line && r1 <= s.mcus_per_column) {
            s.cov_x = (uint16_t)c0;
            s.cov_y = (uint16_t)r0;
            s.cov_cols = (uint16_t)(c1 - c0);
            s.cov_rows = (uint16_t)(r1 - r0);
        }
    }
    s.shadow_mask = keep_canvas_ ? kKeepUnreachedMcus : 0;
    for (int c = 0; c < job.scan_components; c++)
        for (int d = c + 1; d < job.scan_components; d++)
            if (job.comp[c].component_index == job.comp[d].component_index) s.shadow_mask |= (uint8_t)(1u << c);
    memcpy(s.blk_comp, job.blk_comp, sizeof s.blk_comp);
    memcpy(s.blk_x, job.blk_x, sizeof s.blk_x);
    memcpy(s.blk_y, job.blk_y, sizeof s.blk_y);
}

// Dispose() as the reference runs it (dispose_pass_kernel), then the store goes to the writer as it is
void DeviceBatch::plan_dispose_job(int j, bool listed) {
    const ScanJob &job = jobs_[j];
    h_scans_[j].reserved0 |= kScanStoreHoldsSamples;
    DisposeJob dj;
    memset(&dj, 0, sizeof dj);
    dj.bpm = (uint32_t)job.blocks_per_mcu;
    dj.level_shift = 1u << (job.geo.frame.precision - 1);
    memcpy(dj.blk_comp, job.blk_comp, sizeof dj.blk_comp);
    for (int c = 0; c < kMaxScanComponents; c++) {
        dj.n[c] = job.dispose_n[c];
        for (int t = 0; t < job.dispose_n[c]; t++) dj.quant[c][t] = quant_index(job.dispose_q[c][t]);
    }
    dj.n_blocks = 0xFFFFFFFFu;  // (marks "scan index in coef_off": resolved by resolve_offsets, once the store's place is known)
    dj.coef_off = (uint64_t)j;
    if (listed) dispose_jobs_.push_back(dj);
}

// One entropy scan of a progressive frame: its launch group, its dependencies, the kernel it takes and its chain.
void DeviceBatch::plan_progressive_scan(UploadPlan &p, const ImagePlan &img, int j) {
    const ScanJob &job = jobs_[j];
    DevScan &s = h_scans_[j];
    // launch groups: dependency levels; JPGPU_PROG_BY_SCAN=1 (profiling aid): scan k of every frame in a launch of its
    // own, in file order -- one kernel duration per scan kind of the script (tools/trace/progressive_by_scan.sh)
    const bool by_scan = p.sw.prog_by_scan || prog_by_scan_;
    const int ordinal = by_scan ? j - img.jobs[0] - 1 : job.ordinal;
    prog_scans_++;
    prog_max_deps_ = std::max(prog_max_deps_, (int)job.n_deps);
    if (by_scan) prog_pipelined_ = false;
    if ((size_t)ordinal >= p.prog_work_by_ordinal.size()) {
        p.prog_work_by_ordinal.resize((size_t)ordinal + 1);
        p.prog_streams_by_ordinal.resize((size_t)ordinal + 1);
    }
    // the frame job precedes its scans in the job list: scan k of the frame is job img.jobs[0] + 1 + k
    for (int d = 0; d < 3; d++) s.dep[d] = d < job.n_deps && job.deps[d] >= 0 ? (uint32_t)(img.jobs[0] + 1 + job.deps[d]) : kNoDep;
    s.publishes = job.has_consumers ? 1 : 0;
    // test hook: "k:ms" makes scan k (0-based, in file order) of every progressive frame slow: it idles ms at its start and
    // after every progress word -- a producer its followers catch up with, which the launches only produce by chance
    if (p.sw.dbg_delay_scan >= 0 && p.sw.dbg_delay_scan == j - img.jobs[0] - 1) s.debug_delay_ms = (uint8_t)std::min(255, std::max(0, p.sw.dbg_delay_ms));
    // an AC scan whose band is empty (Ss > Se: a corrupted header; the reference's loops over the band then never run and
    // the scan reads no bit) goes to the lane kernel, whose loops are the reference's: the stream kernel's block decoders
    // are written for a band of at least one coefficient (tests/golden/stress/progressive_se_below_ss_122.jpg)
    const bool empty_band = job.ss != 0 && job.ss > job.se;
    if (job.n_deps > 3 || s.n_intervals != 1 || s.n_intervals > p.sw.stream_max_intervals || empty_band || job.force_lane) prog_pipelined_ = false;
    if (s.n_intervals <= p.sw.stream_max_intervals && !job.force_lane && !empty_band) {
        for (uint32_t i = 0; i < s.n_intervals; i++) p.prog_streams_by_ordinal[ordinal].push_back({(uint32_t)j, i});
        const int chain = progressive_chain(job);
        int in_chain = 0;
        for (int jj = img.jobs[0] + 1; jj < j; jj++) in_chain += progressive_chain(jobs_[jj]) == chain;
        if (p.prog_chain_work[chain].size() <= (size_t)in_chain) p.prog_chain_work[chain].resize((size_t)in_chain + 1);
        prog_chain_scans_[chain]++;
        for (uint32_t i = 0; i < s.n_intervals; i++) p.prog_chain_work[chain][(size_t)in_chain].push_back({(uint32_t)j, i});
    } else {
        prog_chains_ok_ = false;  // a scan of many restart intervals (lane kernel): level by level
        for (uint32_t first = 0; first < s.n_intervals; first += 256) p.prog_work_by_ordinal[ordinal].push_back({(uint32_t)j, first});
    }
    compressed_bytes_ += s.data_len;
}

// A scan with a store of its own: the store advances, then the entropy work -- K2S, or K2 and whether it hands over half-line planes.
void DeviceBatch::plan_entropy_work(UploadPlan &p, size_t ii, int j) {
    ImagePlan &img = images_[ii];
    const ScanJob &job = jobs_[j];
    DevScan &s = h_scans_[j];
    const uint64_t nblocks = (uint64_t)s.mcus_per_line * s.mcus_per_column * s.blocks_per_mcu;
    if (job.kind == kScanFrameOnly && !img.replay_skip) prog_clear_.push_back({p.coef_off, nblocks});
    p.coef_off += nblocks;
    p.real_blocks += nblocks;
    img.total_blocks += nblocks;
    compressed_bytes_ += s.data_len;
    if (job.kind == kScanFrameOnly) return;  // the Dispose() pass: IDCT work only
    // scans without restart intervals are decoded by the self-synchronising subsequence decoder (K2S)
    bool null_table = false;
    for (int c = 0; c < job.scan_components; c++) null_table |= job.dc_slot[c] == kNullHuffSlot || job.ac_slot[c] == kNullHuffSlot;
    const bool use_subseq = s.dri == 0 && s.total_mcus > 0 && s.data_len >= 512 && !null_table && !p.sw.no_subseq &&
                            !(entropy_only_ && ii < preset_no_subseq_.size() && preset_no_subseq_[ii]);
    if (use_subseq) {
        s.sub_shift = (uint8_t)p.subseq_shift;
        sub_shift_used_ = (int)p.subseq_shift;
        s.n_subs = (uint32_t)((((uint64_t)s.data_len * 8) + ((1u << p.subseq_shift) - 1)) >> p.subseq_shift);
        s.sub_off = total_subs_;
        total_subs_ += s.n_subs;
        max_subs_per_scan_ = std::max(max_subs_per_scan_, s.n_subs);
        if (!img.replay_skip) {
            sub_scan_ids_.push_back((uint32_t)j);
            for (uint32_t first = 0; first < s.n_subs; first += 256) p.sub_work.push_back({(uint32_t)j, first});
        }
        return;
    }
    for (uint32_t first = 0; first < s.n_intervals && !img.replay_skip; first += p.huff_intervals_per_wg) p.huff_work.push_back({(uint32_t)j, first});
    // Half-line planes for the scans K2's interval decoder writes, where the image is this one scan: its region is the
    // image's, and the padding (an even count of whole intervals) goes behind it.  (The scans of a multi-scan image lie back
    // to back in one dense run of the image's blocks, which is what the coefficient readers hand out: they stay dense.)
    // (a windowed image's scan is always handed over dense: the split form of K3 would need a window variant of its own)
    // (... and so is an oriented image's and a filtered one's: its samples go through the scratch image, which only the generic class fills)
    // (... and a grey image's, on either road: K3Y reads component 0's blocks at their places in the dense store, the scratch road is the generic class)
    // (... and the scans of an image that takes libjpeg's transform: K3J reads every block at its place in the dense store)
    const bool split_wanted = !p.sw.handoff_dense && !entropy_only_ && !keep_canvas_ && !img.windowed && img.orientation == 1 && !img.fancy && img.luma == kLumaNone && !img.islow, split_always = p.sw.handoff_set;
    const int k3_class = fmt_is_interleaved(format_) && !color_kind_by_file(img.color_kind) && img.orientation == 1 && !img.fancy && img.luma == kLumaNone && !img.islow ? idct_layout_class(s) : 0;
    // (an image the replay of failed progressive frames leaves alone keeps this form: its planes and flag words are the first pass's, at the
    // first pass's places, and the coefficient readers expand them from the descriptors of whichever plan is in force)
    if (split_wanted && job.kind == kScanSequential && s.dri != 0 && img.jobs.size() == 1 && s.total_mcus > 0 &&
        s.blocks_per_mcu != 0 && k3_variant(format_, k3_class, kK3Split).exists &&
        // The planes pay where few blocks reach into coefficients 32..63; all that is known of that in front of the decode is
        // how many bytes of entropy data a block has.  Q75 content has 5.4 (3 % of the blocks flagged; the step 4.9 % faster),
        // Q85 8.7, Q90 12.3 (66 % flagged: K2 gains 0.12 ms, K3 loses 0.19: 1.8 % slower) -- RESULTS.md, first section.
        (split_always || (uint64_t)s.data_len <= nblocks * kSplitMaxBytesPerBlock)) {
        // (in front of every scan's flag words, one whole line: the zero bytes K3 fetches for unflagged blocks)
        p.flag_words = (p.flag_words + kSplitZeroWords - 1) / kSplitZeroWords * kSplitZeroWords + kSplitZeroWords;
        s.reserved0 |= kScanSplitHandoff | (p.flag_words << kSplitFlagShift);  // (the buffer-relative base is added by resolve_offsets)
        p.flag_words += split_flag_words(s.n_intervals, s.dri, s.blocks_per_mcu);
        p.coef_off += split_region_blocks(s.n_intervals, s.dri, s.blocks_per_mcu) - nblocks;
        split_scans_.push_back((uint32_t)j);
        split_max_blocks_ = std::max<uint32_t>(split_max_blocks_, (uint32_t)nblocks);
    }
}

// no fused conversion for a scan of image ii: its samples go to the scratch image, then ycc_to_rgb_kernel (once per image) -- or, for an image
// of kind RGB, CMYK or YCCK, the batch's one K3C launch (plan_color_convert) -- or, for an image of any kind whose orientation is not 1, the
// batch's one K3O launch (plan_orient_convert), which converts as well.  An image that is filtered (JPGPU_UPSAMPLE_FANCY) is listed for the
// batch's one K3U call (plan_fancy_convert) in place of the first two, and for K3O besides if it is turned
void DeviceBatch::list_rgb_convert(size_t ii) {
    const ImagePlan &img = images_[ii];
    auto list_in = [&](std::vector<RgbConvert> &list) {
        for (const RgbConvert &rc : list)
            if (rc.image == (uint32_t)ii) return;
        list.push_back({(uint32_t)ii, img.out_offset, (uint64_t)img.win.width * img.win.height, img.num_components});  // (the window's pixels)
    };
    if (img.luma != kLumaNone) {  // (one list, whatever its kind and orientation, and none of the four others)
        list_in(luma_convert_);
        return;
    }
    if (img.fancy) list_in(fancy_convert_);
    if (img.orientation != 1) list_in(orient_convert_);
    else if (!img.fancy) list_in(color_kind_by_file(img.color_kind) ? color_convert_ : rgb_convert_);
}

// K3's work for one scan: tile size and alignment, layout class, scratch conversion, ordering level, work entries, the partial-MCU entry.
void DeviceBatch::plan_idct_work(UploadPlan &p, size_t ii, int j, bool overlapping_scans) {
    const ImagePlan &img = images_[ii];
    const ScanJob &job = jobs_[j];
    DevScan &s = h_scans_[j];
    if (img.luma == kLumaFast) {  // (no entry in any K3 list, nor in a conversion list: K3Y's own work)
        plan_luma_work(ii, j);
        return;
    }
    const bool rgb_out = fmt_is_rgb(format_);
    // An image that takes libjpeg's transform (JPGPU_ARITHMETIC_LIBJPEG): no entry in any K3 list -- K3J's own work, which leaves the samples in
    // the scratch image where the generic class would, for the conversion the image is listed for.  (Not where the store holds samples by now:
    // the second issue of a progressive file that failed runs Dispose() literally, and K3 flushes what it left.)
    if (img.islow && (s.reserved0 & kScanStoreHoldsSamples) == 0) {
        list_rgb_convert(ii);
        p.scan_level[(size_t)j] = 0;
        plan_islow_work(ii, j);  // (K3J's list at full size, K3R's at a reduced one)
        return;
    }
    // (... decoded at a reduced size: no K3 form writes a reduced picture, and its slot is too small for the frame.  The second issue of such a
    // file lists no transform: the slot keeps what K3R left in it at the first issue, and the conversion runs on that.)
    if (img.scale > 1) {
        list_rgb_convert(ii);
        p.scan_level[(size_t)j] = 0;
        return;
    }
    const uint32_t generic_per_wg = (uint32_t)kIdctBlocksPerWg / s.blocks_per_mcu;
    uint32_t mcus_per_wg = generic_per_wg;
    if (p.sw.tile_align) {
        // a tile whose pixel rows are whole 128-byte lines: neighbouring tiles (other workgroups, other XCDs, other
        // L2s) never write two halves of one line
        uint32_t row_bytes = 8u * s.max_h;
        if (fmt_is_sample_bytes(format_)) row_bytes *= s.frame_components;
        else if (format_ == JPGPU_FMT_RGB_U8) row_bytes *= 3;
        else if (format_ == JPGPU_FMT_RGBA_U8) row_bytes *= 4;
        else if (format_ == JPGPU_FMT_PLANAR_I16 || format_ == JPGPU_FMT_EXTENDED_U16) row_bytes *= 2;
        else if (fmt_is_rgb_planes(format_)) row_bytes *= fmt_rgb_plane_sample_bytes(format_);
        // (RGB_PLANAR_U8 like PLANAR_U8: one byte per pixel in each plane's row; its float forms two or four)
        for (uint32_t t = mcus_per_wg; t * 4 >= mcus_per_wg * 3 && t > 0; t--)
            if ((t * row_bytes) % 128 == 0) {
                mcus_per_wg = t;
                break;
            }
    }
    const bool holds_samples = (s.reserved0 & kScanStoreHoldsSamples) != 0;
    // (a windowed image: today's rule with the window's width, and its first column on an MCU boundary -- idct_window_layout_class)
    int cls = holds_samples ? kIdctClassStoreHoldsSamples
                            : (fmt_is_interleaved(format_) ? (img.windowed ? idct_window_layout_class(s, format_) : idct_layout_class(s)) : 0);
    // RGB / RGBA of a frame with overlapping scans (below): every scan's samples go to the scratch image in file order and
    // are converted at the end -- a fused conversion of one scan would be overwritten by the scratch image's
    if (!holds_samples && overlapping_scans && rgb_out) cls = 0;
    // ... and so do the samples of an image whose kind is RGB, CMYK or YCCK (JPGPU_COLOR_FILE): the fused classes convert YCbCr and grey
    if (!holds_samples && color_kind_by_file(img.color_kind)) cls = 0;
    // ... and of an image that is turned on its way out (orientation 2..8): the scratch image is what K3O reads
    if (!holds_samples && img.orientation != 1) cls = 0;
    // ... and of an image whose chroma is filtered (JPGPU_UPSAMPLE_FANCY): the scratch image is what K3U reads
    if (!holds_samples && img.fancy) cls = 0;
    // ... and of a grey image on the scratch road: the scratch image is what K3Y's luma_plane_kernel reads
    if (!holds_samples && img.luma == kLumaScratch) cls = 0;
    if ((cls == 0 || holds_samples) && rgb_out) list_rgb_convert(ii);
    // A baseline frame whose LATER scans write a component this one writes too (a corrupted selector: one component
    // scanned twice, another never): in the reference the later WriteBlock wins -- where the later scan GOT to; a later
    // scan that fails or ends early leaves this scan's samples behind its last block -- and two scans' tiles in one
    // launch have no order.  Such a later scan is ORDERED behind the scans it overlaps: its transform goes to a later
    // launch (level = 1 + the highest level among the earlier scans sharing a component with it), on the bytewise form,
    // touching nothing it did not reach (kKeepUnreachedMcus).  Round 4 left the earlier scan's transform out when the
    // later scans covered all its components (wrong when they were truncated) and did not order partial overlaps.
    int level = 0;
    if (job.kind == kScanSequential && img.jobs.size() > 1) {
        for (int j2 : img.jobs) {
            if (j2 == j) break;
            const ScanJob &o = jobs_[(size_t)j2];
            if (o.kind != kScanSequential || o.disabled) continue;
            if (component_mask(job) & component_mask(o)) level = std::max(level, p.scan_level[(size_t)j2] + 1);
        }
    }
    p.scan_level[(size_t)j] = level;
    if (level > 0) {
        s.shadow_mask |= kKeepUnreachedMcus;
        if ((size_t)level > p.idct_later_levels.size()) p.idct_later_levels.resize((size_t)level);
        if ((size_t)level > p.idct_later_win_levels.size()) p.idct_later_win_levels.resize((size_t)level);
        if (img.windowed) {  // (any superset of the window's MCUs will do on the later levels: the whole grid, whose numbering is the scan's)
            s.cov_x = s.cov_y = 0;
            s.cov_cols = (uint16_t)s.mcus_per_line;
            s.cov_rows = (uint16_t)s.mcus_per_column;
        }
        const uint32_t grun = generic_per_wg * p.idct_tiles_per_wg;
        std::vector<IdctWork> &later = img.windowed ? p.idct_later_win_levels[(size_t)level - 1] : p.idct_later_levels[(size_t)level - 1];
        for (uint32_t first = 0; first < s.total_mcus; first += grun)
            later.push_back({(uint32_t)j, first, std::min(grun, s.total_mcus - first), generic_per_wg});
        if (rgb_out) list_rgb_convert(ii);  // (bytewise form: samples to the scratch image, then ycc_to_rgb_kernel)
    } else {
        const uint32_t run = mcus_per_wg * p.idct_tiles_per_wg;
        std::vector<IdctWork> &list = img.windowed ? p.idct_win_by_class[cls] : (s.reserved0 & kScanSplitHandoff) ? p.idct_split_by_class[cls] : p.idct_work_by_class[cls];
        // (a windowed image: the MCUs of its cover, counted as a raster of their own; tiles stay full)
        const uint32_t listed = img.windowed ? (uint32_t)s.cov_cols * s.cov_rows : s.total_mcus;
        for (uint32_t first = 0; first < listed; first += run)
            list.push_back({(uint32_t)j, first, std::min(run, listed - first), mcus_per_wg});
        // the caller's canvas under a whole-pixel layout: the MCU a failing scan stops in is written block by block
        if (keep_canvas_ && job.kind == kScanSequential && fmt_is_sample_bytes(format_) &&
            (cls == kLayYccH1V1 || cls == kLayYccH2V1 || cls == kLayYccH2V2))
            p.idct_partial.push_back({(uint32_t)j, kIdctPartialMcu, 1, generic_per_wg});
    }
}

// What needs every scan's final place: the Dispose jobs' stores, the totals, the flag words' base; K1's lists are complete too.
void DeviceBatch::resolve_offsets(UploadPlan &p) {
    for (DisposeJob &dj : dispose_jobs_) {  // the frames' stores have their places now
        const DevScan &fs = h_scans_[(size_t)dj.coef_off];
        dj.coef_off = fs.coef_off;
        dj.n_blocks = fs.total_mcus * (uint32_t)fs.blocks_per_mcu;
        dispose_max_blocks_ = std::max(dispose_max_blocks_, dj.n_blocks);
    }
    total_blocks_ = p.real_blocks;
    coef_store_blocks_ = p.coef_off;
    // the flag words of the split scans lie behind the blocks and the tile of slack, in the same buffer
    for (uint32_t j : split_scans_) h_scans_[j].reserved0 += ((coef_store_blocks_ + (uint64_t)kIdctBlocksPerWg) * 16) << kSplitFlagShift;
    out_bytes_ = p.out_off;
    planes_bytes_ = p.planes_off;
    total_ends_ = p.ends_off;
    n_chunk_work_ = (int)p.chunk_work.size();
    std::stable_sort(p.k1_order.begin(), p.k1_order.end(), [](const ChunkWork &a, const ChunkWork &b) { return a.chunk < b.chunk; });
    n_k1_groups_ = (int)p.k1_order.size();
}

// K2's work.  Runs of consecutive scans that stage the same tables in the same slots (all of a batch of files from one encoder,
// typically) are POOLED (round 6; the K2S final pass below has had it since round 5): one entry per WAVE of 64 restart intervals,
// taken from a counter by the waves of one workgroup per CU (huffman_pool_kernel).  Everything else keeps a workgroup per
// huffman_waves() * 64 intervals of one scan.  (JPGPU_OVERLAP, the opt-in two-stream issue order, cuts the plain list in two: no pools then.)
void DeviceBatch::pool_huffman_runs(UploadPlan &p) {
    std::vector<HuffWork> &huff_work = p.huff_work;
    k2_pools_.clear();
    std::vector<HuffWork> plain, pooled;
#ifdef JPGPU_K2_NO_POOL  // (A/B build variant: tools/trace/ab_build.sh "-DJPGPU_K2_NO_POOL" ...)
    const bool no_pool = true;
#else
    const bool no_pool = p.sw.overlap;
#endif
    for (size_t i = 0, k; i < huff_work.size() && !no_pool; i = k) {
        k = same_tables_run(h_scans_, i, huff_work.size(), [&](size_t q) { return huff_work[q].scan; });
        uint64_t chunks = 0;
        for (size_t q = i; q < k; q++)
            if (huff_work[q].first_interval == 0) chunks += (h_scans_[huff_work[q].scan].n_intervals + 63u) / 64u;
        const bool pool = (int)k2_pools_.size() < kK2MaxPools && chunks >= 2 && chunks < 0x7FFFFFFFu;
        if (pool) k2_pools_.push_back({(int)pooled.size(), (int)chunks});
        for (size_t q = i; q < k; q++) {
            if (!pool) plain.push_back(huff_work[q]);
            else if (huff_work[q].first_interval == 0)
                for (uint32_t first = 0; first < h_scans_[huff_work[q].scan].n_intervals; first += 64u) pooled.push_back({huff_work[q].scan, first});
        }
    }
    if (!no_pool) huff_work.swap(plain);
    n_huff_work_ = (int)huff_work.size();
    huff_work.insert(huff_work.end(), pooled.begin(), pooled.end());  // (one buffer: the pooled list behind the plain one)
}

// K2S: the table sets of the round kernel's lookups, the gather list of the later rounds, the final pass and its pools.
void DeviceBatch::plan_subseq_lists(UploadPlan &p) {
    // The K2S round kernel's lookups: one set per distinct set of tables among the DRI = 0 scans (one for a batch from one encoder),
    // built once per upload (sr_lut_build_kernel) -- the workgroups of every round built them themselves until round 6.
    for (uint32_t j : sub_scan_ids_) {
        uint32_t k = 0;
        while (k < p.sr_set_scan.size() && !same_tables(h_scans_[p.sr_set_scan[k]], h_scans_[j])) k++;
        if (k == p.sr_set_scan.size()) p.sr_set_scan.push_back(j);
        h_scans_[j].sr_set = k;
    }
    n_sr_sets_ = (int)p.sr_set_scan.size();
    n_sub_work_ = (int)p.sub_work.size();
    // ... and the list of the rounds behind round 1 (a workgroup per kSubseqGatherSpan subsequences), behind it in the same buffer
    for (uint32_t j : sub_scan_ids_)
        for (uint32_t first = 0; first < h_scans_[j].n_subs; first += kSubseqGatherSpan) p.sub_work.push_back({j, first});
    n_sub_gather_ = (int)p.sub_work.size() - n_sub_work_;
    // The final pass.  Runs of consecutive scans that stage the same tables in the same slots (all of a batch of files from one
    // encoder, typically) are POOLED: one entry per wave of 64 lanes, taken from a counter by the waves of one workgroup per CU
    // (k2s_subseq.hip).  Everything else takes a workgroup per subseq_final_waves() waves of one scan.
    sub_pools_.clear();
#ifdef JPGPU_SF_NO_POOL  // (A/B build variants since round 6: tools/trace/ab_build.sh "-DJPGPU_SF_NO_POOL" ...)
    const bool no_pool = true;
#else
    const bool no_pool = !subseq_pool_fits(k2_tab_bytes_);  // (ten waves + the tables must fit a CU)
#endif
    // (a batch that cannot fill the machine with two subsequences per lane takes one: twice the waves, half as long each)
#ifdef JPGPU_SF_ONE_SUB  // (A/B build variant)
    sub_final_spl_ = 1;
#else
    sub_final_spl_ = (kSubFinalSubsPerLane >= 2 && total_subs_ >= p.sw.subseq_two_per_lane_from) ? 2 : 1;
#endif
    const uint32_t lanes_subs = 64u * (uint32_t)sub_final_spl_;
    std::vector<HuffWork> pooled;
    for (size_t i = 0, k; i < sub_scan_ids_.size(); i = k) {
        k = same_tables_run(h_scans_, i, sub_scan_ids_.size(), [&](size_t q) { return sub_scan_ids_[q]; });
        uint64_t waves = 0;
        for (size_t q = i; q < k; q++) waves += (h_scans_[sub_scan_ids_[q]].n_subs + lanes_subs - 1) / lanes_subs;
        const bool pool = !no_pool && waves >= (uint64_t)kSubFinalPoolMinChunks && (int)sub_pools_.size() < kSubFinalMaxPools && waves < 0x7FFFFFFFu;
        if (pool) sub_pools_.push_back({(int)pooled.size(), (int)waves});
        for (size_t q = i; q < k; q++) {
            const uint32_t j = sub_scan_ids_[q];
            const uint32_t step = pool ? lanes_subs : lanes_subs * (uint32_t)subseq_final_waves();
            for (uint32_t first = 0; first < h_scans_[j].n_subs; first += step) (pool ? pooled : p.sub_final_work).push_back({j, first});
        }
    }
    n_sub_final_work_ = (int)p.sub_final_work.size();
    p.sub_final_work.insert(p.sub_final_work.end(), pooled.begin(), pooled.end());  // (one buffer: the pooled list behind the plain one)
    n_sub_scans_ = (int)sub_scan_ids_.size();
}

// The progressive work list: the lane kernel's entries by ordinal, the stream kernel's by ordinal, the pipelined launch's own list,
// the stream work once more by chain.  (prog_pipelined_ is complete here: every scan has been visited.)
void DeviceBatch::assemble_progressive_lists(UploadPlan &p) {
    std::vector<HuffWork> &prog_work = p.prog_work;
    prog_begin_.assign(1, 0);
    for (const std::vector<HuffWork> &w : p.prog_work_by_ordinal) {
        prog_work.insert(prog_work.end(), w.begin(), w.end());
        prog_begin_.push_back((int)prog_work.size());
    }
    prog_stream_begin_.assign(1, (int)prog_work.size());
    for (const std::vector<HuffWork> &w : p.prog_streams_by_ordinal) {
        prog_work.insert(prog_work.end(), w.begin(), w.end());
        prog_stream_begin_.push_back((int)prog_work.size());
    }
    // The pipelined launch's list.  Fewer waves per frame let more frames share one resident launch (8 instead of 10: 512 frames
    // instead of 409 with two Huffman tables staged; at 256 frames the launch is as fast either way -- what made it slower than
    // a 32-frame launch was the release fences, see progressive_stream_kernel): a scan whose ONLY producer is a cheap scan, and
    // that is cheap itself, runs behind its producer in the same wave -- it could not have overtaken it anyway.  "Cheap": the wave's entropy bytes stay under half of the frame's largest scan (the
    // long pole is left alone) and under 1 MiB, nothing follows the chained scan, and it is an AC scan.  libjpeg's script: Cr first ->
    // Cr refinement, Cb first -> Cb refinement: 8 waves per frame instead of 10.
    prog_pipe_begin_ = (int)prog_work.size();
    std::vector<uint8_t> is_tail(h_scans_.size(), 0);  // scans that run behind their producer: no entry of their own in the pipelined list
    for (const ImagePlan &img : images_) {
        if (img.jobs.size() < 2 || p.sw.no_wave_chains) continue;
        const int j0 = img.jobs[0] + 1, n = (int)img.jobs.size() - 1;  // the frame job precedes its scans
        uint64_t largest = 0;
        // (a scan's own entropy bytes: DevScan::data_len; ScanJob::entropy_len runs to the end of the file)
        for (int k = 0; k < n; k++)
            if (jobs_[(size_t)(j0 + k)].kind == kScanProgressive) largest = std::max<uint64_t>(largest, h_scans_[(size_t)(j0 + k)].data_len);
        std::vector<uint64_t> wave_bytes((size_t)n, 0);  // of the wave that ENDS with scan k
        std::vector<uint8_t> has_next((size_t)n, 0);
        for (int k = 0; k < n; k++) {
            const ScanJob &job = jobs_[(size_t)(j0 + k)];
            if (job.kind != kScanProgressive) continue;
            const uint64_t own = h_scans_[(size_t)(j0 + k)].data_len;
            wave_bytes[(size_t)k] = own;
            // (only a scan nobody follows: behind its producer it starts later than it would beside it, and whatever waited
            // for it would start later too -- Y AC 1-5 -> Y AC 6-63 -> Y refinement in one wave put 60 ms in front of the
            // last luma refinement)
            if (job.n_deps != 1 || job.deps[0] < 0 || job.deps[0] >= k || job.has_consumers) continue;
            // (not a DC refinement: 7 waves per frame instead of 8 only helps batches of 513-585 frames and has not been
            // measured since the wrong frame once seen with it turned out to be the end-of-band skip in the stream kernel)
            if (job.scan_components != 1 || job.ss == 0) continue;
            const int a = job.deps[0];
            if (jobs_[(size_t)(j0 + a)].kind != kScanProgressive || has_next[(size_t)a] || k - a > 255) continue;
            const uint64_t together = wave_bytes[(size_t)a] + own;
            if (together > largest / 2 || together > (1u << 20)) continue;
            if (p.sw.dbg_status && &img == &images_[0])
                fprintf(stderr, "jpgpu: wave chain: scan %d behind scan %d (%llu + %llu bytes, largest scan %llu)\n", k, a,
                        (unsigned long long)wave_bytes[(size_t)a], (unsigned long long)own, (unsigned long long)largest);
            h_scans_[(size_t)(j0 + a)].wave_next = (uint8_t)(k - a);
            has_next[(size_t)a] = 1;
            is_tail[(size_t)(j0 + k)] = 1;
            prog_wave_tails_++;
            wave_bytes[(size_t)k] = together;
        }
    }
    for (const std::vector<HuffWork> &w : p.prog_streams_by_ordinal)
        for (const HuffWork &hw : w)
            if (!is_tail[hw.scan]) prog_work.push_back(hw);
    prog_pipe_count_ = (int)prog_work.size() - prog_pipe_begin_;
    for (int x = 0; x < jpgpu_ctx::kProgChains; x++) {
        prog_chain_begin_[x].assign(1, (int)prog_work.size());
        for (const std::vector<HuffWork> &w : p.prog_chain_work[x]) {
            prog_work.insert(prog_work.end(), w.begin(), w.end());
            prog_chain_begin_[x].push_back((int)prog_work.size());
        }
    }
}

// Images whose scans do not cover every frame component (a scan header that names one component twice and another never;
// no scan at all): the reference leaves those samples of the caller's buffer alone.  The batch owns the output buffer,
// so "alone" is defined as zero, what a freshly allocated managed array holds.
void DeviceBatch::plan_output_clears() {
    out_clear_.clear();
    for (const ImagePlan &img : images_) {
        if (img.status != JPGPU_OK || img.out_bytes == 0) continue;
        // frame components are 0..254 (a baseline frame may carry up to 255; scans are capped at 4): a 256-bit set
        uint64_t covered[4] = {0, 0, 0, 0};
        for (int j : img.jobs) {
            const DevScan &s = h_scans_[j];
            if (jobs_[j].kind == kScanProgressive) continue;
            for (int c = 0; c < s.scan_components; c++) covered[s.comp[c].component_index >> 6] |= 1ull << (s.comp[c].component_index & 63);
        }
        bool all = true;
        // ... and a component whose sampling factor is neither the frame's maximum nor 1 (round 6): the decoder's (offsetX + x) * 8
        // placement leaves the last columns / rows of every MCU unwritten (k3_idct.hip, interleaved_output_from_tile)
        for (int j : img.jobs) {
            const DevScan &s = h_scans_[j];
            if (jobs_[j].kind != kScanSequential) continue;  // (a progressive frame's Flush places the blocks side by side)
            for (int c = 0; c < s.scan_components; c++) all &= !((s.comp[c].h > 1 && s.comp[c].hs > 1) || (s.comp[c].v > 1 && s.comp[c].vs > 1));
        }
        for (int c = 0; c < img.num_components; c++) all &= ((covered[c >> 6] >> (c & 63)) & 1ull) != 0;
        if (!all && !img.replay_skip) out_clear_.push_back({img.out_offset, img.out_bytes, img.planes_offset, img.planes_bytes, slot_bytes(img)});
        // RGB / RGBA = the callers' converter applied to the YCbCr8 buffer (DecodeAction.cs:71-74): an image without any scan
        // leaves that buffer as it was (zero here), and the converter still runs over it
        if (img.jobs.empty() && !img.replay_skip && fmt_is_rgb(format_)) list_rgb_convert((size_t)(&img - images_.data()));
    }
}

// The descriptors of the K3C launch: one per image of kind RGB, CMYK or YCCK whose samples go through the scratch image.
void DeviceBatch::plan_color_convert() {
    color_images_.clear();
    color_max_pixels_ = 0;
    for (const RgbConvert &rc : color_convert_) {
        color_images_.push_back({rc.out_offset, rc.out_offset, rc.pixels, (uint32_t)images_[rc.image].color_kind, 0u});
        color_max_pixels_ = std::max(color_max_pixels_, rc.pixels);
    }
}

// K3's list: class by class (dense scans, then split scans, each interleaved over the XCDs), the ordered levels, the partial-MCU entries.
void DeviceBatch::assemble_idct_lists(UploadPlan &p) {
    std::vector<IdctWork> &idct_work = p.idct_work;
    idct_class_begin_[0] = 0;
    for (int c = 0; c < kNumIdctLayoutClasses; c++) {
        std::vector<IdctWork> &w = p.idct_work_by_class[c];
        xcd_interleave(w, p.sw.xcds);
        idct_work.insert(idct_work.end(), w.begin(), w.end());
        idct_split_begin_class_[c] = (int)idct_work.size();
        std::vector<IdctWork> &ws = p.idct_split_by_class[c];
        xcd_interleave(ws, p.sw.xcds);
        idct_work.insert(idct_work.end(), ws.begin(), ws.end());
        idct_class_begin_[c + 1] = (int)idct_work.size();
    }
    idct_win_class_begin_[0] = (int)idct_work.size();
    for (int c = 0; c < kNumIdctLayoutClasses; c++) {
        std::vector<IdctWork> &w = p.idct_win_by_class[c];
        xcd_interleave(w, p.sw.xcds);
        idct_work.insert(idct_work.end(), w.begin(), w.end());
        idct_win_class_begin_[c + 1] = (int)idct_work.size();
    }
    n_idct_work_ = (int)idct_work.size();
    idct_later_begin_.assign(1, n_idct_work_);
    idct_later_win_.clear();
    for (size_t lv = 0; lv < std::max(p.idct_later_levels.size(), p.idct_later_win_levels.size()); lv++)
        for (int win = 0; win < 2; win++) {
            const std::vector<std::vector<IdctWork>> &levels = win ? p.idct_later_win_levels : p.idct_later_levels;
            if (lv >= levels.size() || levels[lv].empty()) continue;
            idct_work.insert(idct_work.end(), levels[lv].begin(), levels[lv].end());
            idct_later_begin_.push_back((int)idct_work.size());
            idct_later_win_.push_back((uint8_t)win);
        }
    if (!p.idct_partial.empty()) {
        idct_work.insert(idct_work.end(), p.idct_partial.begin(), p.idct_partial.end());
        idct_later_begin_.push_back((int)idct_work.size());
        idct_later_win_.push_back(0);
    }
    idct_listed_mcus_ = 0;
    for (const IdctWork &w : idct_work) idct_listed_mcus_ += w.n_mcus;
}

// ---- two halves for decode()'s overlapped issue order (see decode()): images [0, half_image) and [half_image, n), balanced by
// blocks; the Huffman work list is in image order already (one index cuts it), the IDCT work gets a second list with
// the classes of each half interleaved over the XCDs on their own
// The descriptors of the K3O launch: one per image whose orientation is not 1, with the stored window K3 leaves in the scratch image.
void DeviceBatch::plan_orient_convert() {
    orient_images_.clear();
    orient_max_tiles_ = 0;
    for (const RgbConvert &rc : orient_convert_) {
        const ImagePlan &img = images_[rc.image];
        // (a filtered image: what K3U staged behind the fetch rectangle, (Y, Cb', Cr') of the stored window)
        const uint64_t src_off = rc.out_offset + (img.fancy ? fancy_staging_offset(img) : 0u);
        orient_images_.push_back({src_off, rc.out_offset, img.win.width, img.win.height, (uint32_t)img.color_kind, (uint32_t)img.orientation});
        orient_max_tiles_ = std::max(orient_max_tiles_, orient_tiles(img.win.width, img.win.height));
    }
}

// The descriptors of the K3U call: one per filtered image, with the fetch rectangle K3 leaves in the scratch image and the stored window
// that comes out of it -- to the output, or to the staging slot of an image K3O turns afterwards.
void DeviceBatch::plan_fancy_convert() {
    fancy_images_.clear();
    fancy_max_tiles_ = 0;
    n_fancy_staged_ = 0;
    for (const RgbConvert &rc : fancy_convert_) {
        const ImagePlan &img = images_[rc.image];
        const jpgpu_rect f = fancy_fetch_rect(img);
        const bool staged = img.orientation != 1;
        FancyImage g;
        g.src_off = rc.out_offset;
        g.dst_off = rc.out_offset + (staged ? fancy_staging_offset(img) : 0u);
        g.fetch_x = f.x, g.fetch_y = f.y, g.fetch_w = f.width;
        g.win_x = img.win.x, g.win_y = img.win.y, g.win_w = img.win.width, g.win_h = img.win.height;
        g.hs = img.chroma_hs, g.vs = img.chroma_vs;
        g.cw = k3u_chroma_extent(img.pic_w, g.hs), g.ch = k3u_chroma_extent(img.pic_h, g.vs);
        g.staged = staged ? 1u : 0u;
        n_fancy_staged_ += staged ? 1 : 0;
        fancy_images_.push_back(g);
        fancy_max_tiles_ = std::max(fancy_max_tiles_, fancy_tiles(img.win.width, img.win.height));
    }
}

// K3Y's work for the one scan of an image on the fast road: the luma blocks of the window's MCU cover, row by row, in units of
// kLumaUnitBlocks neighbouring blocks, kLumaUnitsPerWg consecutive units per workgroup.
void DeviceBatch::plan_luma_work(size_t ii, int j) {
    const ImagePlan &img = images_[ii];
    const DevScan &s = h_scans_[j];
    n_luma_fast_++;
    luma_work_windowed_ |= img.windowed;
    const uint32_t cols = (uint32_t)s.cov_cols * s.comp[0].h, rows = (uint32_t)s.cov_rows * s.comp[0].v;
    const uint32_t chunks = (cols + kLumaUnitBlocks - 1) / kLumaUnitBlocks;
    const uint64_t units = (uint64_t)chunks * rows;
    for (uint64_t u = 0; u < units; u += kLumaUnitsPerWg)
        luma_work_.push_back({(uint32_t)j, (uint32_t)(u / chunks), (uint32_t)(u % chunks), (uint32_t)std::min<uint64_t>(kLumaUnitsPerWg, units - u)});
}

// K3J's work for one scan of an image that takes libjpeg's transform: every block of the window's MCU cover, MCU row by MCU row, the blocks
// of kIslowThreads / blocks_per_mcu consecutive MCUs of a row per workgroup.  An image decoded at a reduced size: the same division in K3R's
// list, each entry with m = 8 / scale.
void DeviceBatch::plan_islow_work(size_t ii, int j) {
    const DevScan &s = h_scans_[j];
    const uint32_t row_blocks = (uint32_t)s.cov_cols * s.blocks_per_mcu, step = islow_blocks_per_wg(s.blocks_per_mcu);
    for (uint32_t row = 0; row < s.cov_rows; row++)
        for (uint32_t first = 0; first < row_blocks; first += step) {
            if (images_[ii].scale > 1) reduced_work_.push_back({(uint32_t)j, row, first, 8u / images_[ii].scale});
            else islow_work_.push_back({(uint32_t)j, row, first, 0u});
        }
}

// The descriptors of K3Y's scratch-road launch: one per grey image that is not on the fast road, with the stored window K3 leaves in the
// scratch image.
void DeviceBatch::plan_luma_convert() {
    luma_images_.clear();
    luma_max_tiles_ = 0;
    for (const RgbConvert &rc : luma_convert_) {
        const ImagePlan &img = images_[rc.image];
        luma_images_.push_back({rc.out_offset, rc.out_offset, img.win.width, img.win.height, (uint32_t)img.color_kind, (uint32_t)img.orientation});
        luma_max_tiles_ = std::max(luma_max_tiles_, orient_tiles(img.win.width, img.win.height));
    }
}

void DeviceBatch::plan_overlap_halves(UploadPlan &p) {
    overlap_ok_ = false;
    // OFF by default: with the round-2 kernels both stages are HBM-heavy (K2 writes the coefficient buffer at 4.7 TB/s)
    // and cannot share a CU (K2 takes 159 KB of its 160 KB LDS), so the halves time-slice instead of overlapping:
    // 16.39-16.52 ms overlapped vs 16.16-16.37 ms serial per 1024 x 4K (gpurun r02e, both issue orders below)
    const bool wanted = p.sw.overlap && dispose_jobs_.empty() && split_scans_.empty();  // (the generic Dispose() pass is issued by run_idct alone)
    uint32_t half_image = 0;
    uint64_t acc = 0;
    for (size_t ii = 0; ii < images_.size() && acc * 2 < total_blocks_; ii++) {
        acc += images_[ii].total_blocks;
        half_image = (uint32_t)ii + 1;
    }
    huff_half_ = 0;
    while (huff_half_ < n_huff_work_ && h_scans_[p.huff_work[huff_half_].scan].image_index < half_image) huff_half_++;
    // worth it for batches that keep the machine busy for milliseconds: the halves cost four launches and two events
    if (wanted && !entropy_only_ && p.sub_work.empty() && p.prog_work.empty() && total_blocks_ >= (4u << 20) && huff_half_ > 0 &&
        huff_half_ < n_huff_work_ && rgb_convert_.empty() && color_convert_.empty() && orient_convert_.empty() && fancy_convert_.empty() && luma_convert_.empty() && luma_work_.empty() && islow_work_.empty() && reduced_work_.empty() && format_ != JPGPU_FMT_EXTENDED_U16 && idct_later_begin_.size() == 1 &&
        idct_win_class_begin_[kNumIdctLayoutClasses] == idct_win_class_begin_[0]) {  // (no windowed image: the halves have no list for their work)
        for (int half = 0; half < 2; half++) {
            idct_half_begin_[half][0] = (int)p.idct_work_halves.size();
            for (int c = 0; c < kNumIdctLayoutClasses; c++) {
                std::vector<IdctWork> w;
                // idct_work_by_class[c] was interleaved by assemble_idct_lists: take the entries back in memory order
                for (const IdctWork &x : p.idct_work_by_class[c])
                    if ((h_scans_[x.scan].image_index < half_image) == (half == 0)) w.push_back(x);
                std::sort(w.begin(), w.end(), [](const IdctWork &a, const IdctWork &b) { return a.scan != b.scan ? a.scan < b.scan : a.first_mcu < b.first_mcu; });
                xcd_interleave(w, p.sw.xcds);
                p.idct_work_halves.insert(p.idct_work_halves.end(), w.begin(), w.end());
                idct_half_begin_[half][c + 1] = (int)p.idct_work_halves.size();
            }
        }
        overlap_ok_ = true;
    }
}

void DeviceBatch::init_status() {
    h_status_.assign(jobs_.size(), DevScanStatus());
    for (size_t j = 0; j < jobs_.size(); j++) {
        DevScanStatus &st = h_status_[j];
        memset(&st, 0, sizeof st);
        st.first_error = kNoError;
        st.decoded_mcus = h_scans_[j].total_mcus;
    }
}

// Allocate, copy, clear, build the lookups, copy the input, synchronise.  `ups` is the one place that says what goes to the device.
int DeviceBatch::upload_plan(const UploadPlan &p, const std::vector<const uint8_t *> &file_ptr, const std::vector<size_t> &file_len) {
    hipStream_t up = ctx_->upload_stream;  // everything an upload does stays off the decode stream
    hipError_t e;
    const DevUpload ups[] = {
        {&d_scans_, h_scans_.data(), h_scans_.size() * sizeof(DevScan), 0},
        {&d_status_, h_status_.data(), h_status_.size() * sizeof(DevScanStatus), 0},
        {&d_huff_pool_, huff_pool_.data(), huff_pool_.size() * sizeof(DevHuffTable), 0},
        {&d_quant_pool_, quant_pool_.data(), quant_pool_.size() * sizeof(DevQuantTable), 0},
        {&d_huff_work_, p.huff_work.data(), p.huff_work.size() * sizeof(HuffWork), 0},
        {&d_chunk_work_, p.chunk_work.data(), p.chunk_work.size() * sizeof(ChunkWork), 0},
        {&d_k1_order_, p.k1_order.data(), p.k1_order.size() * sizeof(ChunkWork), 16},
        {&d_sub_work_, p.sub_work.data(), p.sub_work.size() * sizeof(HuffWork), 0},
        {&d_sub_final_work_, p.sub_final_work.data(), p.sub_final_work.size() * sizeof(HuffWork), 0},
        {&d_prog_work_, p.prog_work.data(), p.prog_work.size() * sizeof(HuffWork), 0},
        {&d_prog_sync_, nullptr, 0, (size_t)(p.prog_work.empty() ? 0 : 256)},
        {&d_sub_scan_ids_, sub_scan_ids_.data(), sub_scan_ids_.size() * sizeof(uint32_t), 0},
        {&d_sub_exit_a_, nullptr, 0, (size_t)total_subs_ * sizeof(uint32_t) + 256},
        {&d_sub_exit_b_, nullptr, 0, (size_t)total_subs_ * sizeof(uint32_t) + 256},
        {&d_sub_nblk_, nullptr, 0, (size_t)total_subs_ * sizeof(uint32_t) + 256},
        {&d_sub_first_, nullptr, 0, (size_t)total_subs_ * sizeof(uint32_t) + 256},
        {&d_sub_entry_, nullptr, 0, (size_t)total_subs_ * sizeof(uint32_t) + 256},
        {&d_sub_dcsum_, nullptr, 0, (size_t)total_subs_ * 16 + 256},
        {&d_sub_dcentry_, nullptr, 0, (size_t)total_subs_ * 16 + 256},
        {&d_sub_changed_, nullptr, 0, kSubseqCtlWords * sizeof(uint32_t)},
        {&d_dispose_, dispose_jobs_.data(), dispose_jobs_.size() * sizeof(DisposeJob), 0},
        {&d_sub_same_, nullptr, 0, (size_t)total_subs_ * sizeof(uint32_t) + 256},
        {&d_sub_perm_, nullptr, 0, (size_t)total_subs_ * sizeof(uint32_t) + 256},
        {&d_lut_pool_, nullptr, 0, huff_pool_.size() * kLutPoolBytesPerTable},
        {&d_chunk_sums_, nullptr, 0, (size_t)p.total_chunks * sizeof(ChunkSum) + 256},
        {&d_k1_tickets_, nullptr, 0, 256},  // [0] the ticket counter, [1] the device's give-up word
        {&d_k2_tickets_, nullptr, 0, 256},  // K2's pooled runs: a ticket counter each (cleared per upload, never between decodes)
        {&d_sr_set_scan_, p.sr_set_scan.data(), p.sr_set_scan.size() * sizeof(uint32_t), 16},
        {&d_sr_luts_, nullptr, 0, p.sr_set_scan.size() * kSrLutSetBytes + 16},
        {&d_idct_work_, p.idct_work.data(), p.idct_work.size() * sizeof(IdctWork), 0},
        {&d_idct_work_halves_, p.idct_work_halves.data(), p.idct_work_halves.size() * sizeof(IdctWork), 0},
        {&d_ends_, nullptr, 0, (size_t)total_ends_ * sizeof(uint32_t) + 256},
        {&d_ends_u_, nullptr, 0, (size_t)total_ends_ * sizeof(uint32_t) + 256},
        {&d_unstuffed_, nullptr, 0, (size_t)input_bytes_},
        {&d_split_ids_, split_scans_.data(), split_scans_.size() * sizeof(uint32_t), 16},
        // + one tile of slack (IDCT DMA reads whole tiles) + the split scans' flag words
        {&d_coefs_, nullptr, 0, entropy_only_ ? 256 : (size_t)coef_store_blocks_ * 128 + (size_t)kIdctBlocksPerWg * 128 + (size_t)p.flag_words * 8 + 256},
        {&d_out_, nullptr, 0, entropy_only_ ? 256 : (size_t)out_bytes_ + 256},
        {&d_rgb_scratch_, nullptr, 0, rgb_convert_.empty() && color_convert_.empty() && orient_convert_.empty() && fancy_convert_.empty() && luma_convert_.empty() ? 0 : (size_t)out_bytes_ + 256},
        {&d_color_images_, color_images_.data(), color_images_.size() * sizeof(ColorImage), 0},
        {&d_orient_images_, orient_images_.data(), orient_images_.size() * sizeof(OrientImage), 0},
        {&d_fancy_images_, fancy_images_.data(), fancy_images_.size() * sizeof(FancyImage), 0},
        {&d_luma_images_, luma_images_.data(), luma_images_.size() * sizeof(LumaImage), 0},
        {&d_luma_work_, luma_work_.data(), luma_work_.size() * sizeof(LumaWork), 0},
        {&d_islow_work_, islow_work_.data(), islow_work_.size() * sizeof(IslowWork), 0},
        {&d_reduced_work_, reduced_work_.data(), reduced_work_.size() * sizeof(ReducedWork), 0},
        {&d_planes_, nullptr, 0, format_ == JPGPU_FMT_EXTENDED_U16 && !entropy_only_ ? (size_t)planes_bytes_ + 256 : 0},
        {&d_input_, nullptr, 0, (size_t)input_bytes_},
    };
    bool copying = false;
    if ((e = reserve_and_copy(ups, up, &copying)) != hipSuccess) return hip_fail(e, copying ? "hipMemcpyAsync(descriptors)" : "hipMalloc");
    // the flag region starts from zero: the zero bytes in front of every scan's words stay so (K2 writes flag words only)
    // (not in the replay of failed progressive frames: it decodes no split scan, and the words of the images it leaves alone are K2's)
    uint8_t *const flags = (uint8_t *)d_coefs_.ptr + ((size_t)coef_store_blocks_ + (size_t)kIdctBlocksPerWg) * 128;
    if (!split_scans_.empty() && !in_replay_ && (e = hipMemsetAsync(flags, 0, (size_t)p.flag_words * 8, up)) != hipSuccess) return hip_fail(e, "hipMemsetAsync(hand-off flags)");
    if ((e = hipMemsetAsync(d_k2_tickets_.ptr, 0, kK2MaxPools * sizeof(uint32_t), up)) != hipSuccess) return hip_fail(e, "hipMemsetAsync(K2 tickets)");
    // K1 in one pass: descriptors cleared when (re)allocated only (their tags are never reused), tickets + the give-up word per upload
    const size_t want = (size_t)p.total_chunks * kMarkerDescBytes + 256;
    if (want > d_k1_desc_.cap) {
        if ((e = d_k1_desc_.reserve(want)) != hipSuccess) return hip_fail(e, "hipMalloc(K1 descriptors)");
        if ((e = hipMemsetAsync(d_k1_desc_.ptr, 0, d_k1_desc_.cap, up)) != hipSuccess) return hip_fail(e, "hipMemsetAsync(K1 descriptors)");
    }
    if ((e = hipMemsetAsync(d_k1_tickets_.ptr, 0, 2 * sizeof(uint32_t), up)) != hipSuccess) return hip_fail(e, "hipMemsetAsync(K1 tickets)");
    if (!h_k1_giveup_ && (e = hipHostMalloc((void **)&h_k1_giveup_, 64, hipHostMallocMapped)) != hipSuccess) return hip_fail(e, "hipHostMalloc(K1 give-up word)");
    *h_k1_giveup_ = 0;
    k1_epoch_ = 0;
    k1_onepass_ = !p.sw.k1_three_pass;
    // (word kSubseqCtlSameDone: no twins found for this upload yet)
    if ((e = hipMemsetAsync(d_sub_changed_.ptr, 0, kSubseqCtlWords * sizeof(uint32_t), up)) != hipSuccess) return hip_fail(e, "hipMemsetAsync(K2S control)");
    if ((e = launch_lut_pool(up, (const DevHuffTable *)d_huff_pool_.ptr, (int)huff_pool_.size(), (uint8_t *)d_lut_pool_.ptr)) != hipSuccess) return hip_fail(e, "lut_pool_kernel");
    if ((e = launch_sr_luts(up, (const DevScan *)d_scans_.ptr, (const uint32_t *)d_sr_set_scan_.ptr, (int)p.sr_set_scan.size(), (const uint8_t *)d_lut_pool_.ptr,
                            (uint8_t *)d_sr_luts_.ptr)) != hipSuccess) return hip_fail(e, "sr_lut_build_kernel");
    if (!p.files_resident) {
        // single scan jobs / frames handed over by the decoder mirror: small, copied as they are
        // slack before the first file and after the last one is read by the kernels' wide loads: keep it defined
        if ((e = hipMemsetAsync(d_input_.ptr, 0, 256, up)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
        for (size_t i = 0; i < images_.size(); i++) {
            const ImagePlan &img = images_[i];
            if (img.status != JPGPU_OK || img.jobs.empty() || !file_ptr[i] || file_len[i] == 0) continue;
            if ((e = hipMemcpyAsync((uint8_t *)d_input_.ptr + img.file_offset, file_ptr[i], file_len[i], hipMemcpyHostToDevice, up)) != hipSuccess) return hip_fail(e, "hipMemcpyAsync(input)");
            const uint64_t tail = img.file_offset + file_len[i];
            const size_t pad = (size_t)(align_up(tail, 256) - tail);
            if (pad && (e = hipMemsetAsync((uint8_t *)d_input_.ptr + tail, 0, pad, up)) != hipSuccess) return hip_fail(e, "hipMemsetAsync(tail)");
        }
        if ((e = hipMemsetAsync((uint8_t *)d_input_.ptr + input_bytes_ - 256, 0, 256, up)) != hipSuccess) return hip_fail(e, "hipMemsetAsync(slack)");
    }
    if ((e = hipStreamSynchronize(up)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize(upload)");  // the caller's buffers may be released after upload returns
    work_in_flight_ = false;  // the upload stream waited for this batch's earlier device work
    return JPGPU_OK;
}

}  // namespace jpgpu
