// jpeglibrary_amd/csrc/device_optimize.h -- device-resident batch of JpegOptimizer runs (see device_optimize.cpp)
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../include/jpgpu.h"
#include "device_batch.h"
#include "device_encode.h"
#include "encode_kernels.h"
#include "kx_lossless.h"
#include "optimize_walk.h"
#include "transform_plan.h"

namespace jpgpu {

// JpegHuffmanEncodingTableBuilder.Build(false) (ref: JpegHuffmanEncodingTableBuilder.cs:68-175, 237-283): canonical
// codes in DHT order from the 256 symbol counts.  false = "No symbol is recorded." / a code size beyond the
// reference's 60-entry array.
struct OptimalCode {
    uint16_t code;
    uint8_t symbol, length;
};
// perm[i] = original index of the key the restated Array.Sort(T[], Comparison<T>) leaves at position i (ascending by key)
void net_sort_permutation(const int32_t *keys, int n, int32_t *perm);
bool build_optimal_table(const uint32_t freq[256], std::vector<OptimalCode> *codes, bool most_optimal = false);  // Build(optimal)
// The JpegHuffmanEncodingTable of those codes, both ways it is read: GetCode for all 256 symbols into *table -- a symbol without a
// code gets the table's first code, _symbolMap being 0 for it (ref: JpegHuffmanEncodingTable.cs:21-37, 94-100) -- and TryWrite's
// bytes (:50-86: the 16 counts, then the symbols) appended to *dht.  The Tc/Th byte in front of them is the caller's.
void optimal_codes_to_table(const std::vector<OptimalCode> &codes, EncHuffTable *table, std::vector<uint8_t> *dht);

class OptimizeBatch {
  public:
    explicit OptimizeBatch(jpgpu_ctx *ctx) : ctx_(ctx), batch_(ctx) {}
    ~OptimizeBatch();
    // SetInput x n: host marker walks (Scan()'s and Optimize()'s) + H2D of the files
    int upload(const uint8_t *const *jpeg, const size_t *len, int n, int strip);
    // Scan() + Optimize(strip) x n: statistics, tables, transcode
    int run();
    int size() const { return (int)plans_.size(); }
    int result(int i, jpgpu_image_result *res, size_t *out_len);
    int download(int i, void *dst, size_t cap);
    // the statistics Scan() collected for table `t` of image i (builder-creation order); false past the last table
    bool statistics(int i, int t, uint8_t *table_class, uint8_t *identifier, uint32_t counts[256]) const;
    float last_ms() const { return last_ms_; }
    void set_most_optimal_coding(bool on) { most_optimal_ = on; }  // JpegOptimizer.MostOptimalCoding
    // The lossless transform: the policy and the edge policy are state of the optimizer, the list is consumed by the next upload
    int set_orientation_policy(int policy);
    int set_orientations(const uint8_t *orientations, int n);
    int set_edge_policy(int edge);
    int image_transform(int i, jpgpu_transform_info *info) const;
    // ... and its window ("Window" of the same section): the origin policy is state, the list is consumed by the next upload
    int set_origin_policy(int origin);
    int set_windows(const jpgpu_rect *windows, int n);
    int image_window(int i, jpgpu_rect *applied) const;
    int turn_sources() const { return road_.sources; }  // files the coefficient road of the last upload entropy-decoded
    // of the last run (zeros: nothing was turned), HIP events all three: KX alone; the entropy decode in front of it; the dense copy
    void last_turn_ms(float ms[3]) const {
        for (int k = 0; k < 3; k++) ms[k] = road_.ms[k];
    }

  private:
    struct Plan : WalkPlan {  // (optimize_walk.h: what the host walks leave; below, what the device passes add)
        bool build_failed = false;  // BuildTables threw (it runs at the end of the scan: in front of anything a later marker throws)
        int job = -1;  // scan job inside batch_
        std::string dht;  // the rewritten DHT segment (marker, length, tables)
        uint64_t entropy_off = 0, entropy_len = 0;
        bool by_subsequence = false;  // DRI = 0 scan: transcoded by subsequence (KTS), bytes in d_sout_
        uint64_t out_len = 0;
        // the lossless transform: the image's plan (orientation 1 and no window: the image takes the road above and nothing below is read), and
        // its place among the images of the upload that take the coefficient road (-1: not among them, or refused)
        TransformPlan transform;
        int turn = -1;
    };
    // The coefficient road (the lossless transform): the turned files once more, as the decoder takes them (its entropy stage fills the dense store KX
    // reads), KX, statistics and tables, the encoder's entropy stages.  Made by the first upload that turns something, released by the next that turns nothing.
    struct RoadPlans {                          // (of one upload)
        int sources = 0;                        // files `batch` entropy-decodes
        std::vector<DevTurnImage> turn_images;  // per turned image: its KX descriptor,
        std::vector<TurnWork> turn_work;
        std::vector<DevEncImage> images;        // ... and what the encoder's general kernels need of it
        std::vector<DevEncLayout> layouts;
        std::vector<EncWork> work_blk, work_stat;
        uint64_t blocks_total = 0;
    };
    struct Road : RoadPlans {
        std::unique_ptr<DeviceBatch> batch;
        float ms[3] = {};  // of the last run: KX, the entropy decode in front of it, the dense copy
        hipEvent_t ev_kx[2] = {}, ev_td[3] = {};
        DevBuffer d_turn_images, d_turn_work, d_coefs, d_images, d_layouts, d_work_blk, d_work_stat, d_hist, d_tables;
        EntropyTail tail;
        void release();  // nothing stays on the device
    };
    int fail(int status, const std::string &msg);
    int hip_fail(hipError_t e, const char *what);
    // upload() is the list of these; what they hand one another is an Upload that lives for the call
    struct Upload;
    int take_pending_lists(Upload &u);
    void plan_on_host(const Upload &u);
    int hand_files_to_decoder(const Upload &u);
    void admit_and_sort(Upload &u);
    int plan_road(const Upload &u);
    bool plan_road_image(Plan &p, const ImagePlan *img);
    int reserve_and_upload();
    // run() is the list of these; what they hand one another is a Run that lives for the call
    struct Run;
    int count_symbols(Run &r);
    int build_tables(Run &r);
    int measure_and_place(Run &r);
    int emit_intervals(Run &r);
    int emit_subsequences_and_stuff(Run &r);
    void collect_lengths(const Run &r);
    // ... and of the turned images: entropy decode into the dense store, KX, statistics and tables, the encoder's entropy stages
    int decode_turned(Run &r);
    int turn_blocks(Run &r);
    int build_turned_tables(Run &r);
    int emit_turned(Run &r);
    // BuildTables of one image: `hist` and `enc` are the rows of the job's n_huff tables
    void build_image_tables(Plan &p, const uint32_t *hist, EncHuffTable *enc) const;
    void plan_turned_image(Plan &p, const uint8_t *data, size_t len, bool strip, int given, const jpgpu_rect *window);
    jpgpu_ctx *ctx_;
    DeviceBatch batch_;
    Road road_;
    int orient_policy_ = JPGPU_ORIENT_STORED, edge_policy_ = JPGPU_EDGE_REFUSE;
    std::vector<uint8_t> pending_orientations_;  // of the next upload (empty: none)
    int origin_policy_ = JPGPU_ORIGIN_REFUSE;
    std::vector<jpgpu_rect> pending_windows_;
    int n_work_emit_ = 0, n_sub_work_emit_ = 0;  // entries of work_ / sub_work_ in front of the turned images' (which are only counted)
    std::vector<Plan> plans_;
    std::vector<uint32_t> scan_ids_;   // jobs that are transcoded, one lane per restart interval ...
    std::vector<HuffWork> work_;
    std::vector<uint32_t> sub_scan_ids_;  // ... and the DRI = 0 jobs transcoded by subsequence
    std::vector<HuffWork> sub_work_;
    std::vector<uint32_t> h_hist_;     // [jobs][8][256]
    bool ran_ = false;
    bool most_optimal_ = false;
    float last_ms_ = 0;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    DevBuffer d_work_, d_scan_ids_, d_hist_, d_enc_, d_sizes_, d_offsets_, d_base_, d_totals_, d_out_;
    // subsequence path: bit counts / offsets per subsequence, raw (unstuffed) bits, the encoder's stuffing stage
    DevBuffer d_sub_work_, d_sub_scan_ids_, d_sub_bits_, d_sub_bitoff_, d_sub_totals_, d_scan_raw_off_, d_raw_, d_simages_, d_swork_chunk_,
        d_chunk_ff_, d_sout_, d_sout_len_;
};

}  // namespace jpgpu
