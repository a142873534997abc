// jpeglibrary_amd/csrc/device_encode.h -- device-resident batch encode (see device_encode.cpp)
#pragma once
#include <string>
#include <vector>

#include "../../include/jpgpu.h"
#include "device_batch.h"
#include "encode_kernels.h"
#include "encode_progressive.h"
#include "optimize_walk.h"  // put_marker, put_length

namespace jpgpu {

void rgb_ycc_factors(int32_t out[8]);

// The marker segments Encode() writes around the Huffman tables (ref: JpegEncoder.cs:261-280), from the lists the caller's Set* and
// AddComponent calls left: SOI, DQT, (DRI,) SOF0 into *pre, SOS into *post.
struct EncSegmentQuant {
    uint8_t identifier;
    const uint16_t *elements;  // 64, zig-zag, each 1..255 (element precision 0)
};
struct EncSegmentComponent {
    uint8_t id, h, v, tq, td, ta;
};
void write_marker_segments(const EncSegmentQuant *quant, int n_quant, const EncSegmentComponent *comp, int n_comp, int width, int height,
                           int restart_interval, std::vector<uint8_t> *pre, std::vector<uint8_t> *post);
// ... and the whole of SOI..SOS: pre, the DHT segment of `dht_body` (per table its Tc/Th byte, 16 counts and symbols), post
void assemble_header(const std::vector<uint8_t> &pre, const std::vector<uint8_t> &dht_body, const std::vector<uint8_t> &post,
                     std::vector<uint8_t> *header);

// SOI .. SOS as libjpeg writes them (include/jpgpu.h 4d): SOI, APP0 "JFIF", one DQT segment per table, SOF0, one DHT segment per standard
// table, (DRI,) SOS.  `im` holds the geometry and the tables; a one-component image names table 0 and the two luminance Huffman tables only.
// `dht`: the bodies of the DHT segments (Tc/Th, counts, values) in place of the standard tables; frame 0xC2: a progressive frame's header, which ends
// behind SOF2 (every scan brings its tables and its SOS).
void write_libjpeg_header(const DevEncImage &im, int restart_interval, std::vector<uint8_t> *header, const std::vector<std::vector<uint8_t>> *dht = nullptr,
                          int frame = 0xC0);
// ... and where the 64 elements of quantisation table `identifier` stand in it (0: the header holds no such table)
size_t libjpeg_header_quant_at(const DevEncImage &im, int identifier);

// The stuffing stage's (E4, launch_stuff) layout, for the encoder's images and the optimizer's DRI = 0 scans (descriptors in the
// encoder's image form): from raw_bits[k] and the image's header_len, restart_interval and n_units, where its raw bytes lie
// (raw_off; left alone unless place_raw: the one-pass emit has placed them already), where its finished stream goes (out_off: the
// header, then the worst case of the stuffing) and its chunks of kEncStuffChunk raw bytes (chunk_off, at least one per stream).
struct StuffPlan {
    std::vector<EncWork> work_chunk;
    uint64_t raw_bytes = 0, out_bytes = 0;  // what the raw and the output buffer hold, every stream 256-byte aligned
    uint32_t chunks = 0;
};
StuffPlan plan_stuffing_layout(DevEncImage *images, const uint64_t *raw_bits, int n, bool place_raw);

// E2 -> E3 -> E4 as kernels of their own (block_bits_kernel, emit_kernel, the stuff kernels) over coefficients that lie on the device: the
// buffers the three hand one another, and one method per step.  What the kernels read beside them is the caller's (a Source); so are the
// events and the host round trips between the steps.  A step that fails returns HIP's error and leaves the name of the call in `failed`.
struct EntropyTail {
    struct Source {
        const DevEncImage *images;  // on the device
        const EncWork *work_blk;    // one entry per 256 units of an image
        int n_work_blk;
        const EncHuffTable *tables;
        const int16_t *coefs;
        const DevEncLayout *layouts;
        bool any_plain;
    };
    DevBuffer bits, bit_off, raw_bits, raw, marks, chunk_ff, work_chunk, out, out_len;  // (bit_off: per workgroup its base (u64) | its bits (u32))
    std::vector<uint64_t> h_raw_bits, h_out_len;  // per image: what E2 counted, how long the finished stream is
    StuffPlan stuff;
    uint64_t emit_words = 0;  // emit_kernel's LDS buffer, in words
    const char *failed = "";
    hipError_t reserve(uint64_t total_blocks, size_t n_work_blk, size_t n_images);  // what does not depend on the data
    hipError_t count_bits(hipStream_t stream, const Source &s, int n_images);
    hipError_t read_bit_counts(hipStream_t stream, int n_images);  // -> h_raw_bits, the stream synchronised
    // E3's LDS words, the stuffing stage's layout (into images[]; place_raw false: the raw streams are placed and written already), room for it
    hipError_t plan(hipStream_t stream, DevEncImage *images, int n_images, bool place_raw);
    hipError_t upload_chunk_work(hipStream_t stream);
    hipError_t emit(hipStream_t stream, const Source &s);
    hipError_t stuff_bytes(hipStream_t stream, const DevEncImage *images);
    hipError_t read_lengths(hipStream_t stream, int n_images);  // -> h_out_len, the stream synchronised
    void release();
};

// A jpgpu_encode_description resolved on the host (no device needed): the reference's checks, the marker segments, the by-symbol
// Huffman tables and the block map of the general kernels -- or the jpgpu_encode_params of the EncodeAction arrangement it is.
struct EncPlan {
    int status = JPGPU_OK;  // JPGPU_OK, or what Encode() of this image reports (the refused arrangement, an empty builder)
    std::string message;
    bool legacy = false;    // an EncodeAction arrangement: today's entry point takes it
    jpgpu_encode_params params = {};
    bool legacy_has_quant = false;  // SetQuantizationTable with the caller's tables 0 and 1 (legacy_quant)
    uint16_t legacy_quant[2][64] = {};
    int width = 0, height = 0, in_components = 0, input_rgb = 0, restart_interval = 0;  // of a described arrangement
    bool any_builder = false;
    int most_optimal = 0;
    int n_slots = 0;
    struct Slot {
        bool given = false;
        uint8_t tc_th = 0;         // the DHT's Tc/Th byte
        EncHuffTable table;        // given: GetCode for all 256 symbols
        std::vector<uint8_t> dht;  // given: 16 counts + symbols, as TryWrite writes them
    };
    std::vector<Slot> slots;    // n_slots of them (none for an EncodeAction arrangement handed over as its parameters)
    std::vector<uint8_t> header_pre, header_post;  // SOI, DQT, (DRI,) SOF0 | SOS
    std::vector<uint8_t> header;                   // without builders: SOI .. SOS
    std::vector<DevEncLayout> layout;  // one (none for an EncodeAction arrangement handed over as its parameters)
    uint32_t bpm = 0;
};
// returns JPGPU_OK (plan->status may still refuse the image) or the argument error of the call, with its message in *error
int resolve_encode_description(const jpgpu_encode_description &d, EncPlan *plan, std::string *error);

class EncodeBatch {
  public:
    explicit EncodeBatch(jpgpu_ctx *ctx) : ctx_(ctx) {}
    ~EncodeBatch();
    int upload(const uint8_t *const *pixels, const jpgpu_encode_params *params, int n);  // SetInputReader x n (+ H2D)
    int upload_described(const uint8_t *const *pixels, const jpgpu_encode_description *desc, int n);
    // the same from pixels that are in device memory already (jpgpu_encoder_upload_device): nothing is copied, E1 reads the caller's
    // memory; pixel_layouts[i] = JPGPU_PIXELS_INTERLEAVED / JPGPU_PIXELS_PLANAR (null: all interleaved)
    int upload_device(const void *const *device_pixels, const jpgpu_encode_params *params, const int32_t *pixel_layouts, int n);
    int upload_described_device(const void *const *device_pixels, const jpgpu_encode_description *desc, const int32_t *pixel_layouts, int n);
    int set_quantization_table(int i, int identifier, const uint16_t *zigzag64);           // SetQuantizationTable of image i
    // the arithmetic of the uploads from here on (jpgpu_encoder_set_arithmetic_policy), and what image i of the last one was planned with
    int set_arithmetic_policy(int policy);
    int image_arithmetic(int i, int *arithmetic) const;
    // the entropy coding of the uploads from here on (jpgpu_encoder_set_coding_policy), and what image i of the last one was planned with
    int set_coding_policy(int policy);
    int image_coding(int i, int *coding) const;
    int encode();                                                                        // JpegEncoder.Encode() x n
    // device time of the last encode() by stage (HIP events on the context's stream): E1 pixels -> quantised blocks, E2 bit counts
    // and offsets, E3 bit emission, E4 byte stuffing; ms[4] = the four together (the host round trips between them excluded)
    int stage_ms(float ms[5]);
    int size() const { return (int)images_.size(); }
    int encoded_size(int i, size_t *bytes) const;
    int image_status(int i) const { return (i >= 0 && i < (int)status_.size()) ? status_[i] : JPGPU_ERR_ARGUMENT; }
    int download(int i, void *dst, size_t cap);
    int download_coefficients(int i, int16_t *dst, size_t cap_blocks);
    uint32_t total_blocks(int i) const { return (i >= 0 && i < (int)images_.size()) ? images_[i].total_blocks : 0; }
    void *output_device(int i, size_t *bytes) const {
        if (i < 0 || i >= (int)images_.size() || !encoded_) return nullptr;
        if (bytes) *bytes = (size_t)tail_.h_out_len[i];
        return stream_of(i);
    }

  private:
    int fail(int status, const std::string &msg);
    int hip_fail(hipError_t e, const char *what);
    // device = pixels[] are device addresses laid out as pixel_layouts[] says (null: interleaved); else host memory to copy
    int upload_params(const uint8_t *const *pixels, const jpgpu_encode_params *params, int n, bool device, const int32_t *pixel_layouts);
    int upload_descriptions(const uint8_t *const *pixels, const jpgpu_encode_description *desc, int n, bool device, const int32_t *pixel_layouts);
    int upload_plans(const uint8_t *const *pixels, const std::vector<EncPlan> &plans, bool device, const int32_t *pixel_layouts);
    // layout_plans is the list of these; what they hand one another is an UploadPlan that lives for the call
    struct UploadPlan;
    int layout_plans(UploadPlan &up, const std::vector<EncPlan> &plans);
    int check_device_arguments(const UploadPlan &up, int n);
    int check_libjpeg_params(const jpgpu_encode_params *params, int n);
    int check_coding_params(const jpgpu_encode_params *params, int n);
    void reset_upload_state(int n);
    int plan_described_image(UploadPlan &up, int i, const EncPlan &pl);
    int plan_encode_action_image(UploadPlan &up, int i, const EncPlan &pl);
    int place_pixels(const UploadPlan &up, int i, int input_rgb);
    void plan_image_work(UploadPlan &up, int i, bool statistics);
    int check_device_pixels(const uint8_t *const *pixels);
    void place_table_slots(UploadPlan &up);
    int reserve_and_upload(const UploadPlan &up);
    // encode() is the list of these; what they hand one another is an EncodeRun that lives for the call
    struct EncodeRun;
    int upload_image_descriptors();
    int run_fdct(const EncodeRun &r);
    int build_coding_tables(const EncodeRun &r);
    bool build_image_tables(int i, const EncPlan *described, const uint32_t *counters, bool most_optimal, EncHuffTable *tables);
    EntropyTail::Source tail_source(const EncodeRun &r) const;
    int try_one_pass_emit(EncodeRun &r);
    int count_bits_two_kernels(const EncodeRun &r);
    int plan_stuffing(const EncodeRun &r);
    int place_headers(const EncodeRun &r);
    int emit_and_stuff(const EncodeRun &r);
    bool build_libjpeg_tables(int i, const uint32_t *counters, EncHuffTable *tables);
    // the finished stream of image i in device memory
    uint8_t *stream_of(int i) const {
        if (coding_ == JPGPU_CODING_PROGRESSIVE) return (uint8_t *)prog_.out.ptr + prog_.files[(size_t)i].dst_off;
        return (uint8_t *)tail_.out.ptr + images_[(size_t)i].out_off;
    }
    // coding "progressive" (device_encode_progressive.cpp): the scans of every image as units of work, planned at the upload; the entropy
    // coder of encode() behind E1
    struct Progressive {
        std::vector<DevProgScan> scans;
        std::vector<int> scan_image;          // the image a scan belongs to
        std::vector<EncWork> work;            // per 256 blocks of a scan
        std::vector<DevProgFile> files;       // per image
        std::vector<DevEncImage> streams;     // per scan: the stuffing stage's descriptor (its "header": the scan's DHT segments and SOS)
        std::vector<uint8_t> headers;         // every image's frame header, every scan's DHT + SOS
        uint64_t total_blocks = 0;
        int max_scans = 0;
        DevBuffer d_scans, d_work, d_info, d_heads, d_bits, d_wg_bits, d_wg_base, d_stats, d_tables, d_files, d_streams, d_headers, out, d_file_len;
        EntropyTail tail;  // E4 over the scans
        void release();
    };
    Progressive prog_;
    int plan_progressive();
    int encode_progressive();
    jpgpu_ctx *ctx_;
    int coding_policy_ = JPGPU_CODING_STANDARD;  // state of the encoder, read by the uploads like the arithmetic policy
    int coding_ = JPGPU_CODING_STANDARD;         // ... and what the last upload was planned with
    int arithmetic_policy_ = JPGPU_ARITHMETIC_REFERENCE;  // state of the encoder: jpgpu_encoder_upload and _upload_device read it
    std::vector<DevEncImage> images_;
    std::vector<std::vector<uint8_t>> headers_;        // SOI .. SOS as Encode() writes them (optimizeCoding: rebuilt per encode())
    std::vector<std::vector<uint8_t>> headers_pre_;    // optimizeCoding: SOI, DQT, SOF0 ...
    std::vector<std::vector<uint8_t>> headers_post_;   // ... and SOS; the DHT between them depends on the statistics
    std::vector<int> optimized_;                       // images with optimizeCoding
    std::vector<uint8_t> most_optimal_;                // ... and MostOptimalCoding (package merge)
    std::vector<int> status_;                          // per image: JPGPU_OK or the reference's failure ("No symbol is recorded.")
    std::vector<std::string> messages_;                // ... and its message
    std::vector<int> general_;                         // described images that are no EncodeAction arrangement (DevEncImage.layout = k + 1)
    std::vector<EncPlan> general_plans_;               // ... their resolved descriptions
    std::vector<DevEncLayout> layouts_;
    DevBuffer d_layouts_;
    bool any_general_builder_ = false;
    bool upload_described_ = false;                    // the last upload was jpgpu_encoder_upload_described
    bool pixels_on_device_ = false;                    // the last upload was a device upload: DevEncImage.px_off is an address, d_pixels_ is not in use
    DevBuffer d_hist_;
    bool encoded_ = false;
    hipEvent_t ev_[6] = {};
    uint64_t total_blocks_ = 0;
    int n_work_mcu_ = 0, n_work_blk_ = 0, n_work_stat_ = 0;
    DevBuffer d_samples_;  // E1a -> E1b: gathered samples, enc_sample_bytes_per_mcu per MCU
    DevBuffer d_pixels_, d_images_, d_tables_, d_work_mcu_, d_work_blk_, d_work_stat_, d_coefs_, d_headers_;
    EntropyTail tail_;  // E2 .. E4 behind them
    std::vector<uint8_t> header_bytes_;  // every image's SOI..SOS, concatenated (one upload per encode)
    // E2 + E3 as one pass (bits_emit_kernel): restart-free uploads only; the LDS stretch buffer is sized from the previous encode()
    // of this upload (0: not known yet; 0xFFFFFFFF: a stretch did not fit or a wait ran out -- the two-kernel path from then on)
    DevBuffer d_chain_, d_work_order_;
    bool any_restart_ = false;
    uint32_t emit_hint_ = 0;
    int one_pass_emits_ = 0, fused_emit_fallbacks_ = 0;  // encode() calls that issued bits_emit_kernel / of those, the ones that had to issue the two kernels after it

  public:
    void emit_counters(int *one_pass, int *fell_back) const {
        if (one_pass) *one_pass = one_pass_emits_;
        if (fell_back) *fell_back = fused_emit_fallbacks_;
    }
};

}  // namespace jpgpu
