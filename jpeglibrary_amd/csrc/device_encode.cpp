// jpeglibrary_amd/csrc/device_encode.cpp -- device-resident batch ENCODE: what JpegEncoder.Encode() does for a set of images
// (ref: JpegEncoder.cs:255-291 with the call sequence of apps/JpegEncode/EncodeAction.cs:38-63, optimizeCoding = false).
// The host writes the marker segments (SOI, DQT, SOF0, DHT, SOS -- the reference's JpegWriter calls, byte for byte);
// the per-block arithmetic and the entropy coding run in encode_kernels.hip.
#include "device_encode.h"
#include "device_optimize.h"
#include "libjpeg_huffman.h"

#include <string.h>

#include <algorithm>

namespace jpgpu {

// JPGPU_ENC_NO_FUSED (measurement): E1 as its two kernels for every image
static bool enc_fused_enabled() {
    static const bool on = getenv("JPGPU_ENC_NO_FUSED") == nullptr;
    return on;
}
// JPGPU_ENC_TWO_PASS_EMIT (measurement): E2 and E3 as their two kernels for every upload (bits_emit_kernel never used)
static bool enc_fused_emit_enabled() {
    static const bool on = getenv("JPGPU_ENC_TWO_PASS_EMIT") == nullptr;
    return on;
}


namespace {
uint64_t align_up64(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// ref: JpegStandardQuantizationTable.cs:12-34 (zig-zag order)
const uint16_t kStdLum[64] = {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49,
                              35, 37, 29, 40, 58, 51, 61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56,
                              80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99};
const uint16_t kStdChr[64] = {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// ref: JpegStandardHuffmanEncodingTable.cs:14-83
const uint8_t kDcLumLen[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChrLen[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVal[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumLen[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
const uint8_t kAcLumVal[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChrLen[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
const uint8_t kAcChrVal[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct StdTable {
    const uint8_t *lengths, *values;
    int count;
};
const StdTable kStd[4] = {{kDcLumLen, kDcVal, 12}, {kAcLumLen, kAcLumVal, 162}, {kDcChrLen, kDcVal, 12}, {kAcChrLen, kAcChrVal, 162}};

// ref: JpegStandardHuffmanEncodingTable.BuildCanonicalCode (:85-131) + JpegHuffmanEncodingTable.GetCode (:94-100)
void build_enc_table(const StdTable &s, EncHuffTable *t) {
    memset(t, 0, sizeof *t);
    uint8_t remaining[16], len_of[256];
    memcpy(remaining, s.lengths, 16);
    int pos = 0, current = 1;
    for (int i = 0; i < s.count; i++) {
        while (remaining[pos] == 0) {
            pos++;
            current++;
        }
        remaining[pos]--;
        len_of[i] = (uint8_t)current;
    }
    uint16_t bit_code = 0;
    int bit_count = len_of[0];
    t->code[s.values[0]] = 0;
    t->len[s.values[0]] = len_of[0];
    for (int i = 1; i < s.count; i++) {
        if (len_of[i] > bit_count) {
            bit_code++;
            bit_code = (uint16_t)(bit_code << (len_of[i] - bit_count));
            bit_count = len_of[i];
        } else {
            ++bit_code;
        }
        t->code[s.values[i]] = bit_code;
        t->len[s.values[i]] = len_of[i];
    }
}

// ref: JpegStandardQuantizationTable.ScaleByQuality (:64-87)
void scale_by_quality(const uint16_t *src, int quality, uint16_t *dst) {
    const int scale = quality < 50 ? 5000 / quality : 200 - (quality * 2);
    for (int i = 0; i < 64; i++) {
        int x = src[i];
        x = ((x * scale) + 50) / 100;
        dst[i] = (uint16_t)std::min(std::max(x, 1), 255);
    }
}
}  // namespace

// Fix() factors of apps/JpegEncode/JpegRgbToYCbCrConverter.cs:38-56 (float32 arithmetic like the reference's Fix, :59-62)
void rgb_ycc_factors(int32_t out[8]) {
    auto fix = [](float x) { return (int32_t)((x * (float)(1L << 16)) + 0.5F); };
    out[0] = fix(0.299F);
    out[1] = fix(0.587F);
    out[2] = fix(0.114F);
    out[3] = fix(0.168735892F);
    out[4] = fix(0.331264108F);
    out[5] = fix(0.5F);
    out[6] = fix(0.418687589F);
    out[7] = fix(0.081312411F);
}

// ------------------------------------------------------------------------------------------------ marker segments

// EncodeBatch::set_quantization_table patches the DQT this writes, in place, at 2 + 2 + 2 + identifier * 65 + 1: nothing but SOI in
// front of the segment, ONE segment, and per table one identifier byte + 64 one-byte elements in list order.  Keep that true.
void write_marker_segments(const EncSegmentQuant *quant, int n_quant, const EncSegmentComponent *comp, int n_comp, int width, int height,
                           int restart_interval, std::vector<uint8_t> *pre, std::vector<uint8_t> *post) {
    std::vector<uint8_t> &h = *pre;
    h.clear();
    put_marker(h, 0xD8);
    put_marker(h, 0xDB);  // WriteQuantizationTables (:305-330): ONE segment, every table of the list in SetQuantizationTable order, used or not
    put_length(h, (uint16_t)(65 * n_quant));
    for (int t = 0; t < n_quant; t++) {
        h.push_back(quant[t].identifier);  // JpegQuantizationTable.TryWrite: precision 0 << 4 | identifier
        for (int i = 0; i < 64; i++) h.push_back((uint8_t)quant[t].elements[i]);
    }
    if (restart_interval) {  // DRI in front of SOF0: the reference's decoder latches it there even without Identify()
        put_marker(h, 0xDD);
        put_length(h, 2);
        h.push_back((uint8_t)(restart_interval >> 8));
        h.push_back((uint8_t)restart_interval);
    }
    put_marker(h, 0xC0);  // WriteStartOfFrame (:353-381)
    put_length(h, (uint16_t)(6 + 3 * n_comp));
    h.push_back(8);
    h.push_back((uint8_t)(height >> 8));
    h.push_back((uint8_t)height);
    h.push_back((uint8_t)(width >> 8));
    h.push_back((uint8_t)width);
    h.push_back((uint8_t)n_comp);
    for (int c = 0; c < n_comp; c++) {
        h.push_back(comp[c].id);
        h.push_back((uint8_t)((comp[c].h << 4) | comp[c].v));
        h.push_back(comp[c].tq);
    }
    std::vector<uint8_t> &sos = *post;
    sos.clear();
    put_marker(sos, 0xDA);  // WriteStartOfScan (:387-408)
    put_length(sos, (uint16_t)(1 + 2 * n_comp + 3));
    sos.push_back((uint8_t)n_comp);
    for (int c = 0; c < n_comp; c++) {
        sos.push_back(comp[c].id);
        sos.push_back((uint8_t)((comp[c].td << 4) | (comp[c].ta & 0xf)));
    }
    sos.push_back(0);
    sos.push_back(63);
    sos.push_back(0);
}

// WriteHuffmanTables (:336-347) between the two: ONE segment, every table of the collection in SetHuffmanTable order
void assemble_header(const std::vector<uint8_t> &pre, const std::vector<uint8_t> &dht_body, const std::vector<uint8_t> &post,
                     std::vector<uint8_t> *header) {
    std::vector<uint8_t> &h = *header;
    h = pre;
    put_marker(h, 0xC4);
    put_length(h, (uint16_t)dht_body.size());
    h.insert(h.end(), dht_body.begin(), dht_body.end());
    h.insert(h.end(), post.begin(), post.end());
}

// ------------------------------------------------------------------------------------------------ libjpeg's header

namespace {
template <typename Body>
void put_segment(std::vector<uint8_t> &h, int marker, const Body &body) {
    put_marker(h, marker);
    put_length(h, (uint16_t)body.size());
    h.insert(h.end(), body.begin(), body.end());
}
}  // namespace

// jcmarker.c: write_file_header (SOI, APP0), write_frame_header (a DQT segment per table in use, SOF0), write_scan_header (a DHT
// segment per table in use: DC then AC of each component's pair; DRI; SOS)
void write_libjpeg_header(const DevEncImage &im, int restart_interval, std::vector<uint8_t> *header, const std::vector<std::vector<uint8_t>> *dht, int frame) {
    std::vector<uint8_t> &h = *header;
    h.clear();
    const int nc = (int)im.components;
    put_marker(h, 0xD8);
    put_segment(h, 0xE0, std::vector<uint8_t>{'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});  // version 1.01, no units, density 1 x 1, no thumbnail
    for (int t = 0; t < (nc == 3 ? 2 : 1); t++) {
        std::vector<uint8_t> body(1, (uint8_t)t);
        for (int i = 0; i < 64; i++) body.push_back((uint8_t)im.quant[t][i]);
        put_segment(h, 0xDB, body);
    }
    std::vector<uint8_t> sof = {8, (uint8_t)(im.height >> 8), (uint8_t)im.height, (uint8_t)(im.width >> 8), (uint8_t)im.width, (uint8_t)nc};
    for (int c = 0; c < nc; c++) {
        sof.push_back((uint8_t)(c + 1));
        sof.push_back(c == 0 ? (uint8_t)((im.luma_h << 4) | im.luma_v) : (uint8_t)0x11);
        sof.push_back(c == 0 ? 0 : 1);
    }
    put_segment(h, frame, sof);
    if (frame == 0xC2) return;  // a progressive frame: every scan brings its tables and its SOS
    for (int t = 0; t < (nc == 3 ? 4 : 2); t++) {  // DC0, AC0, DC1, AC1
        if (dht) {
            put_segment(h, 0xC4, (*dht)[(size_t)t]);
            continue;
        }
        std::vector<uint8_t> body(1, (uint8_t)(((t & 1) << 4) | (t >> 1)));
        body.insert(body.end(), kStd[t].lengths, kStd[t].lengths + 16);
        body.insert(body.end(), kStd[t].values, kStd[t].values + kStd[t].count);
        put_segment(h, 0xC4, body);
    }
    if (restart_interval) put_segment(h, 0xDD, std::vector<uint8_t>{(uint8_t)(restart_interval >> 8), (uint8_t)restart_interval});
    std::vector<uint8_t> sos(1, (uint8_t)nc);
    for (int c = 0; c < nc; c++) {
        sos.push_back((uint8_t)(c + 1));
        sos.push_back(c == 0 ? 0x00 : 0x11);
    }
    sos.insert(sos.end(), {0, 63, 0});
    put_segment(h, 0xDA, sos);
}

size_t libjpeg_header_quant_at(const DevEncImage &im, int identifier) {
    if (identifier != 0 && im.components != 3) return 0;
    return 2 + 18 + (size_t)identifier * 69 + 5;  // SOI, APP0, the DQT segments in front (marker, length, identifier, 64 elements each)
}

// ------------------------------------------------------------------------------------------------ stuffing stage layout

StuffPlan plan_stuffing_layout(DevEncImage *images, const uint64_t *raw_bits, int n, bool place_raw) {
    StuffPlan sp;
    for (int i = 0; i < n; i++) {
        DevEncImage &im = images[i];
        const uint64_t raw_len = (raw_bits[i] + 7) / 8;
        if (place_raw) im.raw_off = sp.raw_bytes;
        im.out_off = sp.out_bytes;
        im.chunk_off = sp.chunks;
        const uint32_t chunks = std::max<uint32_t>(1u, (uint32_t)((raw_len + kEncStuffChunk - 1) / kEncStuffChunk));
        for (uint32_t c = 0; c < chunks; c++) sp.work_chunk.push_back({(uint32_t)i, c});
        sp.chunks += chunks;
        sp.raw_bytes = align_up64(sp.raw_bytes + raw_len + 64, 256);
        // every byte may need stuffing; two marker bytes per restart interval
        sp.out_bytes = align_up64(sp.out_bytes + im.header_len + 2 * raw_len + 2 + 64 + (im.restart_interval ? 2 * (uint64_t)im.n_units : 0), 256);
    }
    return sp;
}

// ------------------------------------------------------------------------------------------------ described images

// ---- EntropyTail: E2 -> E3 -> E4
hipError_t EntropyTail::reserve(uint64_t total_blocks, size_t n_work_blk, size_t n_images) {
    failed = "hipMalloc";
    const size_t slack = 256 + 16;  // (the kernels read past the payload)
    hipError_t e = bits.reserve((size_t)total_blocks * sizeof(uint32_t) + slack);
    if (e == hipSuccess) e = bit_off.reserve(((n_work_blk * sizeof(uint64_t) + 255) & ~(size_t)255) + n_work_blk * sizeof(uint32_t) + 256 + slack);
    if (e == hipSuccess) e = raw_bits.reserve(n_images * sizeof(uint64_t) + slack);
    if (e == hipSuccess) e = out_len.reserve(n_images * sizeof(uint64_t) + slack);
    return e;
}

hipError_t EntropyTail::count_bits(hipStream_t stream, const Source &s, int n_images) {
    failed = "block_bits_kernel";
    uint32_t *wg_bits = reinterpret_cast<uint32_t *>((uint8_t *)bit_off.ptr + (((size_t)s.n_work_blk * sizeof(uint64_t) + 255) & ~(size_t)255));
    return launch_block_bits(stream, s.images, s.work_blk, s.n_work_blk, s.tables, s.coefs, (uint32_t *)bits.ptr, n_images, wg_bits, (uint64_t *)bit_off.ptr,
                             (uint64_t *)raw_bits.ptr, s.layouts, s.any_plain);
}

// one host round trip: a count per image, the stream synchronised (what fed its async copies may leave scope)
static hipError_t read_counts(hipStream_t stream, const DevBuffer &from, int n_images, std::vector<uint64_t> *to) {
    to->assign((size_t)n_images, 0);
    const hipError_t e = hipMemcpyAsync(to->data(), from.ptr, (size_t)n_images * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}
hipError_t EntropyTail::read_bit_counts(hipStream_t stream, int n_images) {
    failed = "hipMemcpy(bit counts)";
    return read_counts(stream, raw_bits, n_images, &h_raw_bits);
}
hipError_t EntropyTail::read_lengths(hipStream_t stream, int n_images) {
    failed = "hipMemcpy(stream lengths)";
    return read_counts(stream, out_len, n_images, &h_out_len);
}

hipError_t EntropyTail::plan(hipStream_t stream, DevEncImage *images, int n_images, bool place_raw) {
    // E3's LDS buffer: twice the largest average stretch a workgroup (256 blocks or restart intervals) of any image writes,
    // in steps of 4 KB -- the smaller it is the more workgroups share a CU; a workgroup whose stretch does not fit falls back
    // to atomics in HBM (launch_emit clamps to 8-32 KB).  Images whose AVERAGE stretch is beyond 32 KB (restart intervals of
    // several MCUs: every lane then writes a stretch of its own and the atomics do not collide) do not count; a batch of
    // nothing else asks for no LDS at all.
    emit_words = 0;
    for (int i = 0; i < n_images; i++) {
        const uint64_t wgs = ((uint64_t)images[i].n_units + 255) / 256;
        const uint64_t avg_words = h_raw_bits[(size_t)i] / 32 / std::max<uint64_t>(wgs, 1) + 1;
        if (avg_words <= kEmitLdsWordsMax) emit_words = std::max<uint64_t>(emit_words, 2 * avg_words);
    }
    stuff = plan_stuffing_layout(images, h_raw_bits.data(), n_images, place_raw);
    const size_t raw_bytes = (size_t)stuff.raw_bytes;
    const DevUpload grow[] = {{&raw, nullptr, 0, place_raw ? raw_bytes + 256 : 0},
                              {&marks, nullptr, 0, place_raw ? raw_bytes / 8 + 256 : 0},
                              {&out, nullptr, 0, (size_t)stuff.out_bytes + 256},
                              {&chunk_ff, nullptr, 0, (size_t)stuff.chunks * sizeof(uint32_t) + 256},
                              {&work_chunk, nullptr, 0, stuff.work_chunk.size() * sizeof(EncWork) + 16}};
    bool copying = false;
    failed = "hipMalloc";
    hipError_t e = reserve_and_copy(grow, stream, &copying);
    if (e != hipSuccess || !place_raw) return e;
    // (emit_kernel ORs into zeroed words; the one-pass form has one writer per word and no restart marks)
    failed = "hipMemsetAsync(raw)";
    e = hipMemsetAsync(raw.ptr, 0, raw_bytes + 256, stream);
    if (e == hipSuccess) e = hipMemsetAsync(marks.ptr, 0, raw_bytes / 8 + 256, stream);
    return e;
}

hipError_t EntropyTail::upload_chunk_work(hipStream_t stream) {
    failed = "hipMemcpyAsync(chunk work)";
    return hipMemcpyAsync(work_chunk.ptr, stuff.work_chunk.data(), stuff.work_chunk.size() * sizeof(EncWork), hipMemcpyHostToDevice, stream);
}

hipError_t EntropyTail::emit(hipStream_t stream, const Source &s) {
    failed = "emit_kernel";
    return launch_emit(stream, s.images, s.work_blk, s.n_work_blk, s.tables, s.coefs, (const uint32_t *)bits.ptr, (const uint64_t *)bit_off.ptr,
                       (const uint64_t *)raw_bits.ptr, (uint8_t *)raw.ptr, (uint32_t *)marks.ptr,
                       (uint32_t)std::min<uint64_t>((emit_words + 1023) & ~1023ull, kEmitLdsWordsMax), s.layouts, s.any_plain);
}

hipError_t EntropyTail::stuff_bytes(hipStream_t stream, const DevEncImage *images) {
    failed = "stuff kernels";
    return launch_stuff(stream, images, (const EncWork *)work_chunk.ptr, (int)stuff.work_chunk.size(), (const uint64_t *)raw_bits.ptr, (const uint8_t *)raw.ptr,
                        (const uint32_t *)marks.ptr, (uint32_t *)chunk_ff.ptr, (uint8_t *)out.ptr, (uint64_t *)out_len.ptr);
}

void EntropyTail::release() {
    for (DevBuffer *b : {&bits, &bit_off, &raw_bits, &raw, &marks, &chunk_ff, &work_chunk, &out, &out_len}) b->release();
}

namespace {
// JpegHuffmanEncodingTable(JpegHuffmanCanonicalCode[]) (ref: JpegHuffmanEncodingTable.cs:21-37), TryWrite (:50-86), GetCode (:94-100)
void resolve_given_table(const jpgpu_encode_huffman_table &t, EncPlan::Slot *slot) {
    const int n = t.num_codes;
    int code_count = 0;
    uint8_t symbol_map[256] = {};
    for (int i = 0; i < n; i++)
        if (t.length[i] != 0) {
            symbol_map[t.symbol[i]] = (uint8_t)i;
            code_count++;
        }
    for (int s = 0; s < 256; s++) {  // a symbol the table does not hold: entry 0
        slot->table.code[s] = t.code[symbol_map[s]];
        slot->table.len[s] = t.length[symbol_map[s]];
    }
    slot->dht.clear();
    for (int len = 1; len <= 16; len++) {
        int count = 0;
        for (int i = n - code_count; i < n; i++) count += t.length[i] == len;
        slot->dht.push_back((uint8_t)count);
    }
    for (int i = n - code_count; i < n; i++) slot->dht.push_back(t.symbol[i]);
}

// the four standard tables in SetHuffmanTable order (DC0, AC0, DC1, AC1): table t's Tc/Th byte, and its 16 counts + symbols
uint8_t std_tc_th(int t) { return (uint8_t)(((t & 1) << 4) | (t >> 1)); }
void append_std_dht(int t, std::vector<uint8_t> *dht) {
    dht->insert(dht->end(), kStd[t].lengths, kStd[t].lengths + 16);
    dht->insert(dht->end(), kStd[t].values, kStd[t].values + kStd[t].count);
}

// ---- what the reference's setters throw on (JpegEncoder.cs:102-240), and what this interface cannot express; the slots
// (d.huffman_tables[]) of every component's DC and AC table on the way
int check_description(const jpgpu_encode_description &d, int dc_slot[4], int ac_slot[4], const char **msg) {
    auto bad = [&](int status, const char *m) {
        *msg = m;
        return status;
    };
    if (d.width <= 0 || d.height <= 0 || d.width > 65535 || d.height > 65535) return bad(JPGPU_ERR_ARGUMENT, "image dimensions out of range");
    if (d.num_components < 0 || d.num_components > JPGPU_ENC_MAX_COMPONENTS) return bad(JPGPU_ERR_ARGUMENT, "1 to 4 components can be described.");
    if (d.num_components == 0) return bad(JPGPU_ERR_INVALID_OPERATION, "No component is specified.");
    if (d.num_quant_tables < 1 || d.num_quant_tables > JPGPU_ENC_MAX_TABLES) return bad(JPGPU_ERR_ARGUMENT, "1 to 8 quantization tables can be described.");
    if (d.num_huffman_tables < 1 || d.num_huffman_tables > JPGPU_ENC_MAX_TABLES) return bad(JPGPU_ERR_ARGUMENT, "1 to 8 Huffman tables can be described.");
    const int nc = d.num_components;
    for (int c = 0; c < nc; c++) {
        const jpgpu_encode_component &k = d.components[c];
        if ((k.h != 1 && k.h != 2 && k.h != 4) || (k.v != 1 && k.v != 2 && k.v != 4)) return bad(JPGPU_ERR_ARGUMENT, "Subsampling factor can only be 1, 2 or 4.");
        for (int o = 0; o < c; o++)
            if (d.components[o].component_index == k.component_index) return bad(JPGPU_ERR_ARGUMENT, "The component index is already used by another component.");
        for (int i = 0; i < 64; i++)
            if (k.quant[i] == 0 || k.quant[i] > 255) return bad(JPGPU_ERR_ARGUMENT, "Quantization table elements must be in 1..255 (element precision 0).");
    }
    for (int t = 0; t < d.num_quant_tables; t++) {
        for (int o = 0; o < t; o++)
            if (d.quant_tables[o].identifier == d.quant_tables[t].identifier) return bad(JPGPU_ERR_ARGUMENT, "A quantization table identifier appears twice.");
        for (int i = 0; i < 64; i++)
            if (d.quant_tables[t].elements[i] == 0 || d.quant_tables[t].elements[i] > 255)
                return bad(JPGPU_ERR_ARGUMENT, "Quantization table elements must be in 1..255 (element precision 0).");
    }
    for (int t = 0; t < d.num_huffman_tables; t++) {
        const jpgpu_encode_huffman_table &h = d.huffman_tables[t];
        if (h.table_class > 1) return bad(JPGPU_ERR_ARGUMENT, "Huffman table class is 0 (DC) or 1 (AC).");
        for (int o = 0; o < t; o++)  // AddTable (JpegHuffmanEncodingTableCollection.cs:82-88) throws InvalidOperationException
            if (d.huffman_tables[o].table_class == h.table_class && d.huffman_tables[o].identifier == h.identifier)
                return bad(JPGPU_ERR_INVALID_OPERATION, "Operation is not valid due to the current state of the object.");
        if (h.given) {
            if (h.num_codes < 1 || h.num_codes > 256) return bad(JPGPU_ERR_ARGUMENT, "A given Huffman table holds 1 to 256 codes.");
            for (int i = 0; i < h.num_codes; i++)
                if (h.length[i] > 16 || (h.length[i] < 16 && (h.code[i] >> h.length[i]) != 0))
                    return bad(JPGPU_ERR_ARGUMENT, "A Huffman code is at most 16 bits long and fits its length.");
        }
    }
    auto find_slot = [&](int cls, int id) {
        for (int t = 0; t < d.num_huffman_tables; t++)
            if (d.huffman_tables[t].table_class == cls && d.huffman_tables[t].identifier == id) return t;
        return -1;
    };
    for (int c = 0; c < nc; c++) {
        dc_slot[c] = find_slot(0, d.components[c].td);
        ac_slot[c] = find_slot(1, d.components[c].ta);
        if (dc_slot[c] < 0 || ac_slot[c] < 0) return bad(JPGPU_ERR_ARGUMENT, "Huffman table is not defined.");
    }
    if (d.in_components < nc || d.in_components > 255) return bad(JPGPU_ERR_ARGUMENT, "The input holds fewer samples per pixel than components were added.");
    if (d.input_rgb < 0 || d.input_rgb > 2) return bad(JPGPU_ERR_ARGUMENT, "input_rgb is 0 (samples), 1 (R,G,B) or 2 (R,G,B,A).");
    if (d.input_rgb && (nc != 3 || d.in_components != (d.input_rgb == 2 ? 4 : 3))) return bad(JPGPU_ERR_ARGUMENT, "RGB input needs 3 components.");
    if (d.restart_interval < 0 || d.restart_interval > 65535) return bad(JPGPU_ERR_ARGUMENT, "restart interval out of range (0..65535)");
    return JPGPU_OK;
}

// ---- tables: a given one in its by-symbol and its DHT form, a builder as a slot to be filled from the image's statistics
void resolve_table_slots(const jpgpu_encode_description &d, EncPlan *plan) {
    plan->n_slots = d.num_huffman_tables;
    plan->slots.assign((size_t)plan->n_slots, EncPlan::Slot());
    plan->most_optimal = d.most_optimal_coding != 0;
    for (int t = 0; t < plan->n_slots; t++) {
        const jpgpu_encode_huffman_table &h = d.huffman_tables[t];
        EncPlan::Slot &s = plan->slots[t];
        memset(&s.table, 0, sizeof s.table);
        s.given = h.given != 0;
        s.tc_th = (uint8_t)((h.table_class << 4) | (h.identifier & 0xf));
        if (s.given) resolve_given_table(h, &s);
        else plan->any_builder = true;
    }
}

// ---- geometry: the general kernels' block map (DevEncLayout).  Returns whether a component has the maximum factors both ways.
bool resolve_block_map(const jpgpu_encode_description &d, const int dc_slot[4], const int ac_slot[4], EncPlan *plan) {
    const int nc = d.num_components;
    DevEncLayout &L = plan->layout[0];
    uint32_t max_h = 1, max_v = 1;
    for (int c = 0; c < nc; c++) {
        max_h = std::max<uint32_t>(max_h, d.components[c].h);
        max_v = std::max<uint32_t>(max_v, d.components[c].v);
    }
    L.ncomp = (uint32_t)nc;
    L.max_h = max_h;
    L.max_v = max_v;
    L.own_blocks = plan->any_builder ? 1 : 0;
    const uint32_t hb = ((uint32_t)d.width + 7) / 8, vb = ((uint32_t)d.height + 7) / 8;
    uint32_t b = 0;
    bool full_resolution = false;
    for (int c = 0; c < 4; c++)
        for (int i = 0; i < 64; i++) L.quant[c][i] = 1;
    for (int c = 0; c < nc; c++) {
        const jpgpu_encode_component &k = d.components[c];
        L.h[c] = k.h;
        L.v[c] = k.v;
        L.hs[c] = (uint8_t)(max_h / k.h);
        L.vs[c] = (uint8_t)(max_v / k.v);
        L.dc_slot[c] = (uint8_t)dc_slot[c];
        L.ac_slot[c] = (uint8_t)ac_slot[c];
        L.first_blk[c] = (uint8_t)b;
        L.grid_w[c] = (hb + L.hs[c] - 1) / L.hs[c];  // JpegBlockAllocator.cs:61-62
        L.grid_h[c] = (vb + L.vs[c] - 1) / L.vs[c];
        for (int i = 0; i < 64; i++) L.quant[c][i] = k.quant[i];
        for (uint32_t y = 0; y < k.v; y++)
            for (uint32_t x = 0; x < k.h; x++) {
                L.blk_comp[b] = (uint8_t)c;
                L.blk_x[b] = (uint8_t)x;
                L.blk_y[b] = (uint8_t)y;
                if (L.hs[c] == 1 && L.vs[c] == 1) L.tail_first = b;
                L.blk_info[b] = (uint32_t)c | (x << 2) | (y << 4) | ((uint32_t)k.h << 6) | ((uint32_t)k.v << 9) | ((uint32_t)dc_slot[c] << 12) |
                                ((uint32_t)ac_slot[c] << 15) | ((uint32_t)L.first_blk[c] << 18) | (((uint32_t)L.first_blk[c] + k.h * k.v - 1u) << 24);
                b++;
            }
        full_resolution = full_resolution || (L.hs[c] == 1 && L.vs[c] == 1);
    }
    plan->bpm = b;
    const uint32_t mcus_per_line = ((uint32_t)d.width + 8 * max_h - 1) / (8 * max_h), mcus_per_column = ((uint32_t)d.height + 8 * max_v - 1) / (8 * max_v);
    if (L.own_blocks) {  // the last block of the last MCU that lies outside its component's grid: what the dummy block ends up as
        const uint32_t last = mcus_per_line * mcus_per_column - 1, mx = last % mcus_per_line, my = last / mcus_per_line;
        for (uint32_t k = 0; k < b; k++) {
            const uint32_t c = L.blk_comp[k];
            if (mx * L.h[c] + L.blk_x[k] >= L.grid_w[c] || my * L.v[c] + L.blk_y[k] >= L.grid_h[c]) L.dummy_blk = last * b + k;
        }
    }
    return full_resolution;
}

// ---- marker segments, from the lists (JpegEncoder.cs:261-280); without builders the DHT is known now and so is all of SOI..SOS
void write_description_segments(const jpgpu_encode_description &d, EncPlan *plan) {
    EncSegmentQuant quant[JPGPU_ENC_MAX_TABLES];
    EncSegmentComponent comp[JPGPU_ENC_MAX_COMPONENTS];
    for (int t = 0; t < d.num_quant_tables; t++) quant[t] = {d.quant_tables[t].identifier, d.quant_tables[t].elements};
    for (int c = 0; c < d.num_components; c++) {
        const jpgpu_encode_component &k = d.components[c];
        comp[c] = {k.component_index, k.h, k.v, k.tq, k.td, k.ta};
    }
    write_marker_segments(quant, d.num_quant_tables, comp, d.num_components, d.width, d.height, d.restart_interval, &plan->header_pre, &plan->header_post);
    if (plan->any_builder) return;
    std::vector<uint8_t> body;
    for (const EncPlan::Slot &s : plan->slots) {
        body.push_back(s.tc_th);
        body.insert(body.end(), s.dht.begin(), s.dht.end());
    }
    assemble_header(plan->header_pre, body, plan->header_post, &plan->header);
}

// ---- an EncodeAction arrangement?  (apps/JpegEncode/EncodeAction.cs:38-63: what jpgpu_encoder_upload describes)
void classify_encode_action(const jpgpu_encode_description &d, EncPlan *plan) {
    const int nc = d.num_components;
    bool legacy = (nc == 1 || nc == 3) && d.num_quant_tables == 2 && d.num_huffman_tables == 4 && d.quant_tables[0].identifier == 0 &&
                  d.quant_tables[1].identifier == 1 && d.in_components == (d.input_rgb == 2 ? 4 : nc);
    for (int c = 0; legacy && c < nc; c++) {
        const jpgpu_encode_component &k = d.components[c];
        const int t = c == 0 ? 0 : 1;
        legacy = k.component_index == c + 1 && k.tq == t && k.td == t && k.ta == t && (c == 0 || (k.h == 1 && k.v == 1)) &&
                 memcmp(k.quant, d.quant_tables[t].elements, sizeof k.quant) == 0;
    }
    for (int t = 0; legacy && t < 4; t++) {  // DC0, AC0, DC1, AC1: the four standard tables, or all four to be built
        const jpgpu_encode_huffman_table &ht = d.huffman_tables[t];
        legacy = ht.table_class == (t & 1) && ht.identifier == (t >> 1) && (ht.given != 0) == (d.huffman_tables[0].given != 0);
        if (legacy && ht.given) {
            EncPlan::Slot s;
            build_enc_table(kStd[t], &s.table);
            append_std_dht(t, &s.dht);
            legacy = s.dht == plan->slots[t].dht && memcmp(&s.table, &plan->slots[t].table, sizeof s.table) == 0;
        }
    }
    if (!legacy) return;
    plan->legacy = true;
    plan->legacy_has_quant = true;
    plan->params.width = d.width;
    plan->params.height = d.height;
    plan->params.components = nc;
    plan->params.luma_h = d.components[0].h;
    plan->params.luma_v = d.components[0].v;
    plan->params.quality = 50;
    plan->params.input_rgb = d.input_rgb;
    plan->params.optimize_coding = plan->any_builder ? (plan->most_optimal ? 2 : 1) : 0;
    plan->params.restart_interval = d.restart_interval;
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < 64; i++) plan->legacy_quant[t][i] = d.quant_tables[t].elements[i];
}
}  // namespace

int resolve_encode_description(const jpgpu_encode_description &d, EncPlan *plan, std::string *error) {
    *plan = EncPlan();
    plan->layout.assign(1, DevEncLayout());
    memset(&plan->layout[0], 0, sizeof(DevEncLayout));
    int dc_slot[4], ac_slot[4];
    const char *msg = "";
    const int rc = check_description(d, dc_slot, ac_slot, &msg);
    if (rc != JPGPU_OK) {
        if (error) *error = msg;
        return rc;
    }
    plan->width = d.width;
    plan->height = d.height;
    plan->in_components = d.in_components;
    plan->input_rgb = d.input_rgb;
    plan->restart_interval = d.restart_interval;
    resolve_table_slots(d, plan);
    const bool full_resolution = resolve_block_map(d, dc_slot, ac_slot, plan);
    write_description_segments(d, plan);
    // ---- what Encode() of this image reports
    if (!full_resolution) {
        plan->status = JPGPU_ERR_NOT_SUPPORTED;
        plan->message = "No component has the maximum sampling factors in both directions: every block then starts from the block encoded before it "
                        "(one block buffer for the whole scan), which is a serial chain over the image.";
        return JPGPU_OK;
    }
    bool fed[JPGPU_ENC_MAX_TABLES] = {};
    for (int c = 0; c < d.num_components; c++) fed[dc_slot[c]] = fed[ac_slot[c]] = true;
    for (int t = 0; t < plan->n_slots; t++)
        if (!plan->slots[t].given && !fed[t]) {  // JpegHuffmanEncodingTableBuilder.Build of a builder no component feeds
            plan->status = JPGPU_ERR_INVALID_OPERATION;
            plan->message = "No symbol is recorded.";
        }
    classify_encode_action(d, plan);
    return JPGPU_OK;
}

EncodeBatch::~EncodeBatch() {
    for (hipEvent_t ev : ev_)
        if (ev) (void)hipEventDestroy(ev);
    for (DevBuffer *b : {&d_samples_, &d_pixels_, &d_images_, &d_tables_, &d_work_mcu_, &d_work_blk_, &d_work_stat_, &d_coefs_, &d_hist_, &d_headers_, &d_chain_,
                         &d_work_order_, &d_layouts_})
        b->release();
    tail_.release();
    prog_.release();
}

int EncodeBatch::fail(int status, const std::string &msg) {
    ctx_->last_error = msg;
    return status;
}
int EncodeBatch::hip_fail(hipError_t e, const char *what) {
    ctx_->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? JPGPU_ERR_OUT_OF_MEMORY : JPGPU_ERR_DEVICE;
}

// ------------------------------------------------------------------------------------------------ upload

int EncodeBatch::upload(const uint8_t *const *pixels, const jpgpu_encode_params *params, int n) {
    if (n < 0 || (n > 0 && (!pixels || !params))) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encode_upload: null argument");
    return upload_params(pixels, params, n, false, nullptr);
}
int EncodeBatch::upload_described(const uint8_t *const *pixels, const jpgpu_encode_description *desc, int n) {
    if (n < 0 || (n > 0 && (!pixels || !desc))) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_upload_described: null argument");
    return upload_descriptions(pixels, desc, n, false, nullptr);
}
int EncodeBatch::upload_device(const void *const *device_pixels, const jpgpu_encode_params *params, const int32_t *pixel_layouts, int n) {
    if (n < 0 || (n > 0 && (!device_pixels || !params))) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_upload_device: null argument");
    return upload_params(reinterpret_cast<const uint8_t *const *>(device_pixels), params, n, true, pixel_layouts);
}
int EncodeBatch::upload_described_device(const void *const *device_pixels, const jpgpu_encode_description *desc, const int32_t *pixel_layouts, int n) {
    if (n < 0 || (n > 0 && (!device_pixels || !desc))) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_upload_described_device: null argument");
    return upload_descriptions(reinterpret_cast<const uint8_t *const *>(device_pixels), desc, n, true, pixel_layouts);
}

int EncodeBatch::set_arithmetic_policy(int policy) {
    if (policy != JPGPU_ARITHMETIC_REFERENCE && policy != JPGPU_ARITHMETIC_LIBJPEG)
        return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_set_arithmetic_policy: the policy is JPGPU_ARITHMETIC_REFERENCE (0) or JPGPU_ARITHMETIC_LIBJPEG (1)");
    arithmetic_policy_ = policy;
    return JPGPU_OK;
}
int EncodeBatch::image_arithmetic(int i, int *arithmetic) const {
    if (i < 0 || i >= (int)images_.size() || !arithmetic) return JPGPU_ERR_ARGUMENT;
    *arithmetic = (int)images_[(size_t)i].arithmetic;
    return JPGPU_OK;
}

int EncodeBatch::set_coding_policy(int policy) {
    if (policy != JPGPU_CODING_STANDARD && policy != JPGPU_CODING_OPTIMIZED && policy != JPGPU_CODING_PROGRESSIVE)
        return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_set_coding_policy: the policy is JPGPU_CODING_STANDARD (0), JPGPU_CODING_OPTIMIZED (1) or JPGPU_CODING_PROGRESSIVE (2)");
    coding_policy_ = policy;
    return JPGPU_OK;
}
int EncodeBatch::image_coding(int i, int *coding) const {
    if (i < 0 || i >= (int)images_.size() || !coding) return JPGPU_ERR_ARGUMENT;
    *coding = coding_;
    return JPGPU_OK;
}

// What the coding policy refuses of an upload, before anything of the encoder's state is touched
int EncodeBatch::check_coding_params(const jpgpu_encode_params *params, int n) {
    if (coding_policy_ == JPGPU_CODING_STANDARD) return JPGPU_OK;
    if (arithmetic_policy_ != JPGPU_ARITHMETIC_LIBJPEG)
        return fail(JPGPU_ERR_ARGUMENT, "JPGPU_CODING_OPTIMIZED and JPGPU_CODING_PROGRESSIVE are libjpeg's codings: they need JPGPU_ARITHMETIC_LIBJPEG (the reference's encoder has optimize_coding).");
    for (int i = 0; i < n && coding_policy_ == JPGPU_CODING_PROGRESSIVE; i++)
        if (params[i].restart_interval != 0) return fail(JPGPU_ERR_ARGUMENT, "JPGPU_CODING_PROGRESSIVE takes no restart interval.");
    return JPGPU_OK;
}

// What the libjpeg policy refuses of an upload, before anything of the encoder's state is touched
int EncodeBatch::check_libjpeg_params(const jpgpu_encode_params *params, int n) {
    for (int i = 0; i < n; i++) {
        const jpgpu_encode_params &p = params[i];
        if (p.optimize_coding != 0)
            return fail(JPGPU_ERR_ARGUMENT, "optimize_coding under JPGPU_ARITHMETIC_LIBJPEG: libjpeg's optimal tables are not this encoder's, the bytes would be neither's.");
        if (!((p.luma_h == 2 && p.luma_v == 2) || (p.luma_h == 2 && p.luma_v == 1) || (p.luma_h == 1 && p.luma_v == 1)))
            return fail(JPGPU_ERR_ARGUMENT, "JPGPU_ARITHMETIC_LIBJPEG takes luma sampling factors 1 x 1, 2 x 1 and 2 x 2.");
    }
    return JPGPU_OK;
}

int EncodeBatch::upload_params(const uint8_t *const *pixels, const jpgpu_encode_params *params, int n, bool device, const int32_t *pixel_layouts) {
    if (arithmetic_policy_ == JPGPU_ARITHMETIC_LIBJPEG) {
        const int rc = check_libjpeg_params(params, n);
        if (rc != JPGPU_OK) return rc;
    }
    int rc = check_coding_params(params, n);
    if (rc != JPGPU_OK) return rc;
    std::vector<EncPlan> plans((size_t)n);
    for (int i = 0; i < n; i++) {
        plans[(size_t)i].legacy = true;
        plans[(size_t)i].params = params[i];
    }
    upload_described_ = false;
    coding_ = coding_policy_;
    rc = upload_plans(pixels, plans, device, pixel_layouts);
    if (rc == JPGPU_OK && coding_ == JPGPU_CODING_PROGRESSIVE) rc = plan_progressive();
    return rc;
}

int EncodeBatch::upload_descriptions(const uint8_t *const *pixels, const jpgpu_encode_description *desc, int n, bool device, const int32_t *pixel_layouts) {
    if (arithmetic_policy_ == JPGPU_ARITHMETIC_LIBJPEG)
        return fail(JPGPU_ERR_INVALID_OPERATION, "A described image is the reference's encoder state: JPGPU_ARITHMETIC_LIBJPEG covers jpgpu_encoder_upload and jpgpu_encoder_upload_device.");
    if (coding_policy_ != JPGPU_CODING_STANDARD)
        return fail(JPGPU_ERR_ARGUMENT, "JPGPU_CODING_OPTIMIZED and JPGPU_CODING_PROGRESSIVE are libjpeg's codings: they need JPGPU_ARITHMETIC_LIBJPEG and jpgpu_encoder_upload.");
    std::vector<EncPlan> plans((size_t)n);
    for (int i = 0; i < n; i++) {
        std::string error;
        const int rc = resolve_encode_description(desc[i], &plans[(size_t)i], &error);
        if (rc != JPGPU_OK) return fail(rc, error);
    }
    upload_described_ = true;
    coding_ = JPGPU_CODING_STANDARD;
    return upload_plans(pixels, plans, device, pixel_layouts);
}

// A device upload hands the kernels the caller's addresses: every image must lie, whole, inside ONE allocation of device memory of
// the context's device -- E1 reads width x height x in_components bytes from it and nothing says so but this check.
int EncodeBatch::check_device_pixels(const uint8_t *const *pixels) {
    for (size_t i = 0; i < images_.size(); i++) {
        const DevEncImage &im = images_[i];
        if (im.width == 0) continue;  // (a refused arrangement: no kernel reads its pixels)
        const std::string which = "jpgpu_encoder_upload_device: image " + std::to_string(i);
        const uint8_t *p = pixels[i];
        const size_t bytes = (size_t)im.width * im.height * im.in_components;
        const int where = check_device_range(ctx_->device, p, bytes);
        if (where == 1) return fail(JPGPU_ERR_ARGUMENT, which + ": the pixels are not in device memory of the context's device");
        if (where == 2) return fail(JPGPU_ERR_ARGUMENT, which + ": " + std::to_string(bytes) + " bytes of pixels do not lie inside one device allocation");
    }
    return JPGPU_OK;
}

// what layout_plans' stages hand one another
struct EncodeBatch::UploadPlan {
    const uint8_t *const *pixels = nullptr;
    bool device = false;
    const int32_t *pixel_layouts = nullptr;
    std::vector<EncWork> work_mcu, work_blk, work_stat;  // per 128 MCUs | per 256 units (blocks or restart intervals) | per 256 blocks
    std::vector<uint32_t> work_order;                    // bits_emit_kernel's issue order
    std::vector<EncHuffTable> tables;
    uint64_t px_off = 0, coef_off = 0, smp_off = 0;
};

int EncodeBatch::upload_plans(const uint8_t *const *pixels, const std::vector<EncPlan> &plans, bool device, const int32_t *pixel_layouts) {
    UploadPlan up;
    up.pixels = pixels;
    up.device = device;
    up.pixel_layouts = pixel_layouts;
    const int rc = layout_plans(up, plans);
    if (rc != JPGPU_OK && device) {  // a refused device upload leaves nothing behind that an encode() could read through
        images_.clear();
        status_.clear();
        n_work_mcu_ = n_work_blk_ = n_work_stat_ = 0;
        encoded_ = false;
    }
    return rc;
}

// Both uploads: an EncodeAction arrangement (plan.legacy) is laid out as it always was, a described one beside it.  The first
// refusal in image order is the call's.
int EncodeBatch::layout_plans(UploadPlan &up, const std::vector<EncPlan> &plans) {
    const int n = (int)plans.size();
    int rc = check_device_arguments(up, n);
    if (rc != JPGPU_OK) return rc;
    hipError_t e = hipSetDevice(ctx_->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    reset_upload_state(n);
    for (int i = 0; i < n; i++) {
        const EncPlan &pl = plans[(size_t)i];
        rc = pl.legacy ? plan_encode_action_image(up, i, pl) : plan_described_image(up, i, pl);
        if (rc != JPGPU_OK) return rc;
    }
    if (up.device) {  // (every argument check is behind us, nothing has been enqueued)
        rc = check_device_pixels(up.pixels);
        if (rc != JPGPU_OK) return rc;
    }
    pixels_on_device_ = up.device;
    total_blocks_ = up.coef_off;
    n_work_mcu_ = (int)up.work_mcu.size();
    n_work_blk_ = (int)up.work_blk.size();
    n_work_stat_ = (int)up.work_stat.size();
    place_table_slots(up);
    return reserve_and_upload(up);
}

int EncodeBatch::check_device_arguments(const UploadPlan &up, int n) {
    for (int i = 0; i < n && up.device; i++) {
        if (!up.pixels[i]) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_upload_device: null pixel pointer");
        if (up.pixel_layouts && up.pixel_layouts[i] != JPGPU_PIXELS_INTERLEAVED && up.pixel_layouts[i] != JPGPU_PIXELS_PLANAR)
            return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_upload_device: a pixel layout is JPGPU_PIXELS_INTERLEAVED (0) or JPGPU_PIXELS_PLANAR (1)");
    }
    return JPGPU_OK;
}

void EncodeBatch::reset_upload_state(int n) {
    images_.assign((size_t)n, DevEncImage());
    headers_.assign((size_t)n, std::vector<uint8_t>());
    headers_pre_.assign((size_t)n, std::vector<uint8_t>());
    headers_post_.assign((size_t)n, std::vector<uint8_t>());
    optimized_.clear();
    most_optimal_.assign((size_t)n, 0);
    status_.assign((size_t)n, JPGPU_OK);
    messages_.assign((size_t)n, "No symbol is recorded.");
    general_.clear();
    general_plans_.clear();
    layouts_.clear();
    any_general_builder_ = false;
    encoded_ = false;
    any_restart_ = false;
    emit_hint_ = 0;
}

// where image i's pixels are, and how they are laid out (width, height set)
int EncodeBatch::place_pixels(const UploadPlan &up, int i, int input_rgb) {
    DevEncImage &im = images_[i];
    im.px_off = up.device ? (uint64_t)(uintptr_t)up.pixels[i] : up.px_off;
    im.px_planar = (up.device && up.pixel_layouts && up.pixel_layouts[i] == JPGPU_PIXELS_PLANAR) ? 1u : 0u;
    im.plane_stride = (uint64_t)im.width * im.height;
    if (im.px_planar && input_rgb == 2) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_upload_device: Rgba32 pixels (input_rgb == 2) have no planar layout");
    return JPGPU_OK;
}

// The geometry of an image that encodes (sampling factors, bpm, restart interval and pixel format set), its place in the pixel and
// coefficient buffers and its workgroups: per 128 MCUs (E1), per 256 units (E2 / E3) and, with tables to build, per 256 blocks
void EncodeBatch::plan_image_work(UploadPlan &up, int i, bool statistics) {
    DevEncImage &im = images_[i];
    im.mcus_per_line = (im.width + 8 * im.luma_h - 1) / (8 * im.luma_h);
    im.mcus_per_column = (im.height + 8 * im.luma_v - 1) / (8 * im.luma_v);
    im.total_blocks = im.mcus_per_line * im.mcus_per_column * im.bpm;
    // restart intervals (an extension, see jpgpu_encode_params): block_bits / emit then take one lane per INTERVAL
    any_restart_ = any_restart_ || im.restart_interval != 0;
    im.n_units = im.restart_interval ? (im.mcus_per_line * im.mcus_per_column + im.restart_interval - 1) / im.restart_interval : im.total_blocks;
    up.px_off = align_up64(up.px_off + (uint64_t)im.width * im.height * im.in_components, 256);
    up.coef_off += im.total_blocks;
    const uint32_t total_mcus = im.mcus_per_line * im.mcus_per_column;
    for (uint32_t f = 0; f < total_mcus; f += kEncMcusPerWg) up.work_mcu.push_back({(uint32_t)i, f});
    im.work_first = (uint32_t)up.work_blk.size();
    for (uint32_t f = 0; f < im.n_units; f += 256) up.work_blk.push_back({(uint32_t)i, f});
    if (statistics)
        for (uint32_t f = 0; f < im.total_blocks; f += 256) up.work_stat.push_back({(uint32_t)i, f});
}

// A described arrangement: the general kernels (DevEncLayout); a refused one holds no work at all.  (The layout's table slots are
// placed once the number of EncodeAction images with built tables is known: place_table_slots.)
int EncodeBatch::plan_described_image(UploadPlan &up, int i, const EncPlan &pl) {
    DevEncImage &im = images_[i];
    memset(&im, 0, sizeof im);
    status_[i] = pl.status;
    if (pl.status != JPGPU_OK) messages_[i] = pl.message;
    const DevEncLayout &pll = pl.layout[0];
    im.coef_off = up.coef_off;
    general_.push_back(i);
    general_plans_.push_back(pl);
    layouts_.push_back(pll);
    im.layout = (uint32_t)layouts_.size();
    im.width = (uint32_t)pl.width;
    im.height = (uint32_t)pl.height;
    im.in_components = (uint32_t)pl.in_components;
    im.components = pll.ncomp;
    im.luma_h = pll.max_h;
    im.luma_v = pll.max_v;
    im.input_rgb = pl.input_rgb ? 1 : 0;
    im.restart_interval = (uint32_t)pl.restart_interval;
    const int rc = place_pixels(up, i, pl.input_rgb);
    if (rc != JPGPU_OK) return rc;
    rgb_ycc_factors(im.r2y);
    if (pl.status != JPGPU_OK) {
        im.work_first = (uint32_t)up.work_blk.size();
        im.width = im.height = im.restart_interval = 0;  // (no pixels are uploaded for it)
        return JPGPU_OK;
    }
    im.bpm = pl.bpm;
    plan_image_work(up, i, pl.any_builder);
    any_general_builder_ = any_general_builder_ || pl.any_builder;
    headers_[i] = pl.header;
    headers_pre_[i] = pl.header_pre;
    headers_post_[i] = pl.header_post;
    im.header_len = (uint32_t)pl.header.size();
    // tables to be built: the DHT is written once the statistics are in; reserve the largest it can be
    if (pl.any_builder) im.header_len = (uint32_t)(pl.header_pre.size() + 4 + (size_t)pl.n_slots * (1 + 16 + 256) + pl.header_post.size());
    return JPGPU_OK;
}

// An EncodeAction arrangement (apps/JpegEncode/EncodeAction.cs:38-63): tables 0 and 1, components 1..3 with the luma factors on the
// first, the four standard Huffman tables or four built ones
int EncodeBatch::plan_encode_action_image(UploadPlan &up, int i, const EncPlan &pl) {
    const jpgpu_encode_params &p = pl.params;
    // argument checks of the reference's setters (JpegEncoder.cs:175-184, EncodeAction.cs:19-22)
    if (p.quality <= 0 || p.quality > 100) return fail(JPGPU_ERR_ARGUMENT, "Specified argument was out of the range of valid values. (Parameter 'quality')");
    if ((p.luma_h != 1 && p.luma_h != 2 && p.luma_h != 4) || (p.luma_v != 1 && p.luma_v != 2 && p.luma_v != 4))
        return fail(JPGPU_ERR_ARGUMENT, "Subsampling factor can only be 1, 2 or 4.");
    if (p.width <= 0 || p.height <= 0 || p.width > 65535 || p.height > 65535) return fail(JPGPU_ERR_ARGUMENT, "image dimensions out of range");
    if (p.components != 1 && p.components != 3) return fail(JPGPU_ERR_NOT_SUPPORTED, "1 or 3 components are supported.");
    if (p.input_rgb && p.components != 3) return fail(JPGPU_ERR_ARGUMENT, "RGB input needs 3 components.");
    if (p.input_rgb < 0 || p.input_rgb > 2) return fail(JPGPU_ERR_ARGUMENT, "input_rgb is 0 (samples), 1 (R,G,B) or 2 (R,G,B,A).");
    if (p.restart_interval < 0 || p.restart_interval > 65535) return fail(JPGPU_ERR_ARGUMENT, "restart interval out of range (0..65535)");
    DevEncImage &im = images_[i];
    memset(&im, 0, sizeof im);
    im.coef_off = up.coef_off;
    im.width = (uint32_t)p.width;
    im.height = (uint32_t)p.height;
    const int rc = place_pixels(up, i, p.input_rgb);
    if (rc != JPGPU_OK) return rc;
    im.in_components = p.input_rgb == 2 ? 4u : (uint32_t)p.components;  // (2: Rgba32 pixels, the alpha byte stepped over)
    im.components = (uint32_t)p.components;
    // (the policy is read for jpgpu_encode_params alone: a described EncodeAction arrangement is refused under it before it gets here)
    const bool libjpeg = arithmetic_policy_ == JPGPU_ARITHMETIC_LIBJPEG && !pl.legacy_has_quant;
    im.arithmetic = libjpeg ? JPGPU_ARITHMETIC_LIBJPEG : JPGPU_ARITHMETIC_REFERENCE;
    // libjpeg: one component is a non-interleaved scan, one block per MCU whatever its factors, and Pillow writes them as 1 x 1
    im.luma_h = libjpeg && p.components == 1 ? 1u : (uint32_t)p.luma_h;
    im.luma_v = libjpeg && p.components == 1 ? 1u : (uint32_t)p.luma_v;
    im.bpm = im.luma_h * im.luma_v + (im.components == 3 ? 2 : 0);
    im.input_rgb = p.input_rgb ? 1 : 0;
    im.restart_interval = (uint32_t)p.restart_interval;
    const bool libjpeg_tables = libjpeg && coding_ == JPGPU_CODING_OPTIMIZED;  // built from the image by libjpeg's rule (build_libjpeg_tables)
    if (p.optimize_coding || libjpeg_tables) {
        most_optimal_[i] = p.optimize_coding == 2;  // JpegEncoder.MostOptimalCoding
        optimized_.push_back(i);
        im.table_base = 4u * (uint32_t)optimized_.size();  // tables 0..3 are the standard ones
    }
    rgb_ycc_factors(im.r2y);
    if (pl.legacy_has_quant) {  // the described form of SetQuantizationTable(0 / 1)
        memcpy(im.quant, pl.legacy_quant, sizeof im.quant);
    } else {
        scale_by_quality(kStdLum, p.quality, im.quant[0]);
        scale_by_quality(kStdChr, p.quality, im.quant[1]);
    }
    plan_image_work(up, i, p.optimize_coding != 0 || libjpeg_tables);
    if (libjpeg) {  // (E1J gathers into LDS: no samples in HBM; the standard coding builds no tables: the header is final)
        write_libjpeg_header(im, p.restart_interval, &headers_[i], nullptr, coding_ == JPGPU_CODING_PROGRESSIVE ? 0xC2 : 0xC0);
        im.header_len = (uint32_t)headers_[i].size();
        // built tables: the DHT segments are written once the statistics are in; reserve the largest they can be (256 values each)
        if (libjpeg_tables) im.header_len += 4u * 256u;
        return JPGPU_OK;
    }
    if ((up.smp_off >> 8) > 0xFFFFFFFFull) return fail(JPGPU_ERR_OUT_OF_MEMORY, "sample buffer beyond 1 TiB");
    im.smp_off_256 = (uint32_t)(up.smp_off >> 8);
    // (an image fdct_fused_kernel takes has no gathered samples: 4.2 GB less per 256 x 4K)
    if (!enc_fused_enabled() || enc_image_fused_shape(im) == 0)
        up.smp_off = align_up64(up.smp_off + (uint64_t)im.mcus_per_line * im.mcus_per_column * enc_sample_bytes_per_mcu(im.luma_h, im.luma_v, im.components), 256);

    // the marker segments Encode() writes, from EncodeAction's fixed lists; the four standard tables until the statistics say otherwise
    const EncSegmentQuant quant[2] = {{0, im.quant[0]}, {1, im.quant[1]}};
    EncSegmentComponent comp[3];
    for (int c = 0; c < (int)im.components; c++) {
        const uint8_t t = c == 0 ? 0 : 1;
        comp[c] = {(uint8_t)(c + 1), (uint8_t)(c == 0 ? im.luma_h : 1), (uint8_t)(c == 0 ? im.luma_v : 1), t, t, t};
    }
    write_marker_segments(quant, 2, comp, (int)im.components, p.width, p.height, p.restart_interval, &headers_pre_[i], &headers_post_[i]);
    std::vector<uint8_t> body;
    for (int t = 0; t < 4; t++) {
        body.push_back(std_tc_th(t));
        append_std_dht(t, &body);
    }
    assemble_header(headers_pre_[i], body, headers_post_[i], &headers_[i]);
    im.header_len = (uint32_t)headers_[i].size();
    // optimizeCoding: the DHT is written once the statistics are in; reserve the largest it can be (4 x 256 symbols)
    if (im.table_base != 0) im.header_len = (uint32_t)(headers_pre_[i].size() + 4 + 4 * (1 + 16 + 256) + headers_post_[i].size());
    return JPGPU_OK;
}

// bits_emit_kernel's issue order, and the Huffman tables of the upload: the four standard ones, four per EncodeAction image with
// built tables (filled in by encode()), eight slots per described image with its given tables known now
void EncodeBatch::place_table_slots(UploadPlan &up) {
    // the work list's entries by (place inside the image, image)
    up.work_order.resize(up.work_blk.size());
    for (size_t k = 0; k < up.work_order.size(); k++) up.work_order[k] = (uint32_t)k;
    std::stable_sort(up.work_order.begin(), up.work_order.end(), [&](uint32_t a, uint32_t b) { return up.work_blk[a].first < up.work_blk[b].first; });

    up.tables.resize(4 + 4 * optimized_.size() + 8 * general_.size());
    memset(up.tables.data(), 0, up.tables.size() * sizeof(EncHuffTable));
    for (int t = 0; t < 4; t++) build_enc_table(kStd[t], &up.tables[t]);
    for (size_t g = 0; g < general_.size(); g++) {
        layouts_[g].table_base = (uint32_t)(4 + 4 * optimized_.size() + 8 * g);
        layouts_[g].hist_index = (uint32_t)(images_.size() * 4 * 256 + g * 8 * 256);
        for (int t = 0; t < general_plans_[g].n_slots; t++)
            if (general_plans_[g].slots[t].given) up.tables[layouts_[g].table_base + (size_t)t] = general_plans_[g].slots[t].table;
    }
}

int EncodeBatch::reserve_and_upload(const UploadPlan &up) {
    const size_t n = images_.size();
    const DevUpload ups[] = {
        {&d_tables_, up.tables.data(), up.tables.size() * sizeof(EncHuffTable), 0},
        {&d_hist_, nullptr, 0, (n * 4 + general_.size() * 8) * 256 * sizeof(uint32_t) + 256},
        {&d_layouts_, layouts_.data(), layouts_.size() * sizeof(DevEncLayout), 256},
        {&d_work_mcu_, up.work_mcu.data(), up.work_mcu.size() * sizeof(EncWork), 0},
        {&d_work_blk_, up.work_blk.data(), up.work_blk.size() * sizeof(EncWork), 0},
        {&d_work_order_, up.work_order.data(), up.work_order.size() * sizeof(uint32_t), 16},
        {&d_work_stat_, up.work_stat.data(), up.work_stat.size() * sizeof(EncWork), 16},
        {&d_coefs_, nullptr, 0, (size_t)total_blocks_ * 128 + 256},
        {&d_samples_, nullptr, 0, (size_t)up.smp_off + 256},
        {&d_images_, nullptr, 0, n * sizeof(DevEncImage) + 256},
    };
    bool copying = false;
    hipError_t e = reserve_and_copy(ups, ctx_->stream, &copying);
    if (e != hipSuccess) return hip_fail(e, copying ? "hipMemcpyAsync" : "hipMalloc");
    if ((e = tail_.reserve(total_blocks_, up.work_blk.size(), n)) != hipSuccess) return hip_fail(e, tail_.failed);
    // (a device upload copies nothing: E1 reads the caller's memory)
    if (!up.device && (e = d_pixels_.reserve((size_t)up.px_off + 256)) != hipSuccess) return hip_fail(e, "hipMalloc");
    for (size_t i = 0; i < n && !up.device; i++) {
        const DevEncImage &im = images_[i];
        if (im.width == 0) continue;  // (a refused arrangement)
        e = hipMemcpyAsync((uint8_t *)d_pixels_.ptr + im.px_off, up.pixels[i], (size_t)im.width * im.height * im.in_components, hipMemcpyHostToDevice,
                           ctx_->stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(pixels)");
    }
    e = hipStreamSynchronize(ctx_->stream);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, "hipStreamSynchronize(upload)");
}

int EncodeBatch::set_quantization_table(int i, int identifier, const uint16_t *zigzag64) {
    if (i < 0 || i >= (int)images_.size() || !zigzag64) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encoder_set_quantization_table: bad argument");
    if (upload_described_)  // (a description carries its tables: captured ones per component, the DQT's as a list of its own)
        return fail(JPGPU_ERR_INVALID_OPERATION, "jpgpu_encoder_set_quantization_table belongs to jpgpu_encoder_upload: a described image carries its tables.");
    if (identifier != 0 && identifier != 1) return fail(JPGPU_ERR_NOT_SUPPORTED, "Quantization table identifiers 0 and 1 are supported.");
    for (int k = 0; k < 64; k++)
        if (zigzag64[k] == 0 || zigzag64[k] > 255) return fail(JPGPU_ERR_ARGUMENT, "Quantization table elements must be in 1..255 (element precision 0).");
    DevEncImage &im = images_[(size_t)i];
    if (im.arithmetic == JPGPU_ARITHMETIC_LIBJPEG) {  // write_libjpeg_header's DQT segment of this table, if it wrote one
        const size_t at = libjpeg_header_quant_at(im, identifier);
        for (int k = 0; k < 64; k++) {
            im.quant[identifier][k] = zigzag64[k];
            if (at) headers_[(size_t)i][at + (size_t)k] = (uint8_t)zigzag64[k];
        }
        encoded_ = false;
        return JPGPU_OK;
    }
    // the DQT segment write_marker_segments wrote: SOI, FF DB, length, then per table one identifier byte + 64 elements
    const size_t at = 2 + 2 + 2 + (size_t)identifier * 65 + 1;
    for (int k = 0; k < 64; k++) {
        im.quant[identifier][k] = zigzag64[k];
        headers_[(size_t)i][at + (size_t)k] = (uint8_t)zigzag64[k];
        headers_pre_[(size_t)i][at + (size_t)k] = (uint8_t)zigzag64[k];
    }
    encoded_ = false;
    return JPGPU_OK;
}

// ------------------------------------------------------------------------------------------------ encode

// what encode()'s stages hand one another
struct EncodeBatch::EncodeRun {
    int n = 0;                                // images
    const DevEncLayout *layouts = nullptr;    // described images in the upload: their layouts on the device
    bool any_plain = false;                   // EncodeAction arrangements in the upload
    bool fused_emit = false;                  // bits_emit_kernel has counted AND written the raw streams
};

int EncodeBatch::encode() {
    hipError_t e = hipSetDevice(ctx_->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    EncodeRun r;
    r.n = (int)images_.size();
    if (r.n == 0) return JPGPU_OK;
    for (hipEvent_t &ev : ev_)
        if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) return hip_fail(e, "hipEventCreate");
    r.layouts = layouts_.empty() ? nullptr : (const DevEncLayout *)d_layouts_.ptr;
    r.any_plain = layouts_.size() < images_.size();
    tail_.h_raw_bits.assign((size_t)r.n, 0);
    int rc = upload_image_descriptors();
    if (rc != JPGPU_OK) return rc;
    (void)hipEventRecord(ev_[0], ctx_->stream);
    if ((rc = run_fdct(r)) != JPGPU_OK) return rc;
    if ((!optimized_.empty() || any_general_builder_) && (rc = build_coding_tables(r)) != JPGPU_OK) return rc;
    (void)hipEventRecord(ev_[1], ctx_->stream);
    if (coding_ == JPGPU_CODING_PROGRESSIVE) return encode_progressive();  // (its own entropy coder, ev_[2] .. ev_[5] at its stages)
    if ((rc = try_one_pass_emit(r)) != JPGPU_OK) return rc;
    if (!r.fused_emit && (rc = count_bits_two_kernels(r)) != JPGPU_OK) return rc;  // (ev_[2] is recorded behind whichever kernel counted)
    if ((rc = plan_stuffing(r)) != JPGPU_OK) return rc;
    if ((rc = place_headers(r)) != JPGPU_OK) return rc;
    (void)hipEventRecord(ev_[3], ctx_->stream);
    if ((rc = emit_and_stuff(r)) != JPGPU_OK) return rc;  // (ev_[4] between E3 and E4, ev_[5] behind E4)
    encoded_ = true;
    return JPGPU_OK;
}

// image descriptors (raw / output offsets are filled in once the bit counts are known)
int EncodeBatch::upload_image_descriptors() {
    hipError_t e = hipMemcpyAsync(d_images_.ptr, images_.data(), images_.size() * sizeof(DevEncImage), hipMemcpyHostToDevice, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(images)");
    if (n_work_blk_ == 0) {  // nothing but refused arrangements: no kernel counts anything, the streams are empty
        e = hipMemsetAsync(tail_.raw_bits.ptr, 0, images_.size() * sizeof(uint64_t), ctx_->stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(bit counts)");
    }
    return JPGPU_OK;
}

// E1: pixels -> quantised blocks
int EncodeBatch::run_fdct(const EncodeRun &r) {
    size_t max_record = 0;
    uint32_t fused_shapes = 0;
    uint32_t libjpeg_shapes = 0;  // (launch_fdct_libjpeg: 2 x 2, 2 x 1, 1 x 1)
    bool any_other = false, any_other_planar = false;
    // (a device upload: DevEncImage.px_off is the caller's address itself)
    const uint8_t *pixel_base = pixels_on_device_ ? nullptr : (const uint8_t *)d_pixels_.ptr;
    const bool no_fused = !enc_fused_enabled();
    for (const DevEncImage &im : images_) {
        if (im.layout != 0) continue;  // (enc_general_fdct_kernel)
        if (im.arithmetic == JPGPU_ARITHMETIC_LIBJPEG) {
            libjpeg_shapes |= im.luma_h == 1 ? 4u : (im.luma_v == 1 ? 2u : 1u);
            continue;
        }
        max_record = std::max(max_record, enc_sample_bytes_per_mcu(im.luma_h, im.luma_v, im.components));
        const int shape = no_fused ? 0 : enc_image_fused_shape(im);
        if (shape != 0) fused_shapes |= 1u << shape;
        else (im.px_planar ? any_other_planar : any_other) = true;
    }
    hipError_t e = launch_fdct_quant(ctx_->stream, pixel_base, (const DevEncImage *)d_images_.ptr, (const EncWork *)d_work_mcu_.ptr, n_work_mcu_,
                                     (uint8_t *)d_samples_.ptr, (int16_t *)d_coefs_.ptr, max_record, fused_shapes, any_other, any_other_planar);
    if (e != hipSuccess) return hip_fail(e, "fdct_quant_kernel");
    if (libjpeg_shapes) {
        e = launch_fdct_libjpeg(ctx_->stream, pixel_base, (const DevEncImage *)d_images_.ptr, (const EncWork *)d_work_mcu_.ptr, n_work_mcu_, (int16_t *)d_coefs_.ptr,
                                libjpeg_shapes);
        if (e != hipSuccess) return hip_fail(e, "e1j_fdct_kernel");
    }
    if (r.layouts) {
        e = launch_fdct_quant_general(ctx_->stream, pixel_base, (const DevEncImage *)d_images_.ptr, r.layouts, (const EncWork *)d_work_mcu_.ptr, n_work_mcu_,
                                      (int16_t *)d_coefs_.ptr);
        if (e != hipSuccess) return hip_fail(e, "enc_general_fdct_kernel");
    }
    return JPGPU_OK;
}

// One image's tables from its counters, and its SOI..SOS with the DHT they make: every builder of the collection in SetHuffmanTable
// order -- an EncodeAction image's four (DC0, AC0, DC1, AC1; `described` null), or a described image's slots, of which the given
// ones keep their bytes.  false: a builder without symbols, the tables behind it not built (what that means is the caller's).
bool EncodeBatch::build_image_tables(int i, const EncPlan *described, const uint32_t *counters, bool most_optimal, EncHuffTable *tables) {
    std::vector<uint8_t> body;
    bool built = true;
    for (int t = 0; t < (described ? described->n_slots : 4); t++) {
        const EncPlan::Slot *slot = described ? &described->slots[t] : nullptr;
        std::vector<OptimalCode> codes;
        if (slot && slot->given) {
            tables[t] = slot->table;
            body.push_back(slot->tc_th);
            body.insert(body.end(), slot->dht.begin(), slot->dht.end());
        } else if (build_optimal_table(counters + (size_t)t * 256, &codes, most_optimal)) {
            body.push_back(slot ? slot->tc_th : std_tc_th(t));
            optimal_codes_to_table(codes, &tables[t], &body);
        } else {
            built = false;
            break;
        }
    }
    assemble_header(headers_pre_[i], body, headers_post_[i], &headers_[i]);
    images_[i].header_len = (uint32_t)headers_[i].size();
    return built;
}

// JPGPU_CODING_OPTIMIZED: the tables libjpeg builds from the image's counters (DC0, AC0 and, with three components, DC1, AC1), and the
// header with their DHT segments
bool EncodeBatch::build_libjpeg_tables(int i, const uint32_t *counters, EncHuffTable *tables) {
    const DevEncImage &im = images_[i];
    std::vector<std::vector<uint8_t>> dht(4);
    for (int t = 0; t < (im.components == 3 ? 4 : 2); t++)
        libjpeg_build_table(counters + (size_t)t * 256, (uint8_t)(((t & 1) << 4) | (t >> 1)), &tables[t], &dht[(size_t)t]);
    write_libjpeg_header(im, (int)im.restart_interval, &headers_[i], &dht);
    images_[i].header_len = (uint32_t)headers_[i].size();
    return true;
}

// optimizeCoding: BuildHuffmanTables (:491-550) -- statistics on the device, JpegHuffmanEncodingTableBuilder.Build on the host
int EncodeBatch::build_coding_tables(const EncodeRun &r) {
    const size_t n_hist = ((size_t)r.n * 4 + general_.size() * 8) * 256;
    hipError_t e = hipMemsetAsync(d_hist_.ptr, 0, n_hist * sizeof(uint32_t), ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(statistics)");
    e = launch_block_stats(ctx_->stream, (const DevEncImage *)d_images_.ptr, (const EncWork *)d_work_stat_.ptr, n_work_stat_, (const int16_t *)d_coefs_.ptr,
                           (uint32_t *)d_hist_.ptr, any_general_builder_ ? r.layouts : nullptr, !optimized_.empty());
    if (e != hipSuccess) return hip_fail(e, "block_stats_kernel");
    std::vector<uint32_t> hist(n_hist);
    e = hipMemcpyAsync(hist.data(), d_hist_.ptr, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx_->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(statistics)");
    std::vector<EncHuffTable> built(4 * optimized_.size());
    memset(built.data(), 0, built.size() * sizeof(EncHuffTable));
    for (size_t k = 0; k < optimized_.size(); k++) {
        const int i = optimized_[k];
        status_[i] = JPGPU_OK;
        if (images_[i].arithmetic == JPGPU_ARITHMETIC_LIBJPEG) {
            build_libjpeg_tables(i, &hist[(size_t)i * 4 * 256], &built[4 * k]);
            continue;
        }
        // "No symbol is recorded." (a single-component image: empty chrominance builders)
        if (!build_image_tables(i, nullptr, &hist[(size_t)i * 4 * 256], most_optimal_[i] != 0, &built[4 * k])) status_[i] = JPGPU_ERR_INVALID_OPERATION;
    }
    e = built.empty() ? hipSuccess
                      : hipMemcpyAsync((EncHuffTable *)d_tables_.ptr + 4, built.data(), built.size() * sizeof(EncHuffTable), hipMemcpyHostToDevice, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(built tables)");
    // described images: every builder of the collection from the counters of its slot (the components that share a table have
    // added theirs up there)
    std::vector<EncHuffTable> slots(any_general_builder_ ? 8 * general_.size() : 0);
    for (size_t g = 0; g < general_.size(); g++) {
        const int i = general_[g];
        const EncPlan &pl = general_plans_[g];
        if (!pl.any_builder || pl.status != JPGPU_OK) continue;
        if (!build_image_tables(i, &pl, &hist[layouts_[g].hist_index], pl.most_optimal != 0, &slots[8 * g])) {
            status_[i] = JPGPU_ERR_INVALID_OPERATION;  // (resolve_encode_description has seen every such case: not reached)
            messages_[i] = "No symbol is recorded.";
        }
        e = hipMemcpyAsync((EncHuffTable *)d_tables_.ptr + layouts_[g].table_base, &slots[8 * g], 8 * sizeof(EncHuffTable), hipMemcpyHostToDevice, ctx_->stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(built tables)");
    }
    if (any_general_builder_) {  // (`slots` leaves scope; the EncodeAction images' upload is as it always was)
        e = hipStreamSynchronize(ctx_->stream);
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(built tables)");
    }
    return JPGPU_OK;
}

// E2 + E3 as one pass (bits_emit_kernel): the raw streams are placed BEFORE their sizes are known -- a slot of the worst case
// per image (every coefficient a 32-bit field: 256 bytes per block), of which only the stream itself is ever touched
// The chains are per image: a batch of ONE image is one chain, as long as the image has workgroups, and runs at the speed the
// look-back travels (one 8192 x 8192 canvas: 0.13 ms against the two kernels' 0.107); from two images on the one pass wins.
int EncodeBatch::try_one_pass_emit(EncodeRun &r) {
    // (bits_emit_kernel: EncodeAction arrangements)
    if (!enc_fused_emit_enabled() || any_restart_ || emit_hint_ == 0xFFFFFFFFu || r.n < 2 || !layouts_.empty()) return JPGPU_OK;
    uint64_t slot = 0;
    const size_t chain_bytes = 256 + enc_chain_bytes(n_work_blk_);  // control words | one record per workgroup
    for (DevEncImage &im : images_) {
        im.raw_off = slot;
        slot = align_up64(slot + (uint64_t)im.total_blocks * 256 + 64, 256);
    }
    // The worst case is ~50 x the streams themselves (51 GB per 1024 x 4K 4:2:0 where the two kernels size ~1 GB from the counts)
    // and d_raw_ never shrinks: the slots may take a third of what the device has free, no more -- the finished streams, the
    // chunk counts and the next upload's buffers are reserved behind them, and a batch that used to encode must not fail there
    // because this one grabbed the rest.  Beyond that the two kernels run.
    size_t free_b = 0, total_b = 0;
    hipError_t e = (size_t)slot + 256 <= tail_.raw.cap ? hipSuccess : hipMemGetInfo(&free_b, &total_b);
    if (e == hipSuccess && (size_t)slot + 256 > tail_.raw.cap && (size_t)slot + 256 > free_b / 3) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = tail_.raw.reserve((size_t)slot + 256);
    if (e == hipSuccess) e = d_chain_.reserve(chain_bytes + 256);
    if (e != hipSuccess) {  // no room for the worst-case slots: the two kernels size the raw streams from the counts
        (void)hipGetLastError();
        emit_hint_ = 0xFFFFFFFFu;
        return JPGPU_OK;
    }
    one_pass_emits_++;
    e = hipMemsetAsync(d_chain_.ptr, 0, chain_bytes, ctx_->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_images_.ptr, images_.data(), (size_t)r.n * sizeof(DevEncImage), hipMemcpyHostToDevice, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(images)");
    e = launch_bits_emit(ctx_->stream, (const DevEncImage *)d_images_.ptr, (const EncWork *)d_work_blk_.ptr, n_work_blk_, (const EncHuffTable *)d_tables_.ptr,
                         (const int16_t *)d_coefs_.ptr, (uint8_t *)d_chain_.ptr + 256, (uint32_t *)d_chain_.ptr, (uint8_t *)tail_.raw.ptr,
                         (uint64_t *)tail_.raw_bits.ptr, emit_hint_ ? emit_hint_ : 4096u, (const uint32_t *)d_work_order_.ptr);
    if (e != hipSuccess) return hip_fail(e, "bits_emit_kernel");
    (void)hipEventRecord(ev_[2], ctx_->stream);
    uint32_t ctl[2] = {0, 0};
    e = hipMemcpyAsync(tail_.h_raw_bits.data(), tail_.raw_bits.ptr, (size_t)r.n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx_->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ctl, d_chain_.ptr, sizeof ctl, hipMemcpyDeviceToHost, ctx_->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(bit counts)");
    r.fused_emit = ctl[1] == 0;
    if (!r.fused_emit) {  // a stretch beyond the LDS buffer, or a wait that ran out: this upload takes the two kernels from here on
        emit_hint_ = 0xFFFFFFFFu;
        fused_emit_fallbacks_++;
    }
    return JPGPU_OK;
}

EntropyTail::Source EncodeBatch::tail_source(const EncodeRun &r) const {
    return {(const DevEncImage *)d_images_.ptr, (const EncWork *)d_work_blk_.ptr, n_work_blk_, (const EncHuffTable *)d_tables_.ptr, (const int16_t *)d_coefs_.ptr,
            r.layouts, r.any_plain};
}

// E2 as its own kernel (E3 follows the stuffing stage's layout: emit_and_stuff)
int EncodeBatch::count_bits_two_kernels(const EncodeRun &r) {
    hipError_t e = tail_.count_bits(ctx_->stream, tail_source(r), r.n);
    if (e != hipSuccess) return hip_fail(e, tail_.failed);
    (void)hipEventRecord(ev_[2], ctx_->stream);
    // the sizes of the raw and finished streams depend on the data: one host round trip
    e = tail_.read_bit_counts(ctx_->stream, r.n);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, tail_.failed);
}

// where the stuffing stage reads and writes, E3's LDS buffer, and the buffers both need
int EncodeBatch::plan_stuffing(const EncodeRun &r) {
    // (the one-pass form has placed and written the raw streams already)
    const hipError_t e = tail_.plan(ctx_->stream, images_.data(), r.n, !r.fused_emit);
    if (e != hipSuccess) return hip_fail(e, tail_.failed);
    // the next encode() of this upload sizes bits_emit_kernel's LDS buffer like emit_kernel's (no stretch would fit: never again)
    if (emit_hint_ != 0xFFFFFFFFu)
        emit_hint_ = tail_.emit_words == 0 ? 0xFFFFFFFFu : (uint32_t)std::min<uint64_t>((tail_.emit_words + 1023) & ~1023ull, kEmitLdsWordsMax);
    return JPGPU_OK;
}

// the headers: one upload for the batch, put in front of the streams on the device
int EncodeBatch::place_headers(const EncodeRun &r) {
    header_bytes_.clear();
    for (int i = 0; i < r.n; i++) {
        images_[i].hdr_off = (uint32_t)header_bytes_.size();
        header_bytes_.insert(header_bytes_.end(), headers_[i].begin(), headers_[i].end());
    }
    hipError_t e = d_headers_.reserve(header_bytes_.size() + 16);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    e = tail_.upload_chunk_work(ctx_->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_images_.ptr, images_.data(), (size_t)r.n * sizeof(DevEncImage), hipMemcpyHostToDevice, ctx_->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_headers_.ptr, header_bytes_.data(), header_bytes_.size(), hipMemcpyHostToDevice, ctx_->stream);
    if (e == hipSuccess) e = launch_place_headers(ctx_->stream, (const DevEncImage *)d_images_.ptr, r.n, (const uint8_t *)d_headers_.ptr, (uint8_t *)tail_.out.ptr);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(headers)");
    return JPGPU_OK;
}

// E3 (unless the one pass has written the raw streams), E4, and the streams' lengths
int EncodeBatch::emit_and_stuff(const EncodeRun &r) {
    hipError_t e;
    if (!r.fused_emit && (e = tail_.emit(ctx_->stream, tail_source(r))) != hipSuccess) return hip_fail(e, tail_.failed);
    (void)hipEventRecord(ev_[4], ctx_->stream);
    if ((e = tail_.stuff_bytes(ctx_->stream, (const DevEncImage *)d_images_.ptr)) != hipSuccess) return hip_fail(e, tail_.failed);
    (void)hipEventRecord(ev_[5], ctx_->stream);
    e = tail_.read_lengths(ctx_->stream, r.n);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, tail_.failed);
}

int EncodeBatch::stage_ms(float ms[5]) {
    if (!encoded_ || !ev_[5]) return fail(JPGPU_ERR_INVALID_OPERATION, "jpgpu_encoder_stage_ms: no encode has run");
    const int pairs[4][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};  // (the statistics pass of optimizeCoding counts as E1)
    ms[4] = 0;
    for (int k = 0; k < 4; k++) {
        if (hipEventElapsedTime(&ms[k], ev_[pairs[k][0]], ev_[pairs[k][1]]) != hipSuccess) return fail(JPGPU_ERR_DEVICE, "hipEventElapsedTime failed");
        ms[4] += ms[k];
    }
    return JPGPU_OK;
}

int EncodeBatch::encoded_size(int i, size_t *bytes) const {
    if (i < 0 || i >= (int)images_.size() || !bytes || !encoded_) return JPGPU_ERR_ARGUMENT;
    if (status_[i] != JPGPU_OK) {
        ctx_->last_error = messages_[i];
        return status_[i];
    }
    *bytes = (size_t)tail_.h_out_len[i];
    return JPGPU_OK;
}

int EncodeBatch::download(int i, void *dst, size_t cap) {
    if (i < 0 || i >= (int)images_.size() || !dst) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_encode_download: bad argument");
    if (!encoded_) return fail(JPGPU_ERR_INVALID_OPERATION, "Nothing has been encoded yet.");
    if (status_[i] != JPGPU_OK) return fail(status_[i], messages_[i]);
    if (cap < tail_.h_out_len[i]) return fail(JPGPU_ERR_ARGUMENT, "Destination buffer is too small.");
    hipError_t e = hipMemcpy(dst, stream_of(i), (size_t)tail_.h_out_len[i], hipMemcpyDeviceToHost);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, "hipMemcpy(encoded stream)");
}

int EncodeBatch::download_coefficients(int i, int16_t *dst, size_t cap_blocks) {
    if (i < 0 || i >= (int)images_.size() || !dst) return fail(JPGPU_ERR_ARGUMENT, "bad argument");
    if (!encoded_) return fail(JPGPU_ERR_INVALID_OPERATION, "Nothing has been encoded yet.");
    if (cap_blocks < images_[i].total_blocks) return fail(JPGPU_ERR_ARGUMENT, "Destination buffer is too small.");
    const DevEncImage &im = images_[i];
    hipError_t e = hipMemcpy(dst, (const int16_t *)d_coefs_.ptr + im.coef_off * 64, (size_t)im.total_blocks * 128, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(coefficients)");
    if (im.layout != 0 && layouts_[im.layout - 1].own_blocks != 0) {
        // a described arrangement on the TransformBlocks path: blocks outside their component's grid are the allocator's dummy block
        const DevEncLayout &L = layouts_[im.layout - 1];
        for (uint32_t blk = 0; blk < im.total_blocks; blk++) {
            const uint32_t mcu = blk / im.bpm, b = blk - mcu * im.bpm, c = L.blk_comp[b];
            const uint32_t bx = (mcu % im.mcus_per_line) * L.h[c] + L.blk_x[b], by = (mcu / im.mcus_per_line) * L.v[c] + L.blk_y[b];
            if ((bx >= L.grid_w[c] || by >= L.grid_h[c]) && blk != L.dummy_blk) memcpy(dst + (size_t)blk * 64, dst + (size_t)L.dummy_blk * 64, 128);
        }
    } else if (im.table_base != 0 && im.arithmetic == JPGPU_ARITHMETIC_REFERENCE) {
        // optimizeCoding: the blocks as BuildHuffmanTables / WritePreparedScanData see them -- luma blocks outside the
        // component's own grid alias the allocator's dummy block (enc_source_block in encode_kernels.hip)
        const uint32_t ny = im.luma_h * im.luma_v, last = (im.mcus_per_line * im.mcus_per_column - 1) * im.bpm + ny - 1;
        for (uint32_t blk = 0; blk < im.total_blocks; blk++) {
            const uint32_t mcu = blk / im.bpm, b = blk - mcu * im.bpm;
            if (b >= ny) continue;
            const uint32_t bx = (mcu % im.mcus_per_line) * im.luma_h + b % im.luma_h, by = (mcu / im.mcus_per_line) * im.luma_v + b / im.luma_h;
            if (bx < (im.width + 7) / 8 && by < (im.height + 7) / 8) continue;
            if (blk != last) memcpy(dst + (size_t)blk * 64, dst + (size_t)last * 64, 128);
        }
    }
    return JPGPU_OK;
}

}  // namespace jpgpu
