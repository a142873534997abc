// jpeglibrary_amd/csrc/device_encode_progressive.cpp -- coding "progressive" of the libjpeg arithmetic (include/jpgpu.h, 4e): the scans of
// jpeg_simple_progression as units of work over the quantised blocks E1J left, the host's share of it -- the scan script, one table build per
// batch from the statistics of all scans, the segments in front of every scan -- and the order of the kernels (encode_progressive.hip).
#include <string.h>

#include <algorithm>

#include "device_encode.h"
#include "libjpeg_huffman.h"

namespace jpgpu {

namespace {
uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// jpeg_simple_progression: the component (-1: all of them, a DC scan), Ss, Se, Ah, Al
struct ScanSpec {
    int comp, ss, se, ah, al;
};
const ScanSpec kScript3[10] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {2, 1, 63, 0, 1}, {1, 1, 63, 0, 1}, {0, 6, 63, 0, 2},
                               {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}, {0, 1, 63, 1, 0}};
const ScanSpec kScript1[6] = {{-1, 0, 0, 0, 1}, {0, 1, 5, 0, 2}, {0, 6, 63, 0, 2}, {0, 1, 63, 2, 1}, {-1, 0, 0, 1, 0}, {0, 1, 63, 1, 0}};

void put_dht(std::vector<uint8_t> &h, const std::vector<uint8_t> &body) {
    put_marker(h, 0xC4);
    put_length(h, (uint16_t)body.size());
    h.insert(h.end(), body.begin(), body.end());
}
}  // namespace

void EncodeBatch::Progressive::release() {
    for (DevBuffer *b : {&d_scans, &d_work, &d_info, &d_heads, &d_bits, &d_wg_bits, &d_wg_base, &d_stats, &d_tables, &d_files, &d_streams, &d_headers, &out, &d_file_len})
        b->release();
    tail.release();
}

// The upload's share: every image's scans, their blocks' places in the per-block arrays, the work list, and what does not depend on the data
int EncodeBatch::plan_progressive() {
    Progressive &P = prog_;
    P.scans.clear();
    P.scan_image.clear();
    P.work.clear();
    P.files.assign(images_.size(), DevProgFile());
    P.max_scans = 0;
    uint64_t blk_off = 0;
    for (size_t i = 0; i < images_.size(); i++) {
        const DevEncImage &im = images_[i];
        const bool colour = im.components == 3;
        const ScanSpec *script = colour ? kScript3 : kScript1;
        const int n_scans = colour ? 10 : 6;
        P.files[i].first_scan = (uint32_t)P.scans.size();
        P.files[i].n_scans = (uint32_t)n_scans;
        P.max_scans = std::max(P.max_scans, n_scans);
        for (int k = 0; k < n_scans; k++) {
            const ScanSpec &sp = script[k];
            DevProgScan sc;
            memset(&sc, 0, sizeof sc);
            sc.coef_off = im.coef_off;
            sc.bpm = im.bpm;
            sc.ny = im.luma_h * im.luma_v;
            sc.mcus_per_line = im.mcus_per_line;
            sc.ss = (uint32_t)sp.ss;
            sc.se = (uint32_t)sp.se;
            sc.ah = (uint32_t)sp.ah;
            sc.al = (uint32_t)sp.al;
            sc.grid_w = sc.comp_h = sc.comp_v = 1;
            if (sp.ss == 0) {
                sc.n_blocks = im.total_blocks;
            } else {  // the component's own blocks: ceil(ceil(W h / H) / 8) x ceil(ceil(Ht v / V) / 8)
                const uint32_t h = sp.comp == 0 ? im.luma_h : 1u, v = sp.comp == 0 ? im.luma_v : 1u;
                const uint32_t wc = (im.width * h + im.luma_h - 1) / im.luma_h, hc = (im.height * v + im.luma_v - 1) / im.luma_v;
                sc.comp_h = h;
                sc.comp_v = v;
                sc.grid_w = (wc + 7) / 8;
                sc.n_blocks = sc.grid_w * ((hc + 7) / 8);
                sc.first_blk = sp.comp == 0 ? 0u : sc.ny + (uint32_t)sp.comp - 1u;
            }
            sc.blk_off = blk_off;
            blk_off = align_up(blk_off + sc.n_blocks, 16);  // (EP2 reads the bytes of a scan sixteen at a time)
            sc.table = 2u * (uint32_t)P.scans.size();
            sc.work_first = (uint32_t)P.work.size();
            sc.n_wg = (sc.n_blocks + 255u) / 256u;
            for (uint32_t f = 0; f < sc.n_blocks; f += 256) P.work.push_back({(uint32_t)P.scans.size(), f});
            P.scans.push_back(sc);
            P.scan_image.push_back((int)i);
        }
    }
    P.total_blocks = blk_off;
    const size_t n_scans = P.scans.size(), n_work = P.work.size();
    const DevUpload ups[] = {
        {&P.d_scans, nullptr, 0, n_scans * sizeof(DevProgScan) + 16},
        {&P.d_work, P.work.data(), n_work * sizeof(EncWork), 16},
        {&P.d_info, nullptr, 0, (size_t)blk_off + 64},
        {&P.d_heads, nullptr, 0, (size_t)blk_off * sizeof(uint16_t) + 64},
        {&P.d_bits, nullptr, 0, (size_t)blk_off * sizeof(uint32_t) + 64},
        {&P.d_wg_bits, nullptr, 0, n_work * sizeof(uint32_t) + 64},
        {&P.d_wg_base, nullptr, 0, n_work * sizeof(uint64_t) + 64},
        {&P.d_stats, nullptr, 0, n_scans * kProgStatWords * sizeof(uint32_t) + 64},
        {&P.d_tables, nullptr, 0, (2 * n_scans + 2) * sizeof(EncHuffTable)},
        {&P.d_files, nullptr, 0, P.files.size() * sizeof(DevProgFile) + 16},
        {&P.d_streams, nullptr, 0, n_scans * sizeof(DevEncImage) + 16},
        {&P.d_file_len, nullptr, 0, P.files.size() * sizeof(uint64_t) + 16},
    };
    bool copying = false;
    hipError_t e = reserve_and_copy(ups, ctx_->stream, &copying);
    if (e != hipSuccess) return hip_fail(e, copying ? "hipMemcpyAsync" : "hipMalloc");
    if ((e = P.tail.reserve(0, 0, n_scans)) != hipSuccess) return hip_fail(e, P.tail.failed);
    e = hipStreamSynchronize(ctx_->stream);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, "hipStreamSynchronize(upload)");
}

// encode() behind E1 (ev_[1] is recorded).  EP1 .. EP3 for every scan of every image, ONE copy of the statistics to the host and one table
// build for the batch -- which also gives every scan's bit count --, then EP4, EP5, the stuffing stage over the scans and the assembly.
int EncodeBatch::encode_progressive() {
    Progressive &P = prog_;
    hipStream_t stream = ctx_->stream;
    const int n_scans = (int)P.scans.size(), n_work = (int)P.work.size(), n_files = (int)P.files.size();
    const DevProgScan *d_scans = (const DevProgScan *)P.d_scans.ptr;
    const EncWork *d_work = (const EncWork *)P.d_work.ptr;
    const int16_t *coefs = (const int16_t *)d_coefs_.ptr;
    uint16_t *heads = (uint16_t *)P.d_heads.ptr;
    hipError_t e = hipMemcpyAsync(P.d_scans.ptr, P.scans.data(), (size_t)n_scans * sizeof(DevProgScan), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(P.d_heads.ptr, 0, (size_t)P.total_blocks * sizeof(uint16_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(P.d_stats.ptr, 0, (size_t)n_scans * kProgStatWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(progressive)");
    if ((e = launch_prog_classify(stream, d_scans, d_work, n_work, coefs, (uint8_t *)P.d_info.ptr)) != hipSuccess) return hip_fail(e, "prog_classify_kernel");
    if ((e = launch_prog_runs(stream, d_scans, d_work, n_work, (const uint8_t *)P.d_info.ptr, heads)) != hipSuccess) return hip_fail(e, "prog_runs_kernel");
    if ((e = launch_prog_stats(stream, d_scans, d_work, n_work, coefs, heads, (uint32_t *)P.d_stats.ptr)) != hipSuccess) return hip_fail(e, "prog_stats_kernel");
    (void)hipEventRecord(ev_[2], stream);
    std::vector<uint32_t> stats((size_t)n_scans * kProgStatWords);
    e = hipMemcpyAsync(stats.data(), P.d_stats.ptr, stats.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(statistics)");

    // per scan: its tables, the segments in front of it, its bit count; per image: the frame header (set_quantization_table may have changed it)
    std::vector<EncHuffTable> tables(2 * (size_t)n_scans);
    memset(tables.data(), 0, tables.size() * sizeof(EncHuffTable));
    P.streams.assign((size_t)n_scans, DevEncImage());
    P.headers.clear();
    P.tail.h_raw_bits.assign((size_t)n_scans, 0);
    for (int i = 0; i < n_files; i++) {
        P.files[i].hdr_off = (uint32_t)P.headers.size();
        P.files[i].hdr_len = (uint32_t)headers_[i].size();
        P.headers.insert(P.headers.end(), headers_[i].begin(), headers_[i].end());
    }
    for (int s = 0; s < n_scans; s++) {
        const DevEncImage &im = images_[(size_t)P.scan_image[s]];
        const ScanSpec &sp = (im.components == 3 ? kScript3 : kScript1)[s - (int)P.files[(size_t)P.scan_image[s]].first_scan];
        const uint32_t *st = &stats[(size_t)s * kProgStatWords];
        std::vector<uint8_t> h, body;
        uint64_t bits = (uint64_t)st[512] | ((uint64_t)st[513] << 32);
        const int n_tables = sp.ah != 0 && sp.ss == 0 ? 0 : (sp.ss == 0 && im.components == 3 ? 2 : 1);
        for (int t = 0; t < n_tables; t++) {
            const int ident = sp.ss == 0 ? t : (sp.comp == 0 ? 0 : 1);
            EncHuffTable &tab = tables[2 * (size_t)s + (size_t)t];
            libjpeg_build_table(st + t * 256, (uint8_t)(((sp.ss != 0 ? 1 : 0) << 4) | ident), &tab, &body);
            put_dht(h, body);
            for (int y = 0; y < 256; y++) bits += (uint64_t)st[t * 256 + y] * tab.len[y];
        }
        const int first = sp.comp < 0 ? 0 : sp.comp, last = sp.comp < 0 ? (int)im.components - 1 : sp.comp;
        put_marker(h, 0xDA);
        put_length(h, (uint16_t)(1 + 2 * (last - first + 1) + 3));
        h.push_back((uint8_t)(last - first + 1));
        for (int c = first; c <= last; c++) {
            const int t = c == 0 ? 0 : 1;
            h.push_back((uint8_t)(c + 1));
            h.push_back((uint8_t)(sp.ss != 0 ? t : (sp.ah != 0 ? 0 : t << 4)));  // (a DC refinement scan names no table)
        }
        h.push_back((uint8_t)sp.ss);
        h.push_back((uint8_t)sp.se);
        h.push_back((uint8_t)((sp.ah << 4) | sp.al));
        DevEncImage &stream_desc = P.streams[(size_t)s];
        memset(&stream_desc, 0, sizeof stream_desc);
        stream_desc.hdr_off = (uint32_t)P.headers.size();
        stream_desc.header_len = (uint32_t)h.size();
        stream_desc.n_units = 1;
        P.headers.insert(P.headers.end(), h.begin(), h.end());
        P.tail.h_raw_bits[(size_t)s] = bits;
    }
    // the stuffing stage's layout over the scans: raw bytes, staged streams (segments + 2 x raw bytes + EOI at most), chunks
    e = hipMemcpyAsync(P.tail.raw_bits.ptr, P.tail.h_raw_bits.data(), (size_t)n_scans * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(bit counts)");
    if ((e = P.tail.plan(stream, P.streams.data(), n_scans, true)) != hipSuccess) return hip_fail(e, P.tail.failed);
    // the files (include/jpgpu.h 4e, "Output reservation"): the frame header + per scan its segments and 2 x ceil(bits / 8) + EOI at most;
    // 64 bytes of slack, every file 256-byte aligned
    uint64_t out_bytes = 0;
    for (int i = 0; i < n_files; i++) {
        DevProgFile &f = P.files[(size_t)i];
        f.dst_off = out_bytes;
        uint64_t worst = f.hdr_len + 2;
        for (uint32_t k = 0; k < f.n_scans; k++) {
            const size_t s = f.first_scan + k;
            P.scans[s].raw_off = P.streams[s].raw_off;
            P.scans[s].raw_bits = P.tail.h_raw_bits[s];
            worst += P.streams[s].header_len + 2 * ((P.tail.h_raw_bits[s] + 7) / 8);
        }
        out_bytes = align_up(out_bytes + worst + 64, 256);
    }
    const DevUpload ups[] = {
        {&P.d_scans, P.scans.data(), (size_t)n_scans * sizeof(DevProgScan), 0},
        {&P.d_streams, P.streams.data(), (size_t)n_scans * sizeof(DevEncImage), 0},
        {&P.d_files, P.files.data(), (size_t)n_files * sizeof(DevProgFile), 0},
        {&P.d_tables, tables.data(), tables.size() * sizeof(EncHuffTable), 0},
        {&P.d_headers, P.headers.data(), P.headers.size(), 16},
        {&P.out, nullptr, 0, (size_t)out_bytes + 256},
    };
    bool copying = false;
    if ((e = reserve_and_copy(ups, stream, &copying)) != hipSuccess) return hip_fail(e, copying ? "hipMemcpyAsync" : "hipMalloc");
    if ((e = P.tail.upload_chunk_work(stream)) != hipSuccess) return hip_fail(e, P.tail.failed);
    const DevEncImage *d_streams = (const DevEncImage *)P.d_streams.ptr;
    if ((e = launch_place_headers(stream, d_streams, n_scans, (const uint8_t *)P.d_headers.ptr, (uint8_t *)P.tail.out.ptr)) != hipSuccess)
        return hip_fail(e, "place_headers_kernel");
    (void)hipEventRecord(ev_[3], stream);
    const EncHuffTable *d_tables = (const EncHuffTable *)P.d_tables.ptr;
    e = launch_prog_bits(stream, d_scans, n_scans, d_work, n_work, d_tables, coefs, heads, (uint32_t *)P.d_bits.ptr, (uint32_t *)P.d_wg_bits.ptr,
                         (uint64_t *)P.d_wg_base.ptr);
    if (e != hipSuccess) return hip_fail(e, "prog_bits_kernel");
    e = launch_prog_emit(stream, d_scans, d_work, n_work, d_tables, coefs, heads, (const uint32_t *)P.d_bits.ptr, (const uint64_t *)P.d_wg_base.ptr,
                         (uint8_t *)P.tail.raw.ptr);
    if (e != hipSuccess) return hip_fail(e, "prog_emit_kernel");
    (void)hipEventRecord(ev_[4], stream);
    if ((e = P.tail.stuff_bytes(stream, d_streams)) != hipSuccess) return hip_fail(e, P.tail.failed);
    e = launch_prog_assemble(stream, (const DevProgFile *)P.d_files.ptr, n_files, P.max_scans, d_streams, (const uint64_t *)P.tail.out_len.ptr,
                             (const uint8_t *)P.d_headers.ptr, (const uint8_t *)P.tail.out.ptr, (uint8_t *)P.out.ptr, (uint64_t *)P.d_file_len.ptr);
    if (e != hipSuccess) return hip_fail(e, "prog_assemble_kernel");
    (void)hipEventRecord(ev_[5], stream);
    tail_.h_out_len.assign((size_t)n_files, 0);
    e = hipMemcpyAsync(tail_.h_out_len.data(), P.d_file_len.ptr, (size_t)n_files * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(stream lengths)");
    encoded_ = true;
    return JPGPU_OK;
}

}  // namespace jpgpu
