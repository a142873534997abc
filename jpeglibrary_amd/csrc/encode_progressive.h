// jpeglibrary_amd/csrc/encode_progressive.h -- device structures and launch wrappers of the progressive entropy coder
// (encode_progressive.hip): libjpeg's jcphuff.c over quantised blocks in the encoder's coefficient layout (include/jpgpu.h, 4e)
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "encode_kernels.h"

namespace jpgpu {

// One scan of one image: the unit of work.  A DC scan (ss == 0) visits the blocks in the coefficient buffer's own order (MCU order, dummy
// blocks included; one component: its blocks in raster order, which is the same thing).  An AC scan visits the REAL blocks of its one
// component, grid_w x grid_h in raster order: block (bx, by) lies in MCU (by / comp_v) * mcus_per_line + bx / comp_h at first_blk +
// (by % comp_v) * comp_h + bx % comp_h.
struct alignas(16) DevProgScan {
    uint64_t coef_off;    // the image's first block in the coefficient buffer
    uint64_t blk_off;     // the scan's first entry in the per-block arrays (info, run heads, bit offsets)
    uint64_t raw_off;     // its raw (unstuffed) bytes in the raw buffer, 256-byte aligned
    uint64_t raw_bits;    // ... and how many bits they hold (from the statistics: the host knows before anything is written)
    uint32_t n_blocks;    // blocks the scan visits
    uint32_t grid_w;      // AC: blocks per row of the component
    uint32_t comp_h, comp_v, first_blk;
    uint32_t bpm, ny, mcus_per_line;
    uint32_t ss, se, ah, al;
    uint32_t table;       // first of the scan's tables (DC: table 0 for luma, 1 for chroma; AC: one) in the table array
    uint32_t work_first;  // first of its workgroups (256 blocks each) in the work list
    uint32_t n_wg;
    uint32_t reserved;
};
static_assert(sizeof(DevProgScan) % 16 == 0, "DevProgScan must be a multiple of 16 bytes");

// Per scan: two histograms of 256 counters (a DC scan's DC0 and DC1; an AC scan uses the first), then the bits that are not
// Huffman codes as one 64-bit count -- 514 words
constexpr uint32_t kProgStatWords = 2 * 256 + 2;
// The deferred correction bits a run may hold before it is flushed (jcphuff.c: MAX_CORR_BITS 1000 less the 63 a block can add)
constexpr uint32_t kProgMaxDeferred = 937;
constexpr uint32_t kProgMaxRun = 0x7FFF;

// EP1: per block of every AC scan one byte: bit 7 the block ends the run in front of it (it codes a coefficient), bit 6 it extends or
// starts a run behind what it codes, bits 0-5 the correction bits it defers into that run (refinement scans)
hipError_t launch_prog_classify(hipStream_t stream, const DevProgScan *scans, const EncWork *work, int n_work, const int16_t *coefs, uint8_t *info);
// EP2: the EOB runs, resolved by the lane of every block that starts one: heads[b] = the length of the run piece that is coded in
// front of block b's deferred bits (0: none).  heads must be zero on entry.
hipError_t launch_prog_runs(hipStream_t stream, const DevProgScan *scans, const EncWork *work, int n_work, const uint8_t *info, uint16_t *heads);
// EP3: the symbols of every scan counted into stats[scan] (zero on entry)
hipError_t launch_prog_stats(hipStream_t stream, const DevProgScan *scans, const EncWork *work, int n_work, const int16_t *coefs, const uint16_t *heads,
                             uint32_t *stats);
// EP4: bits of every block with the tables built from the statistics (offset inside its workgroup -> bits, the workgroup's total ->
// wg_bits), and the workgroups' bases (one workgroup per scan)
hipError_t launch_prog_bits(hipStream_t stream, const DevProgScan *scans, int n_scans, const EncWork *work, int n_work, const EncHuffTable *tables,
                            const int16_t *coefs, const uint16_t *heads, uint32_t *bits, uint32_t *wg_bits, uint64_t *wg_base);
// EP5: the codes ORed into the zeroed raw buffer, the last block of a scan padding its last byte with one-bits
hipError_t launch_prog_emit(hipStream_t stream, const DevProgScan *scans, const EncWork *work, int n_work, const EncHuffTable *tables, const int16_t *coefs,
                            const uint16_t *heads, const uint32_t *bits, const uint64_t *wg_base, uint8_t *raw);

// EP6: the file: image i's header, then of each of its scans what the stuffing stage wrote (DHT segments, SOS, the stuffed bytes)
// less the EOI it closed them with, then EOI.  scan_streams[s] = the scan's descriptor in the stuffing stage's form (out_off), scan_len
// what that stage reported; files[i] = {first scan, scans, header offset in `headers`, header length}, dst_off[i] where the file goes.
struct DevProgFile {
    uint64_t dst_off;
    uint32_t first_scan, n_scans, hdr_off, hdr_len;
};
hipError_t launch_prog_assemble(hipStream_t stream, const DevProgFile *files, int n_files, int max_scans, const DevEncImage *scan_streams,
                                const uint64_t *scan_len, const uint8_t *headers, const uint8_t *staged, uint8_t *out, uint64_t *file_len);

}  // namespace jpgpu
