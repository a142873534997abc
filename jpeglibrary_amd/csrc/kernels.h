// jpeglibrary_amd/csrc/kernels.h -- launch wrappers of the HIP kernels (internal C++ API of libjpgpu.so)
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "common.h"

namespace jpgpu {

constexpr int kHuffWaves = 11;                // wavefronts per Huffman workgroup at most (what the standard four tables leave room for)
// LDS of the K2 family (k2_huffman.hip, the K2S final pass): the scan's staged tables -- u32 first levels that carry values and
// pairs, round 6: an AC table 2^11 entries, a DC table 2^9, + second level, header and the reference's arrays each -- then
// kK2WaveLdsBytes per wave (64 staged blocks + 64 stream rings) and the block info.
constexpr uint32_t kK2AcTabBytes = 8192 + 512 + 16 + 320, kK2DcTabBytes = 2048 + 512 + 16 + 320, kK2WaveLdsBytes = 8192 + 64 * 68;
constexpr uint32_t kK2LdsBudget = 160 * 1024 - 64;
inline uint32_t k2_scan_tab_bytes(const DevScan &s) {  // a DC table = one that some component decodes its DC symbols with
    uint32_t bytes = 0;
    for (int sl = 0; sl < kMaxHuffSlots; sl++) {
        if (s.huff_pool[sl] == 0xFFFF) continue;
        bool is_dc = false;
        for (int c = 0; c < s.scan_components; c++) is_dc |= s.comp[c].dc_slot == sl;
        bytes += is_dc ? kK2DcTabBytes : kK2AcTabBytes;
    }
    return bytes;
}
// waves per K2 workgroup for a batch whose largest table set takes tab_bytes (eight AC tables still leave seven)
constexpr int huffman_waves(uint32_t tab_bytes) {
    return (int)((kK2LdsBudget - tab_bytes) / kK2WaveLdsBytes) < kHuffWaves ? (int)((kK2LdsBudget - tab_bytes) / kK2WaveLdsBytes) : kHuffWaves;
}
// restart intervals per Huffman workgroup (one per lane): 64 * huffman_waves(table slots of the batch)
constexpr int kIdctBlocksPerWg = 256;         // 8x8 blocks per IDCT tile (one per lane)
constexpr int kIdctTilesPerWg = 16;           // consecutive tiles walked by one IDCT workgroup (prefetch pipeline)


constexpr uint32_t kMarkerChunkBytes = 4096;  // K1 chunk size (256 lanes x 16 bytes)
// consecutive chunks of one scan handled by one K1 workgroup (one work-list entry).  4 was measured in round 2: K1 1.53 ms
// instead of 1.27-1.35 per 1024 x 4K -- the quarter of a million small workgroups are not what K1 waits for, and chunks taken
// one after the other inside a workgroup hide less latency than the same chunks in separate workgroups
constexpr uint32_t kMarkerChunksPerWg = 1;  // marker_count_kernel takes several work entries per workgroup and relies on 1 here
hipError_t launch_marker_index(hipStream_t stream, const uint8_t *data, const DevScan *scans, int n_scans, const ChunkWork *work,
                               int n_chunks, ChunkSum *sums, uint32_t *ends, DevScanStatus *status, uint8_t *udata, uint32_t *ends_u);
// K1 in one pass (k1_markers.hip): desc = kMarkerDescBytes per chunk (cleared when allocated; a group uses its first chunk's),
// tickets[0] = the ticket counter (cleared once per upload; read by -DJPGPU_K1_TICKETS builds only since round 6: a group takes its place
// in `order` from its workgroup index), epoch = decodes of this upload issued before this one, tag = a non-zero
// number no earlier launch over `desc` has used; spin_budget = polls a workgroup may spend waiting for a predecessor before it counts
// the chunks in front of its group itself -- *host_giveup (page-locked host memory) != 0 afterwards says that happened (the results
// are complete either way).
constexpr size_t kMarkerDescBytes = 64;
#ifndef JPGPU_K1_GROUP
#define JPGPU_K1_GROUP 4
#endif
constexpr uint32_t kMarkerGroupChunks = JPGPU_K1_GROUP;  // chunks a workgroup of the one-pass index takes; `order`: (scan, first chunk) per group, by (group, scan)
hipError_t launch_marker_onepass(hipStream_t stream, const uint8_t *data, const DevScan *scans, const ChunkWork *order, int n_groups,
                                 void *desc, uint32_t *tickets, uint32_t epoch, uint32_t tag, uint32_t spin_budget,
                                 uint32_t *host_giveup, uint32_t *ends, DevScanStatus *status, uint8_t *udata, uint32_t *ends_u);
hipError_t launch_huffman(hipStream_t stream, const uint8_t *data, const DevScan *scans, const HuffWork *work, int n_work,
                          const uint32_t *ends, DevScanStatus *status, const DevHuffTable *huff_pool, int16_t *coefs,
                          int n_slots, const uint8_t *lut_pool, uint32_t tab_bytes);
// One pooled run of K2 (huffman_pool_kernel): `work` = its n_chunks entries (scan, first interval) of 64 intervals each, all staging the
// same tables; `groups` workgroups of huffman_waves(tab_bytes) waves each draw from *counter, which is never cleared: the launch takes
// n_chunks + groups * waves tickets, the first of them ticket_base (the sum of the earlier launches' draws).
constexpr int kK2MaxPools = 8;
hipError_t launch_huffman_pool(hipStream_t stream, const uint8_t *data, const DevScan *scans, const HuffWork *work, int n_chunks, uint32_t *counter,
                               uint32_t ticket_base, int groups, const uint32_t *ends, DevScanStatus *status, int16_t *coefs, int n_slots,
                               const uint8_t *lut_pool, uint32_t tab_bytes);
// lut_pool: kLutPoolBytesPerTable per pool table, filled by launch_lut_pool (K2 and the K2S round kernel copy from it)
hipError_t launch_lut_pool(hipStream_t stream, const DevHuffTable *huff_pool, int n_tables, uint8_t *lut_pool);
// Output layout classes of the formats K3 assembles from whole pixels (chosen per scan on the host, see idct_layout_class()): the layouts the
// kernels are instantiated with, and the class of frames whose generic Dispose() pass has run (any format): flush_output_kernel
enum IdctLayout : int { kLayGeneric = 0, kLayYccH1V1 = 1, kLayYccH2V1 = 2, kLayYccH2V2 = 3, kLayGray = 4, kNumIdctLayouts = 5, kIdctClassStoreHoldsSamples = 5 };
constexpr int kNumIdctLayoutClasses = 6;
// Output layout class of a scan for the formats K3 assembles from whole pixels (fmt_is_interleaved; 0 = generic bytewise path, else a specialised kernel).
int idct_layout_class(const DevScan &s);
// Has K3 a form that reads half-line planes (idct_split_kernel) for this output format and layout class?  Not where the output assembly
// of the dense form already takes every register the occupancy allows -- the bytewise generic layout of the interleaved formats, RGB_U8
// from 4:2:2 / 4:2:0, RGBA_U8 from 4:2:0, the scaled sink's gray layout -- the flag bytes held across it would go to scratch: those
// scans stay dense.
constexpr bool idct_split_supported(int format, int layout_class) {
    if (format == kFmtPlanarI16 || format == kFmtPlanarU8 || format == kFmtExtendedU16) return true;
    if (layout_class == kLayGeneric || layout_class >= kIdctClassStoreHoldsSamples) return false;
    if (format == kFmtRgbU8) return layout_class == kLayYccH1V1 || layout_class == kLayGray;
    if (format == kFmtRgbaU8) return layout_class != kLayYccH2V2;
    if (format == kFmtRgbPlanarU8) return true;  // all four fast classes compile at the kernel's launch bounds without spill or scratch (tests/test_planar_rgb_isa_cpu.py)
    // RGB_PLANAR_F16 / _F32, by the compiler's resource report for gfx950: every class fits in both forms without a spilled vector register and
    // without scratch -- dense: 4:4:4, 4:2:2, 4:2:0 162 VGPRs, gray 160; split: 4:4:4 163, 4:2:2 164, 4:2:0 163, gray 163 (of the 168 three waves
    // per SIMD allow).  The split forms have no scalar register left for the six constants: ten scalars (gray: five) wait in lanes of one vector
    // register, moved once per tile outside the task loop (tests/test_float_sink_isa_cpu.py).
    if (format == kFmtRgbPlanarF16 || format == kFmtRgbPlanarF32) return true;
    if (format == kFmtInterleavedU8Scaled) return layout_class != kLayGray;
    return true;
}
// THE rule of K3's kernel variants: which kernel serves work of (output format, layout class) in a form -- dense coefficient blocks, blocks
// handed over as half-line planes, or the work of a windowed image -- and where it writes.  The planner (device_batch_layout.cpp), the launcher
// and the set of kernels the launcher instantiates (k3_idct.hip: launch_k3_variant) all ask here, and tests/test_k3_variants_cpu.py holds the
// whole table: a new sink, class or form is added HERE, and its kernel follows.
enum K3Form : int { kK3Dense = 0, kK3Split = 1, kK3Window = 2, kNumK3Forms = 3 };
struct K3Variant {
    bool exists;      // no kernel: the planner must not list such work, the launcher refuses it
    bool pre;         // the store already holds samples: flush_output_kernel<fmt> / flush_window_kernel<fmt> (lay is kLayGeneric)
    int fmt, lay;     // idct_output_kernel / idct_split_kernel / idct_window_kernel<fmt, lay>
    bool to_scratch;  // INTERLEAVED_U8 samples into the RGB formats' scratch image (`generic_out`), converted behind K3
};
constexpr K3Variant k3_variant(int format, int layout_class, int form) {
    constexpr K3Variant none = {false, false, 0, 0, false};
    if (format < 0 || format >= kNumOutputFormats || layout_class < 0 || layout_class >= kNumIdctLayoutClasses) return none;
    if (format == kFmtExtendedU16) format = kFmtPlanarI16;  // (extend_u16_kernel widens PLANAR_I16 planes: run_idct launches under that number)
    const bool rgb = fmt_is_rgb(format);
    if (form == kK3Window) {  // whole-pixel formats only; sample bytes from the generic layout, fused conversion for RGB_U8 and the three planar sinks
        if (!fmt_is_interleaved(format)) return none;
        const int bytes = format == kFmtInterleavedU8Scaled ? kFmtInterleavedU8Scaled : kFmtInterleavedU8;
        if (layout_class == kIdctClassStoreHoldsSamples) return {true, true, bytes, kLayGeneric, rgb};
        if (layout_class == kLayGeneric) return {true, false, bytes, kLayGeneric, rgb};
        if (format == kFmtRgbU8 || fmt_is_rgb_planes(format)) return {true, false, format, layout_class, false};
        return none;
    }
    if (form != kK3Dense && form != kK3Split) return none;
    if (layout_class == kIdctClassStoreHoldsSamples) {  // the generic Dispose() pass has run: the store goes to the writer as it is (never split)
        const bool own = format == kFmtPlanarI16 || format == kFmtPlanarU8 || format == kFmtInterleavedU8Scaled;
        return form == kK3Dense ? K3Variant{true, true, own ? format : kFmtInterleavedU8, kLayGeneric, rgb} : none;
    }
    if (form == kK3Split && !idct_split_supported(format, layout_class)) return none;
    if (format == kFmtPlanarI16 || format == kFmtPlanarU8) return {true, false, format, kLayGeneric, false};  // planes: no layout class
    // RGB formats without a fused path: the samples go to the scratch image as INTERLEAVED_U8 and are converted by launch_ycc_to_rgb
    if (rgb && layout_class == kLayGeneric) return {true, false, kFmtInterleavedU8, kLayGeneric, true};
    return {true, false, format, layout_class, false};
}
// Is kernel <fmt, lay> of a form (pre: its flush kernel) one the rule reaches from some (format, class)?  Exactly those are compiled.
constexpr bool k3_variant_compiled(int form, bool pre, int fmt, int lay) {
    for (int f = 0; f < kNumOutputFormats; f++)
        for (int c = 0; c < kNumIdctLayoutClasses; c++) {
            const K3Variant v = k3_variant(f, c, form);
            if (v.exists && v.pre == pre && v.fmt == fmt && v.lay == lay) return true;
        }
    return false;
}
// work is sorted by layout class; class_begin[c]..class_begin[c+1] are the workgroups of class c.
// RGB / RGBA formats: classes with a fused conversion write `out`; the generic class writes INTERLEAVED_U8 samples into
// `generic_out` (same offsets), to be converted by launch_ycc_to_rgb (bpp = 3 / 4, or 1: the three planes of RGB_PLANAR_U8 / _F16 / _F32).
// aff: the affine step of RGB_PLANAR_F16 / _F32 (no other format reads it).  Work of a class k3_variant has no kernel for: hipErrorInvalidValue.
hipError_t launch_idct(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const IdctWork *work,
                       const int class_begin[kNumIdctLayoutClasses + 1], const DevScanStatus *status,
                       const DevQuantTable *quant_pool, uint8_t *out, int format, const YccRgbFactors &kf, uint8_t *generic_out,
                       const int *split_begin = nullptr, const OutputAffine &aff = kOutputAffineIdentity);
// The work of windowed images (DevScan::win_*, cov_*; IdctWork counts MCUs of the window's cover): the same lists by class, the class given by
// idct_window_layout_class, never split.  Whole-pixel formats only.
int idct_window_layout_class(const DevScan &s, int format);
hipError_t launch_idct_window(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const IdctWork *work,
                              const int class_begin[kNumIdctLayoutClasses + 1], const DevScanStatus *status, const DevQuantTable *quant_pool, uint8_t *out,
                              int format, const YccRgbFactors &kf, uint8_t *generic_out, const OutputAffine &aff = kOutputAffineIdentity);
// a scan K2 handed over as half-line planes (common.h: kScanSplitHandoff) -> dense int16[blocks][64] at the same offsets of `dense`
hipError_t launch_expand_handoff(hipStream_t stream, const int16_t *coefs, int16_t *dense, const DevScan *scans, const uint32_t *scan_ids, int n_scans,
                                 uint32_t max_blocks);
// the reference's Dispose() taken literally (frames whose component slots do not map one to one onto their components)
hipError_t launch_dispose_pass(hipStream_t stream, int16_t *coefs, const DisposeJob *jobs, int n_jobs, uint32_t max_blocks, const DevQuantTable *quant_pool);
hipError_t launch_ycc_to_rgb(hipStream_t stream, const uint8_t *src, uint8_t *dst, uint64_t n_pixels, int comps, int bpp, const YccRgbFactors &kf,
                             int sample_bytes = 1, const OutputAffine &aff = kOutputAffineIdentity);
// K3C (k3c_color.hip): the images of kind RGB, CMYK and YCCK (JPGPU_COLOR_FILE) from the INTERLEAVED_U8 samples K3's generic class left in
// `scratch` to the batch's RGB format in `out` -- ONE launch for all of them, a descriptor per image.  src_off and dst_off are multiples of
// 256; the scratch slot holds pixels * (kind == kColorRgb ? 3 : 4) bytes, the output pixels * 3 (RGBA_U8: 4) samples.  max_pixels: the
// largest `pixels` among the descriptors.  aff: the affine step of RGB_PLANAR_F16 / _F32.
struct ColorImage {
    uint64_t src_off, dst_off;  // bytes into `scratch` / `out`
    uint64_t pixels;            // of the image, or of its window
    uint32_t kind;              // ColorKind: kColorRgb, kColorCmyk or kColorYcck
    uint32_t reserved;
};
hipError_t launch_color_convert(hipStream_t stream, const uint8_t *scratch, uint8_t *out, const ColorImage *images, int n_images, uint64_t max_pixels,
                                int format, const YccRgbFactors &kf, const OutputAffine &aff);
// K3O (k3o_orient.hip): the images whose orientation is not 1 (include/jpgpu.h, "Orientation"), of every colour kind, from the INTERLEAVED_U8
// samples K3's generic class left in `scratch` -- `width` x `height` pixels of the STORED frame (the image's window there), 1, 3 or 4 bytes
// each by kind, tight -- to the batch's RGB format in `out`, turned: ONE launch for all of them, a descriptor per image, a workgroup per
// tile of kOrientTile x kOrientTile source pixels.  src_off and dst_off are multiples of 256; `out` and `scratch` are different buffers.
// max_tiles: the largest orient_tiles(width, height) among the descriptors.
constexpr uint32_t kOrientTile = 64;
constexpr uint32_t orient_tiles(uint32_t width, uint32_t height) { return ((width + kOrientTile - 1) / kOrientTile) * ((height + kOrientTile - 1) / kOrientTile); }
struct OrientImage {
    uint64_t src_off, dst_off;  // bytes into `scratch` / `out`
    uint32_t width, height;     // of the stored window
    uint32_t kind;              // ColorKind
    uint32_t orientation;       // 2..8
};
hipError_t launch_orient_convert(hipStream_t stream, const uint8_t *scratch, uint8_t *out, const OrientImage *images, int n_images, uint32_t max_tiles,
                                 int format, const YccRgbFactors &kf, const OutputAffine &aff);
// K3U (k3u_upsample.hip): the images that are filtered under JPGPU_UPSAMPLE_FANCY (include/jpgpu.h, "Chroma upsampling"; k3u_taps.h has the
// arithmetic), from the INTERLEAVED_U8 samples K3's generic class left in `scratch` -- the FETCH RECTANGLE of the stored frame, fetch_w
// pixels per line of 3 bytes, whose first pixel is (fetch_x, fetch_y) of the frame: the stored window widened so that every tap is there.
// The window's pixels go to the batch's RGB format at `out` + dst_off (staged == 0), or, for an image K3O turns afterwards, as (Y, Cb', Cr')
// of 3 bytes per pixel to `staging` + dst_off (staged == 1: the sixth sink; `staging` is the scratch buffer, behind the image's fetch
// rectangle).  ONE call for all of them, a descriptor per image, a workgroup per tile of kFancyTileW x kFancyTileH pixels of the window.
// src_off and dst_off are multiples of 256.  max_tiles: the largest fancy_tiles(win_w, win_h) among the descriptors.
constexpr uint32_t kFancyTileW = 128, kFancyTileH = 16;
constexpr uint32_t fancy_tiles(uint32_t width, uint32_t height) { return ((width + kFancyTileW - 1) / kFancyTileW) * ((height + kFancyTileH - 1) / kFancyTileH); }
struct FancyImage {
    uint64_t src_off, dst_off;             // bytes into `scratch` / into `out` or `staging`
    uint32_t fetch_x, fetch_y, fetch_w;    // the fetch rectangle's first pixel in the frame, and its pixels per line
    uint32_t win_x, win_y, win_w, win_h;   // the stored window, in pixels of the frame
    uint32_t cw, ch;                       // the chroma plane's REAL extent: ceil(W / hs) x ceil(H / vs)
    uint32_t hs, vs;                       // (2, 1), (2, 2) or (1, 2)
    uint32_t staged;
};
hipError_t launch_fancy_upsample(hipStream_t stream, const uint8_t *scratch, uint8_t *out, uint8_t *staging, const FancyImage *images, int n_images,
                                 int n_staged, uint32_t max_tiles, int format, const YccRgbFactors &kf, const OutputAffine &aff);
// K3Y (k3y_luma.hip): the images decoded to ONE plane under JPGPU_CHANNELS_LUMA (include/jpgpu.h, "Grey output"), on their two roads.
// The fast road, luma_idct_kernel: component 0's blocks of a scan, straight from the dense coefficient store to the plane at `out` +
// DevScan::out_off, pitch win_w samples.  The luma blocks of the window's MCU cover form a grid of cov_cols * h x cov_rows * v blocks (h, v:
// component 0's factors: the frame's maxima, or v = 1 under a taller MCU, whose sample rows are repeated vs times); a UNIT is kLumaUnitBlocks neighbouring blocks of one row of that grid, one wave's work; a
// workgroup takes `n_units` (1..kLumaUnitsPerWg) consecutive units, the first being chunk `chunk` of block row `row`, the next ones following
// in raster order.  ONE launch for all listed scans.  Component 0 is the scan's first component and its blocks are slots 0 .. h * v - 1 of
// the MCU in raster order (DeviceBatch::luma_fast checks both).  windowed: a listed scan's win_* / cov_* differ from the whole frame's.
constexpr uint32_t kLumaUnitBlocks = 64, kLumaUnitsPerWg = 4;
struct LumaWork {
    uint32_t scan;
    uint32_t row, chunk;  // the first unit: block row of the cover's luma grid, chunk of kLumaUnitBlocks blocks in it
    uint32_t n_units;
};
hipError_t launch_luma_idct(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const LumaWork *work, int n_work, bool windowed,
                            const DevScanStatus *status, const DevQuantTable *quant_pool, uint8_t *out, int format, const OutputAffine &aff);
// The scratch road, luma_plane_kernel: from the INTERLEAVED_U8 samples K3's generic class left in `scratch` -- `width` x `height` pixels of
// the STORED frame (the image's window there), 1, 3 or 4 bytes each by kind, tight -- to the one plane in `out`, turned by `orientation`
// (1..8) like K3O turns: ONE launch for all of them, a descriptor per image, a workgroup per tile of kOrientTile x kOrientTile source pixels.
// The sample is byte 0 for the kinds GRAY and YCBCR, L = (19595 R + 38470 G + 7471 B + 32768) >> 16 of K3C's pixel for RGB, CMYK and YCCK.
// src_off and dst_off are multiples of 256; max_tiles: the largest orient_tiles(width, height) among the descriptors.
struct LumaImage {
    uint64_t src_off, dst_off;  // bytes into `scratch` / `out`
    uint32_t width, height;     // of the stored window
    uint32_t kind;              // ColorKind
    uint32_t orientation;       // 1..8
};
hipError_t launch_luma_plane(hipStream_t stream, const uint8_t *scratch, uint8_t *out, const LumaImage *images, int n_images, uint32_t max_tiles,
                             int format, const YccRgbFactors &kf, const OutputAffine &aff);
// K3J (k3j_islow.hip): the images that take libjpeg's integer transform under JPGPU_ARITHMETIC_LIBJPEG (include/jpgpu.h, "Arithmetic";
// k3j_islow.h has the block transform), from the dense coefficient store to the INTERLEAVED_U8 samples of the image's scratch slot, at
// `scratch` + DevScan::out_off -- exactly where K3's generic class puts them, replication and clip to win_* included -- so that K3C, K3U,
// K3O, K3Y's luma_plane_kernel and K4 run behind it unchanged.  A lane is one block of ANY component; a workgroup takes the blocks of up to
// kIslowThreads / blocks_per_mcu consecutive MCUs of MCU row `row` of the window's MCU cover, from block `first` of that row (a multiple of
// blocks_per_mcu: MCU first / bpm): contiguous in the store, and whole MCUs, so that the workgroup can lay its strip of pixels out in LDS and
// store it row by row.  ONE launch for all listed scans, of whole frames and of windows (cov_* is the whole grid without one).
// DeviceBatch::islow_taken says which images: no scan of theirs overlaps another or names a component twice, every replication is by 1, 2 or 4.
constexpr uint32_t kIslowThreads = 256;
JPGPU_HD constexpr uint32_t islow_blocks_per_wg(uint32_t blocks_per_mcu) { return kIslowThreads / blocks_per_mcu * blocks_per_mcu; }
struct IslowWork {
    uint32_t scan;
    uint32_t row;    // MCU row of the cover
    uint32_t first;  // first block of the workgroup in that row of cov_cols * blocks_per_mcu blocks
    uint32_t pad;
};
hipError_t launch_islow(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const IslowWork *work, int n_work, const DevScanStatus *status,
                        const DevQuantTable *quant_pool, uint8_t *scratch);
// K3R (k3r_reduced.hip): the images of K3J's kind that are decoded at 1/2, 1/4 or 1/8 size (include/jpgpu.h, "Scaled decode"; k3r_reduced.h
// has the block transforms and the per-component rule).  K3J's work division and scratch slot; `m` = 8 / denom is all the kernel needs beyond
// the scan: a component's transform size and residual replication follow from it and the sampling factors.  The DevScan of such an image
// carries win_* in pixels and cov_* in MCUs of the REDUCED picture (an MCU is m * max_h x m * max_v pixels of it); no other kernel reads them
// for it.  ONE launch for all listed scans, behind K3J's.
struct ReducedWork {
    uint32_t scan;
    uint32_t row;    // MCU row of the cover
    uint32_t first;  // first block of the workgroup in that row of cov_cols * blocks_per_mcu blocks
    uint32_t m;      // 4, 2 or 1
};
hipError_t launch_reduced(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const ReducedWork *work, int n_work, const DevScanStatus *status,
                          const DevQuantTable *quant_pool, uint8_t *scratch);

// Waves per workgroup of the POOLED form of the K2S final pass (k2s_subseq.hip: runs of scans that stage the same tables; one workgroup per CU, every wave takes the
// next 64 lanes from a counter): 10 waves + 4 tables fill a CU's LDS.  Runs shorter than kSubFinalPoolMinChunks waves, and runs
// beyond the kSubFinalMaxPools-th, take the plain form.
constexpr int kSubFinalPoolWaves = 11, kSubFinalPoolMinChunks = 40, kSubFinalMaxPools = 8;
constexpr int kSubseqCtlPoolCounter = 72;  // changed_dev words [72, 72 + kSubFinalMaxPools): the pools' counters (cleared by every launch)
struct SubseqPool {
    int first, count;  // entries of the pooled work list (one per wave of 64 lanes)
};
// DRI = 0 scans (K2S): self-synchronising subsequence decode into the coefficient buffer (device_rounds: see launch_subseq_sync).
constexpr uint32_t kSubseqBits = 1024;  // smallest subsequence (DevScan::sub_shift = 10); large batches use 2048 / 4096 bits
hipError_t launch_subseq_decode(hipStream_t stream, const uint8_t *udata, const DevScan *scans, const HuffWork *work, int n_work,
                                const uint32_t *scan_ids, int n_scans, const uint32_t *ends_u, DevScanStatus *status,
                                const DevHuffTable *huff_pool, uint32_t *exit_a, uint32_t *exit_b, uint32_t *nblk, uint32_t *first_block,
                                uint32_t *entry_used, void *dcsum, void *dc_entry, uint32_t *changed_dev, int16_t *coefs, int n_slots,
                                int max_rounds, int *rounds_used, const uint8_t *lut_pool, const HuffWork *final_work, int n_final_work,
                                uint32_t *same_dist, bool *same_valid, int device_rounds, const HuffWork *gather_work, int n_gather,
                                const HuffWork *pool_work, const SubseqPool *pools, int n_pools, int num_cus, uint32_t *lane_perm, int subs_per_lane,
                                uint32_t tab_bytes, const uint8_t *sr_luts);
#ifndef JPGPU_SR_LB
#define JPGPU_SR_LB 10
#endif
constexpr int kSrLutBits = JPGPU_SR_LB;  // lookup width of the K2S round kernel (a 10-bit prefix decides codes of up to 10 bits)
constexpr size_t kSrLutSetBytes = (size_t)kMaxHuffSlots << (kSrLutBits + 2);
// sr_luts: the round kernel's lookups, kMaxHuffSlots << (kSrLutBits + 2) bytes per distinct set of tables among the DRI = 0 scans
// (DevScan::sr_set), built once per upload behind launch_lut_pool; set_scan[k] = a scan that stages set k
hipError_t launch_sr_luts(hipStream_t stream, const DevScan *scans, const uint32_t *set_scan, int n_sets, const uint8_t *lut_pool, uint8_t *sr_luts);
// subs_per_lane: subsequences a lane of the final pass takes (the work lists are built for it): kSubFinalSubsPerLane for batches that
// fill the machine, 1 below kSubFinalFewSubs subsequences in the batch (a lone 67-Mpixel canvas: twice the waves, half as long each)
constexpr uint64_t kSubFinalFewSubs = 1u << 20;
// lane_perm: one uint32 per subsequence -- the final pass's lanes of every scan ordered by the MCUs they own (subseq_order_kernel)
// changed_dev: kSubseqCtlWords uint32 (exits changed per round, the device-driven rounds' state; word kSubseqCtlSameDone is
// cleared once per upload, the rest by every launch).  device_rounds > 0: that many rounds enqueued, nothing read back, the
// caller checks changed_dev when it next waits for the stream (k2s_subseq.hip); 0: the host checks between rounds.
constexpr uint32_t kSubseqGatherSpan = 1024;
constexpr int kSubseqCtlWords = 128, kSubseqCtlSameDone = 96, kSubseqFirstBudget = 16;
constexpr int kSubseqMaxDeviceRounds = 61;  // rounds launch_subseq_decode enqueues at most without the host looking (control words [0, 62))
// waves (of 64 subsequences) per workgroup of the K2S final pass.  4 = two workgroups per CU; one workgroup of 10 waves (K2's
// shape, 25 % more waves per CU) was measured slower: 21.1 vs 19.6 ms K2S per 1024 x 4K -- a workgroup waits for its slowest wave
#ifndef JPGPU_SF_WAVES
#define JPGPU_SF_WAVES 4
#endif
constexpr int subseq_final_waves() { return JPGPU_SF_WAVES; }
// the pooled form (eleven waves per workgroup since round 6) fits while the staged tables leave room for them
constexpr uint32_t kSfWaveLdsBytes = kK2WaveLdsBytes;
constexpr bool subseq_pool_fits(uint32_t tab_bytes) { return tab_bytes + (uint32_t)kSubFinalPoolWaves * kSfWaveLdsBytes <= kK2LdsBudget; }
// subsequences per lane of the K2S final pass (1: 8.1 ms per 1024 x 4K; 2: see DESIGN.md)
#ifndef JPGPU_SF_SUBS
#define JPGPU_SF_SUBS 2
#endif
constexpr int kSubFinalSubsPerLane = JPGPU_SF_SUBS;
// per pool table (lut_pool_kernel): the u16 images as an AC and as a DC table (2^11 + 256 u16 entries, header, the reference's arrays:
// what the K2S round kernel derives its lookups from), then the u32 images of round 6 (2^11 / 2^9 entries that carry values and pairs: K2, K2S final pass)
constexpr size_t kLutPoolBytesPerTable = 2 * (4096 + 512 + 16 + 320) + (8192 + 512 + 16 + 320) + (2048 + 512 + 16 + 320);

// progressive frames (K2P): the scans of one ordinal (position inside their frame) of every progressive frame in the batch
hipError_t launch_progressive(hipStream_t stream, const uint8_t *udata, const DevScan *scans, const HuffWork *work, int n_work,
                              const uint32_t *ends_u, DevScanStatus *status, const DevHuffTable *huff_pool, int16_t *coefs, int n_slots);
hipError_t launch_progressive_streams(hipStream_t stream, const uint8_t *udata, const DevScan *scans, const HuffWork *work, int n_work,
                                      const uint32_t *ends_u, DevScanStatus *status, const DevHuffTable *huff_pool, int16_t *coefs,
                                      int n_slots, int pipelined, uint32_t spin_budget, uint32_t *started);
size_t progressive_stream_lds_bytes(int n_slots);  // LDS of one stream workgroup (residency estimate of the pipelined launch)
int progressive_stream_blocks_per_cu(int n_slots);  // stream workgroups a CU holds at once by the runtime's occupancy query (0 = unknown)

// "O3": PLANAR_I16 planes -> the test writer's uint16 x 4 form (extend_u16_kernel)
hipError_t launch_extend_u16(hipStream_t stream, const uint8_t *planes, uint8_t *out_base, const ExtendPlanes *images, int n_images,
                             uint32_t max_pixels);

// K0 (ingest verification): offset of the first non-RST marker in each segment {offset lo, length} (+ offset hi), 0xFFFFFFFF = none
// JPGPU_UPLOAD_PINNED, segments scattered in page-locked host memory: the device reads them over the host link itself
hipError_t launch_gather_pinned(hipStream_t stream, const GatherPiece *pieces, int n_pieces, uint8_t *dst);
hipError_t launch_first_marker(hipStream_t stream, const uint8_t *data, const void *segs, const uint32_t *seg_hi, int n_segs,
                               uint32_t max_len, uint32_t *first);

// jpgpu_batch_upload_device (k0_device_files.hip): files from the caller's device memory into the input buffer; the length of the
// head the host parser needs of each (kHeadGaveUp: the walk gave up) and the heads packed at head_off[i]; the two bytes at each
// verdict of first_marker_kernel (low byte first, 0 = no such position)
hipError_t launch_gather_device(hipStream_t stream, const GatherPiece *pieces, int n_pieces, uint8_t *dst);
hipError_t launch_head_walk(hipStream_t stream, const uint8_t *data, const DeviceFile *files, int n, uint32_t *head_len);
hipError_t launch_head_scan(hipStream_t stream, const uint32_t *head_len, int n, uint64_t *head_off);  // head_off[n] = the total
hipError_t launch_head_pack(hipStream_t stream, const uint8_t *data, const DeviceFile *files, int n, const uint32_t *head_len,
                            const uint64_t *head_off, uint8_t *heads);
hipError_t launch_verdict_bytes(hipStream_t stream, const uint8_t *data, const void *segs, const uint32_t *seg_hi, const uint32_t *first,
                                int n, uint32_t *bytes);

// KT: symbol-level Huffman transcode of baseline scans (JpegOptimizer): mode 0 count, 1 measure, 2 emit (kt_transcode.hip)
struct EncHuffTable;
hipError_t launch_transcode(hipStream_t stream, int mode, const uint8_t *udata, const uint8_t *input, const DevScan *scans,
                            const HuffWork *work, int n_work, const uint32_t *ends_u, const uint32_t *ends_raw, DevScanStatus *status,
                            const DevHuffTable *huff_pool, uint32_t *hist, const EncHuffTable *enc, uint32_t *sizes,
                            const uint64_t *offsets, uint8_t *out, int n_slots);
hipError_t launch_transcode_offsets(hipStream_t stream, const DevScan *scans, const uint32_t *scan_ids, int n_scans, const uint32_t *sizes,
                                    const uint64_t *base, uint64_t *offsets, uint64_t *totals);
// K2S synchronisation alone + KTS: transcode of DRI = 0 scans by subsequence (kt_transcode.hip)
hipError_t launch_subseq_sync(hipStream_t stream, const uint8_t *udata, const DevScan *scans, const HuffWork *work, int n_work,
                              const uint32_t *scan_ids, int n_scans, const uint32_t *ends_u, DevScanStatus *status,
                              const DevHuffTable *huff_pool, uint32_t *exit_a, uint32_t *exit_b, uint32_t *nblk, uint32_t *first_block,
                              uint32_t *entry_used, void *dcsum, void *dc_entry, uint32_t *changed_dev, int n_slots, int max_rounds,
                              int *rounds_used, const uint8_t *lut_pool, const uint32_t **final_state_out, uint32_t *same_dist, bool *same_valid,
                              int device_rounds, const HuffWork *gather_work, int n_gather, const uint8_t *sr_luts);
// gather_work: (scan, first subsequence) per kSubseqGatherSpan subsequences -- the work list of the rounds behind round 1
// (same_dist: one uint32 per subsequence, *same_valid: "filled for this upload" -- the flat-region twins, k2s_subseq.hip)
hipError_t launch_subseq_transcode(hipStream_t stream, int mode, const uint8_t *udata, const DevScan *scans, const HuffWork *work, int n_work,
                                   const uint32_t *ends_u, DevScanStatus *status, const DevHuffTable *huff_pool, const uint32_t *exit_state,
                                   const uint32_t *first_block, uint32_t *hist, const EncHuffTable *enc, uint32_t *sub_bits,
                                   const uint64_t *sub_bitoff, const uint64_t *scan_raw_off, uint8_t *raw, int n_slots);
hipError_t launch_subseq_bit_offsets(hipStream_t stream, const DevScan *scans, const uint32_t *scan_ids, int n_scans, const uint32_t *sub_bits,
                                     uint64_t *bitoff, uint64_t *totals);

// K4 (k4_resample.hip): the RGB_PLANAR_U8 images in `src` (K3's output buffer) resampled to one dense T[n][3][out_height][out_width] of
// sample_format (RGB_PLANAR_U8 / _F16 / _F32 samples) in `dst`.  One ResizeImage per image that takes part; `tables`: the tap tables of both
// axes as resize_axis_pack lays them out (resize_tables.h), equal (input, output) lengths sharing one.  src is 256-byte aligned with at
// least 16 bytes of slack behind the last image.  aff: the affine step of the float samples.
constexpr int kResizeBandRows = 8;        // output rows one workgroup forms
constexpr int kResizePieceBytes = 4096;   // bytes of one plane's input row staged in LDS at a time
struct ResizeImage {
    uint64_t src_off;          // the image's R plane in src (bytes); G and B follow, w_in * h_in bytes each
    uint64_t dst_off;          // the image's slab in dst (samples)
    uint32_t w_in, h_in;
    uint32_t h_off, h_taps;    // the horizontal table (w_in -> out_width): its first word in `tables`, taps per output
    uint32_t v_off, v_taps;    // the vertical one (h_in -> out_height)
};
hipError_t launch_resample(hipStream_t stream, const uint8_t *src, const ResizeImage *images, int n_images, const uint32_t *tables, void *dst,
                           int out_width, int out_height, int sample_format, const OutputAffine &aff);
// K4 on one plane (k4y_resample_luma.hip): the grey planes of a JPGPU_CHANNELS_LUMA upload of RGB_PLANAR_U8, ONE tight plane per image at
// src_off, to one dense T[n][1][out_height][out_width].  The same descriptors, tables and function per plane; aff.scale[0] and aff.bias[0].
hipError_t launch_resample_luma(hipStream_t stream, const uint8_t *src, const ResizeImage *images, int n_images, const uint32_t *tables, void *dst,
                                int out_width, int out_height, int sample_format, const OutputAffine &aff);
}  // namespace jpgpu
