// jpeglibrary_amd/csrc/k3y_luma.hip -- K3Y: the images decoded to ONE plane under JPGPU_CHANNELS_LUMA (include/jpgpu.h, "Grey output").
//
// luma_idct_kernel<T, WIN>, the fast road: component 0's blocks of a sequential scan, from the dense coefficient store straight to the plane.
// One launch per decode; blockIdx.x = a LumaWork entry (kernels.h): up to four UNITS, a unit being 64 neighbouring blocks of one block row of
// the luma grid of the window's MCU cover.  A wave takes a unit, a lane a block, so a row store of the wave is 64 x 8 neighbouring samples
// of one line of the plane: 512 contiguous bytes for uint8.  The chroma blocks are neither fetched nor transformed.
//   1. the 128 coefficient bytes of every block go to LDS by DMA (sixteen bytes per lane and instruction, K3's swizzled staging): DMA k of
//      the workgroup fills blocks k * 32 .. k * 32 + 31, which belong to unit k / 2 -- wave-uniform -- so a lane finds its source block
//      with one multiply by a reciprocal (component 0 has 1..4 blocks per MCU line) and no division;
//   2. behind ONE barrier the lane runs K3's transform on its block (k3_block_idct.h: the same packed-word dequantisation, the same two
//      butterfly passes, rounding, level shift and saturating pack, bit for bit);
//   3. a block at or behind the block a failing scan threw in, or in an MCU the scan never reached, is zero, as K3 leaves it
//      (DevScanStatus::decoded_mcus, pad[1]; DevScan::first_scan);
//   4. the eight rows go out as one piece of 8 bytes (uint8), one of 16 (float16) or two of 16 (float32), declared aligned for one sample
//      only -- the plane's width is arbitrary --; a block the window cuts on the left or the right goes sample by sample, rows above or below
//      the window are not stored.
// WIN = false: every listed scan is a whole frame (cover = the MCU grid from (0, 0), window = the frame).
//
// luma_plane_kernel<T>, the scratch road: every other image, from the INTERLEAVED_U8 samples K3's generic class left in the scratch image.
// K3O's structure (k3o_orient.hip) with a parked pixel of one byte: blockIdx.y = image, blockIdx.x = a tile of kOrientTile x kOrientTile
// pixels of the SOURCE window; a wave loads a row of the tile, forms the sample -- byte 0 for the kinds GRAY and YCBCR, L of K3C's pixel for
// RGB, CMYK and YCCK --, parks it, and behind one barrier a wave reads 64 neighbouring destination samples of one destination row, along
// the tile's rows (orientations 1..4) or columns (5..8), and stores them side by side.
// (A file of its own so that every other kernel object stays what it was.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "k3_block_idct.h"
#include "k3c_pixel.h"

namespace jpgpu {

namespace {

typedef __attribute__((address_space(3))) void luma_lds_void;
typedef const __attribute__((address_space(1))) void luma_gbl_void;

constexpr uint32_t kLumaThreads = kLumaUnitBlocks * kLumaUnitsPerWg;
static_assert(kLumaThreads == 256 && kLumaUnitBlocks == 64, "a wave per unit, eight DMA instructions of 32 blocks per workgroup");

template <typename T>
constexpr int luma_fmt() {
    return sizeof(T) == 1 ? kFmtRgbPlanarU8 : (sizeof(T) == 2 ? kFmtRgbPlanarF16 : kFmtRgbPlanarF32);
}

// x / n == (x * luma_recip(n)) >> 16 for n = 1..4 and x < 32768 (a frame has at most 8192 blocks per line)
__device__ __forceinline__ uint32_t luma_recip(uint32_t n) { return n == 1u ? 65536u : (n == 2u ? 32768u : (n == 3u ? 21846u : 16384u)); }

// eight samples of one line (lo = bytes 0..3, hi = bytes 4..7) at dst, which is aligned for one sample only
template <typename T>
__device__ __forceinline__ void store_luma8(uint8_t *dst, uint32_t lo, uint32_t hi, float scale, float bias) {
    if constexpr (sizeof(T) == 1) {
        const uint2 w = {lo, hi};
        __builtin_memcpy(dst, &w, 8);
    } else {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; j++) f[j] = affine_sample(((j < 4 ? lo : hi) >> (8 * (j & 3))) & 0xFFu, scale, bias);
        if constexpr (sizeof(T) == 4) {
            __builtin_memcpy(__builtin_assume_aligned(dst, 4), f, 16);
            __builtin_memcpy(__builtin_assume_aligned(dst + 16, 4), f + 4, 16);
        } else {
            const half2v h[4] = {__builtin_convertvector(float2v{f[0], f[1]}, half2v), __builtin_convertvector(float2v{f[2], f[3]}, half2v),
                                 __builtin_convertvector(float2v{f[4], f[5]}, half2v), __builtin_convertvector(float2v{f[6], f[7]}, half2v)};
            __builtin_memcpy(__builtin_assume_aligned(dst, 2), h, 16);
        }
    }
}

template <typename T, bool WIN>
__global__ __launch_bounds__(kLumaThreads, 4) void luma_idct_kernel(const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans,
                                                                    const LumaWork *__restrict__ work, const DevScanStatus *__restrict__ status,
                                                                    const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ out, float scale,
                                                                    float bias) {
    __shared__ __attribute__((aligned(16))) uint8_t sh[kLumaThreads * 128 + 256];
    float *sh_q = reinterpret_cast<float *>(sh + kLumaThreads * 128);  // DevQuantTable::qf of component 0

    const LumaWork wk = work[blockIdx.x];
    const DevScan &s = scans[wk.scan];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bpm = s.blocks_per_mcu, mpl = s.mcus_per_line;
    const uint32_t h0 = s.comp[0].h, v0 = s.comp[0].v;  // component 0's blocks per MCU line and column: the frame's maxima
    const uint32_t rh = luma_recip(h0), rv = luma_recip(v0);
    const uint32_t cov_x = WIN ? (uint32_t)s.cov_x : 0u, cov_y = WIN ? (uint32_t)s.cov_y : 0u;
    const uint32_t cols = (uint32_t)s.cov_cols * h0;          // blocks per row of the cover's luma grid
    const uint32_t chunks = (cols + kLumaUnitBlocks - 1) / kLumaUnitBlocks;
    const uint32_t n_units = wk.n_units < kLumaUnitsPerWg ? wk.n_units : kLumaUnitsPerWg;
    if (n_units == 0 || cols == 0) return;  // (never listed)
    // unit u of the workgroup: `u` chunks behind the first, in raster order (a unit past the last listed one: the last one's place, so that
    // its DMA stays inside the scan's region; nothing of it is stored)
    auto unit_place = [&](uint32_t u, uint32_t &row, uint32_t &chunk) {
        row = wk.row;
        chunk = wk.chunk + (u < n_units ? u : n_units - 1);
        while (chunk >= chunks) {  // (at most three turns)
            chunk -= chunks;
            row++;
        }
    };
    // block column bc of block row `row` of the cover's luma grid: its MCU, its slot there and its number in the scan's dense store
    auto block_of = [&](uint32_t row, uint32_t bc, uint32_t &mcu, uint32_t &slot) {
        const uint32_t mxl = (bc * rh) >> 16, myl = (row * rv) >> 16;
        slot = (row - myl * v0) * h0 + (bc - mxl * h0);
        mcu = (cov_y + myl) * mpl + cov_x + mxl;  // (a frame has fewer than 2^32 blocks)
    };

    // ---- 1. DMA: linear 16-byte slot c = k * 256 + tid (block c >> 3, slot c & 7) receives piece (slot ^ swizzle(block)) of its block
    {
        const uint8_t *coef_bytes = reinterpret_cast<const uint8_t *>(coefs + s.coef_off * 64);
        const uint32_t piece_off = ((tid & 7u) ^ ((tid >> 4) & 7u)) * 16u;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            uint32_t row, chunk, mcu, slot;
            unit_place(k >> 1, row, chunk);
            uint32_t bc = chunk * kLumaUnitBlocks + (k & 1u) * 32u + (tid >> 3);
            bc = bc < cols ? bc : cols - 1;  // (lanes behind the row's last block fetch that block)
            block_of(row, bc, mcu, slot);
            const uint32_t block = mcu * bpm + slot;
            __builtin_amdgcn_global_load_lds((luma_gbl_void *)(coef_bytes + (uint64_t)block * 128 + piece_off),
                                             (luma_lds_void *)(sh + (k * kLumaThreads + wave * 64) * 16), 16, 0, 0);
        }
    }
    if (tid < 64) sh_q[tid] = quant_pool[s.quant_pool[s.comp[0].quant_slot]].qf[tid];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave >= n_units) return;  // (a whole wave; no barrier follows)

    // ---- 2. the lane's block
    uint32_t row, chunk, mcu, slot;
    unit_place(wave, row, chunk);
    const uint32_t bc = chunk * kLumaUnitBlocks + (tid & 63u);
    block_of(row, bc < cols ? bc : cols - 1, mcu, slot);
    uint32_t cw[32], px[32];
    block_load(sh + tid * 128, (tid >> 1) & 7, cw);
    block_idct(cw, sh_q, (int32_t)s.level_shift, px);

    // ---- 3. what the scan did not reach is zero (K3: idct_output_body)
    uint32_t decoded = status ? status[wk.scan].decoded_mcus : s.total_mcus;
    if (decoded > s.total_mcus) decoded = s.total_mcus;
    uint32_t fail_block = 0xFFFFFFFFu;
    if (status != nullptr) {
        const uint32_t fb = status[wk.scan].pad[1];
        if (fb != 0) fail_block = kFailBlockBase - fb;
        for (uint32_t j = s.first_scan; j < wk.scan; j++)
            if (scans[j].image_index == s.image_index && status[j].first_error != kNoError) fail_block = 0;
    }
    const bool reached = mcu < decoded && mcu * bpm + slot < fail_block;
    if (!reached) {
#pragma unroll
        for (int i = 0; i < 32; i++) px[i] = 0;
    }

    // ---- 4. the rows
    if (bc >= cols) return;
    const uint32_t win_w = s.win_w, win_h = s.win_h;
    const int32_t x0 = (int32_t)((cov_x * h0 + bc) * 8u) - (WIN ? (int32_t)s.win_x : 0);
    // (K3's placement, (mcu_y * max_v + by) * 8: where component 0 has ONE block per MCU column under a taller MCU, vs > 1, the block
    // covers 8 * vs lines and every sample row is repeated over vs of them -- WriteBlockSlow's replication; vs == 1 otherwise)
    const uint32_t vs = s.comp[0].vs, myl = (row * rv) >> 16;
    const int32_t y0 = (int32_t)(((cov_y + myl) * (uint32_t)s.max_v + (row - myl * v0)) * 8u) - (WIN ? (int32_t)s.win_y : 0);
    uint8_t *plane = out + s.out_off;
    const bool whole_rows = (!WIN || x0 >= 0) && x0 + 8 <= (int32_t)win_w;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint32_t lo = pack4_u8(px[r * 4 + 0], px[r * 4 + 1]), hi = pack4_u8(px[r * 4 + 2], px[r * 4 + 3]);
        for (uint32_t k = 0; k < vs; k++) {  // (wave-uniform; one turn but for the replicated arrangement)
            const int32_t y = y0 + r * (int32_t)vs + (int32_t)k;
            if ((WIN && y < 0) || y >= (int32_t)win_h) continue;
            const int64_t at = (int64_t)y * win_w + x0;  // (sample index of the row's first column; only used where it is inside)
            if (whole_rows) {
                store_luma8<T>(plane + (uint64_t)at * sizeof(T), lo, hi, scale, bias);
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if ((!WIN || x0 + j >= 0) && x0 + j < (int32_t)win_w)
                        store_plane1<luma_fmt<T>()>(plane, (uint64_t)(at + j), ((j < 4 ? lo : hi) >> (8 * (j & 3))) & 0xFFu, scale, bias);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the scratch road

constexpr uint32_t kLumaPitch = kOrientTile + 4;  // bytes: a tile row starts on a dword

// Pillow's convert("L") of R | G << 8 | B << 16
__device__ __forceinline__ uint32_t luma_of_rgb(uint32_t px) {
    return (19595u * (px & 0xFFu) + 38470u * ((px >> 8) & 0xFFu) + 7471u * ((px >> 16) & 0xFFu) + 32768u) >> 16;
}

// A tile of pixels of BPP bytes: the sixteen loads of a lane are issued together -- a lane outside an edge tile reads the tile's last row or
// column instead and parks nothing -- then turned into the sample and parked.
template <uint32_t BPP>
__device__ __forceinline__ void park_luma_tile(uint8_t *tile, const uint8_t *__restrict__ src, uint32_t width, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th,
                                               uint32_t kind, const YccRgbFactors &kf) {
    const uint32_t c = threadIdx.x & 63u, r0 = threadIdx.x >> 6;
    const uint8_t *col = src + (uint64_t)(x0 + min(c, tw - 1)) * BPP;
    uint32_t s[kOrientTile / 4];
#pragma unroll
    for (uint32_t k = 0; k < kOrientTile / 4; k++) {
        const uint8_t *p = col + (uint64_t)(y0 + min(r0 + 4 * k, th - 1)) * width * BPP;
        if constexpr (BPP == 4) s[k] = *reinterpret_cast<const uint32_t *>(p);  // (the slot starts on a multiple of 256: an aligned dword)
        else if constexpr (BPP == 1) s[k] = p[0];
        else s[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
#pragma unroll
    for (uint32_t k = 0; k < kOrientTile / 4; k++) {
        const uint32_t r = r0 + 4 * k;
        uint32_t v;
        if constexpr (BPP == 4) v = luma_of_rgb(color_pixel(kind, s[k], kf));
        else if constexpr (BPP == 1) v = s[k];
        else v = kind == kColorRgb ? luma_of_rgb(s[k]) : (s[k] & 0xFFu);  // (YCBCR: component 0's sample)
        if (r < th && c < tw) tile[r * kLumaPitch + c] = (uint8_t)v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void luma_plane_kernel(const uint8_t *__restrict__ scratch, uint8_t *__restrict__ out, const LumaImage *__restrict__ images,
                                                         YccRgbFactors kf, float scale, float bias) {
    __shared__ __attribute__((aligned(4))) uint8_t tile[kOrientTile * kLumaPitch];
    const LumaImage g = images[blockIdx.y];
    const uint32_t tiles_x = (g.width + kOrientTile - 1) / kOrientTile, tiles_y = (g.height + kOrientTile - 1) / kOrientTile;
    if (blockIdx.x >= tiles_x * tiles_y) return;  // (the grid is the largest image's; the whole workgroup leaves)
    const uint32_t ty = blockIdx.x / tiles_x, x0 = (blockIdx.x - ty * tiles_x) * kOrientTile, y0 = ty * kOrientTile;
    const uint32_t tw = min(kOrientTile, g.width - x0), th = min(kOrientTile, g.height - y0);  // the tile's part of the source window
    const uint32_t kind = g.kind;
    const uint32_t bpp = kind == kColorGray ? 1u : (kind == kColorCmyk || kind == kColorYcck ? 4u : 3u);
    const uint8_t *src = scratch + g.src_off;
    if (bpp == 4) park_luma_tile<4>(tile, src, g.width, x0, y0, tw, th, kind, kf);
    else if (bpp == 3) park_luma_tile<3>(tile, src, g.width, x0, y0, tw, th, kind, kf);
    else park_luma_tile<1>(tile, src, g.width, x0, y0, tw, th, kind, kf);
    __syncthreads();

    // the destination tile (k3o_orient.hip: the same mapping): along a destination row the source runs along a row (orientations 1..4) or a
    // column (5..8) of the tile, forwards or backwards
    const uint32_t o = g.orientation;
    const bool transposed = o >= 5, flip_x = o == 2 || o == 3 || o == 7 || o == 8, flip_y = o == 3 || o == 4 || o == 6 || o == 7;
    const uint32_t rows = transposed ? tw : th, cols = transposed ? th : tw;  // of the destination tile
    const uint32_t dst_w = transposed ? g.height : g.width;
    const uint32_t sx = flip_x ? g.width - x0 - tw : x0, sy = flip_y ? g.height - y0 - th : y0;  // a flipped axis counts from the far end
    const uint32_t X0 = transposed ? sy : sx, Y0 = transposed ? sx : sy;
    const int32_t row_step = (int32_t)(transposed ? 1u : kLumaPitch) * ((transposed ? flip_x : flip_y) ? -1 : 1);
    const int32_t col_step = (int32_t)(transposed ? kLumaPitch : 1u) * ((transposed ? flip_y : flip_x) ? -1 : 1);
    const int32_t base = (row_step < 0 ? -row_step * (int32_t)(rows - 1) : 0) + (col_step < 0 ? -col_step * (int32_t)(cols - 1) : 0);
    uint8_t *dst = out + g.dst_off;
    const uint32_t X = threadIdx.x & 63u;  // a wave: 64 neighbouring samples of one destination row
#pragma unroll
    for (uint32_t k = 0; k < kOrientTile / 4; k++) {
        const uint32_t Y = 4 * k + (threadIdx.x >> 6);
        if (Y >= rows || X >= cols) continue;
        const uint32_t u = tile[base + row_step * (int32_t)Y + col_step * (int32_t)X];
        store_plane1<luma_fmt<T>()>(dst, (uint64_t)(Y0 + Y) * dst_w + X0 + X, u, scale, bias);
    }
}

}  // namespace

hipError_t launch_luma_idct(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const LumaWork *work, int n_work, bool windowed,
                            const DevScanStatus *status, const DevQuantTable *quant_pool, uint8_t *out, int format, const OutputAffine &aff) {
    if (n_work <= 0) return hipSuccess;
    if (!fmt_is_rgb_planes(format)) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)n_work), block(kLumaThreads);
    const float sc = aff.scale[0], bi = aff.bias[0];
#define JPGPU_LUMA_IDCT(T, WIN) hipLaunchKernelGGL((luma_idct_kernel<T, WIN>), grid, block, 0, stream, coefs, scans, work, status, quant_pool, out, sc, bi)
    if (format == kFmtRgbPlanarU8) {
        if (windowed) JPGPU_LUMA_IDCT(uint8_t, true);
        else JPGPU_LUMA_IDCT(uint8_t, false);
    } else if (format == kFmtRgbPlanarF16) {
        if (windowed) JPGPU_LUMA_IDCT(_Float16, true);
        else JPGPU_LUMA_IDCT(_Float16, false);
    } else {
        if (windowed) JPGPU_LUMA_IDCT(float, true);
        else JPGPU_LUMA_IDCT(float, false);
    }
#undef JPGPU_LUMA_IDCT
    return hipGetLastError();
}

hipError_t launch_luma_plane(hipStream_t stream, const uint8_t *scratch, uint8_t *out, const LumaImage *images, int n_images, uint32_t max_tiles,
                             int format, const YccRgbFactors &kf, const OutputAffine &aff) {
    if (n_images <= 0 || max_tiles == 0) return hipSuccess;
    if (!fmt_is_rgb_planes(format)) return hipErrorInvalidValue;
    const float sc = aff.scale[0], bi = aff.bias[0];
    for (int base = 0; base < n_images; base += 65535) {  // grid.y limit
        const dim3 grid(max_tiles, (uint32_t)std::min(n_images - base, 65535));
        if (format == kFmtRgbPlanarU8) hipLaunchKernelGGL(luma_plane_kernel<uint8_t>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, sc, bi);
        else if (format == kFmtRgbPlanarF16) hipLaunchKernelGGL(luma_plane_kernel<_Float16>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, sc, bi);
        else hipLaunchKernelGGL(luma_plane_kernel<float>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, sc, bi);
    }
    return hipGetLastError();
}

}  // namespace jpgpu
