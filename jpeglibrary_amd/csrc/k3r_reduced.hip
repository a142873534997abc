// jpeglibrary_amd/csrc/k3r_reduced.hip -- K3R: the images decoded at 1/2, 1/4 or 1/8 size with libjpeg's reduced transforms under
// JPGPU_ARITHMETIC_LIBJPEG (include/jpgpu.h, "Scaled decode").
//
// reduced_kernel: one launch per decode behind K3J's; blockIdx.x = a ReducedWork entry (kernels.h): the blocks of up to 256 / blocks_per_mcu
// consecutive MCUs of one MCU row of the window's MCU cover, as K3J (k3j_islow.hip) takes them, and m = 8 / denom of the entry's image.  A lane
// takes a block, of any component.
//   1. the 128 coefficient bytes of every block go to LDS by DMA, K3J's staging; where every component of the scan yields ONE sample per
//      block only the block's first 16-byte piece (zig-zag 0..7, the DC among them) is fetched.  The quantisers go to LDS as they are;
//   2. behind ONE barrier the lane runs its component's transform (k3r_reduced.h): s = reduced_block_size() samples per side -- 8, 4, 2 or 1 --,
//      divergent only between the components of an MCU;
//   3. a block a failing scan did not reach is zero, as K3J leaves it;
//   4. the s x s samples go to the image's scratch slot as INTERLEAVED_U8: the REDUCED picture, in which an MCU is m * max_h x m * max_v pixels
//      and the block lies where K3J puts it, times m / 8, every sample repeated rh x rv times (s * rh = hs * m), clipped to the window --
//      DevScan::win_* and cov_* of such a scan are in pixels and MCUs of the reduced picture.  ASSEMBLED in LDS and stored as aligned dwords
//      where the scan names every component (the strip is at most a quarter of K3J's: it always fits), BYTEWISE otherwise.
// K3C / K3U / K3O / K3Y's luma_plane_kernel / K4 then read the scratch slot as they read K3J's: a picture whose chroma ratio is the residual one.
// (A file of its own so that every other kernel object stays what it was.)
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "k3r_reduced.h"

namespace jpgpu {

namespace {

typedef __attribute__((address_space(3))) void reduced_lds_void;
typedef const __attribute__((address_space(1))) void reduced_gbl_void;

static_assert(kIslowThreads == 256, "eight DMA instructions of 32 blocks per workgroup");
constexpr uint32_t kReducedStaging = kIslowThreads * 128;  // bytes: the coefficient blocks, then the strip of pixels

// sample (r, c) of a block as the transforms leave it
__device__ inline uint8_t reduced_px(const uint32_t (&px)[16], uint32_t r, uint32_t c) { return (uint8_t)(px[2 * r + (c >> 2)] >> (8 * (c & 3u))); }

__global__ __launch_bounds__(kIslowThreads, 4) void reduced_kernel(const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans,
                                                                   const ReducedWork *__restrict__ work, const DevScanStatus *__restrict__ status,
                                                                   const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) uint8_t sh[kReducedStaging + kMaxScanComponents * 128];
    uint16_t *sh_q = reinterpret_cast<uint16_t *>(sh + kReducedStaging);  // DevQuantTable::q of the scan components

    const ReducedWork wk = work[blockIdx.x];
    const DevScan &s = scans[wk.scan];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bpm = s.blocks_per_mcu, mpl = s.mcus_per_line;
    const uint32_t row_blocks = (uint32_t)s.cov_cols * bpm;
    const uint32_t m = wk.m;
    if (bpm == 0 || bpm > (uint32_t)kMaxBlocksPerMcu || wk.first >= row_blocks || wk.row >= s.cov_rows || wk.first % bpm != 0) return;  // (never listed)
    if (m != 1u && m != 2u && m != 4u) return;                                                                                        // (never listed)
    const uint32_t per_wg = islow_blocks_per_wg(bpm);
    const uint32_t n = row_blocks - wk.first < per_wg ? row_blocks - wk.first : per_wg;  // whole MCUs
    const uint32_t mcu_y = (uint32_t)s.cov_y + wk.row;
    const uint32_t mcu_x0 = (uint32_t)s.cov_x + wk.first / bpm;  // the strip's first MCU
    const uint32_t first_block = (mcu_y * mpl + s.cov_x) * bpm + wk.first;  // in the scan's store
    const uint32_t max_h = s.max_h, max_v = s.max_v, C = s.frame_components;

    // the scan's components: inside the frame (DeviceBatch::islow_taken: always), all of them named and filling the MCU's box, one sample each?
    bool assembled = s.scan_components == C, inside = max_h != 0 && max_v != 0, all_dc = true;
    for (uint32_t c = 0; c < (uint32_t)s.scan_components && c < (uint32_t)kMaxScanComponents; c++) {
        const uint32_t h = s.comp[c].h, v = s.comp[c].v;
        inside = inside && s.comp[c].component_index < C && h != 0 && v != 0;
        if (!inside) break;
        assembled = assembled && h * s.comp[c].hs == max_h && v * s.comp[c].vs == max_v;
        all_dc = all_dc && reduced_block_size(m, h, v, max_h, max_v) == 1u;
    }
    if (!inside) return;  // (the whole workgroup leaves, in front of the barriers below)
    // the strip: n_mcu MCUs side by side, m * max_v rows of `pitch` bytes (at most a quarter of K3J's for the layouts encoders make)
    const uint32_t n_mcu = n / bpm;
    const uint32_t rows = m * max_v, pitch = n_mcu * m * max_h * C;
    assembled = assembled && rows * pitch <= kReducedStaging;

    // ---- 1. DMA, K3J's: linear 16-byte slot c = k * 256 + tid (block c >> 3, slot c & 7) receives piece (slot ^ swizzle(block)) of its block
    {
        const uint8_t *coef_bytes = reinterpret_cast<const uint8_t *>(coefs + s.coef_off * 64);
        const uint32_t piece = (tid & 7u) ^ ((tid >> 4) & 7u);
        // (all_dc: only the lanes whose slot receives piece 0 fetch; the other slots of the staging are never read)
        if (!all_dc || piece == 0u) {
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                uint32_t blk = k * 32u + (tid >> 3);
                blk = blk < n ? blk : n - 1;
                __builtin_amdgcn_global_load_lds((reduced_gbl_void *)(coef_bytes + (uint64_t)(first_block + blk) * 128 + piece * 16u),
                                                 (reduced_lds_void *)(sh + (k * kIslowThreads + wave * 64) * 16), 16, 0, 0);
            }
        }
    }
    {
        const uint32_t c = tid >> 6, i = tid & 63u;
        if (c < (uint32_t)s.scan_components) sh_q[c * 64 + i] = quant_pool[s.quant_pool[s.comp[c].quant_slot]].q[i];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- 2. the lane's block (a lane behind the last block: block n - 1 once more, nothing of it stored)
    const bool active = tid < n;
    const uint32_t k_row = active ? tid : n - 1;
    const uint32_t ml = k_row / bpm, b = k_row - ml * bpm;  // the MCU in the strip, the block in the MCU
    const uint32_t mcu_x = mcu_x0 + ml;
    const uint32_t mcu = mcu_y * mpl + mcu_x;
    const uint32_t ci = s.blk_comp[b] & 3u;
    const DevScanComponent comp = s.comp[ci];
    const uint32_t bs = reduced_block_size(m, comp.h, comp.v, max_h, max_v);  // samples per side of the block
    const uint32_t rh = reduced_replication(m, bs, comp.h, max_h), rv = reduced_replication(m, bs, comp.v, max_v);
    uint32_t px[16];
#pragma unroll
    for (int i = 0; i < 16; i++) px[i] = 0;
    reduced_block(bs, sh + k_row * 128, (k_row >> 1) & 7u, sh_q + ci * 64, px);

    // ---- 3. what the scan did not reach is zero (K3J's rule)
    uint32_t decoded = status ? status[wk.scan].decoded_mcus : s.total_mcus;
    if (decoded > s.total_mcus) decoded = s.total_mcus;
    uint32_t fail_block = 0xFFFFFFFFu;
    if (status != nullptr && s.kind == kScanSequential) {
        const uint32_t fb = status[wk.scan].pad[1];
        if (fb != 0) fail_block = kFailBlockBase - fb;
        for (uint32_t j = s.first_scan; j < wk.scan; j++)
            if (scans[j].image_index == s.image_index && status[j].first_error != kNoError) fail_block = 0;
    }
    const bool reached = mcu < decoded && mcu * bpm + b < fail_block;
    if (!reached) {
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = 0;
    }

    // ---- 4. the samples of the reduced picture
    const bool flush = s.kind == kScanFrameOnly;
    const uint32_t W = s.win_w, H = s.win_h;
    const uint32_t wx = s.win_x, wy = s.win_y;
    uint8_t *img = scratch + s.out_off;

    if (!assembled) {  // (workgroup-uniform)
        if (!active) return;
        const uint32_t x0 = flush ? (mcu_x * comp.h + s.blk_x[b]) * comp.hs * m : (mcu_x * max_h + s.blk_x[b]) * m;
        const uint32_t y0 = flush ? (mcu_y * comp.v + s.blk_y[b]) * comp.vs * m : (mcu_y * max_v + s.blk_y[b]) * m;
        uint8_t *at = img + comp.component_index;
#pragma unroll
        for (uint32_t r = 0; r < 8; r++) {
            if (r >= bs) continue;
            for (uint32_t v = 0; v < rv; v++) {
                const uint32_t y = y0 + r * rv + v - wy;  // (above the window wraps to a large value)
                if (y >= H) continue;
                uint8_t *line = at + (uint64_t)y * W * C;
#pragma unroll
                for (uint32_t c = 0; c < 8; c++) {
                    if (c >= bs) continue;
                    const uint8_t u = reduced_px(px, r, c);
                    for (uint32_t h = 0; h < rh; h++) {
                        const uint32_t x = x0 + c * rh + h - wx;
                        if (x < W) line[(uint64_t)x * C] = u;
                    }
                }
            }
        }
        return;
    }

    // every lane holds its samples: the staging becomes the strip.  (h * hs == max_h and v * vs == max_v: the block's place inside its MCU is
    // (blk_x * hs * m, blk_y * vs * m) in both kinds of scan.)
    __syncthreads();
    if (active) {
        uint8_t *at = sh + (s.blk_y[b] * comp.vs * m) * pitch + ((ml * max_h + s.blk_x[b] * comp.hs) * m) * C + comp.component_index;
#pragma unroll
        for (uint32_t r = 0; r < 8; r++) {
            if (r >= bs) continue;
            for (uint32_t v = 0; v < rv; v++) {
                uint8_t *line = at + (r * rv + v) * pitch;
#pragma unroll
                for (uint32_t c = 0; c < 8; c++) {
                    if (c >= bs) continue;
                    const uint8_t u = reduced_px(px, r, c);
                    for (uint32_t h = 0; h < rh; h++) line[(c * rh + h) * C] = u;
                }
            }
        }
    }
    __syncthreads();
    // the strip's pixels [xs, xe) of the reduced picture lie in the window; row r of the strip is line (mcu_y * max_v * m + r) of the picture
    const uint32_t sx0 = mcu_x0 * max_h * m, sx1 = sx0 + n_mcu * max_h * m;
    const uint32_t xs = sx0 > wx ? sx0 : wx, xe = sx1 < wx + W ? sx1 : wx + W;
    if (xs >= xe) return;
    const uint32_t len = (xe - xs) * C;  // bytes of a row's run
    const uint32_t *sh32 = reinterpret_cast<const uint32_t *>(sh);
    for (uint32_t r = 0; r < rows; r++) {
        const uint32_t y = mcu_y * max_v * m + r - wy;
        if (y >= H) continue;  // (workgroup-uniform)
        uint8_t *dst = img + ((uint64_t)y * W + (xs - wx)) * C;
        const uint32_t src = r * pitch + (xs - sx0) * C;  // byte offset in the staging
        uint32_t head = (uint32_t)(0u - (uint32_t)reinterpret_cast<uintptr_t>(dst)) & 3u;
        head = head < len ? head : len;
        const uint32_t n_dw = (len - head) >> 2, tail = (len - head) & 3u;
        for (uint32_t k = tid; k < n_dw; k += kIslowThreads) {
            const uint32_t o = src + head + 4u * k;
            const uint32_t lo = sh32[o >> 2], hi = sh32[(o >> 2) + 1];  // (the second may lie behind the strip, inside `sh`: its bytes are shifted out or belong to the run)
            *reinterpret_cast<uint32_t *>(dst + head + 4u * k) = __builtin_amdgcn_alignbyte(hi, lo, o & 3u);
        }
        if (tid < head) dst[tid] = sh[src + tid];
        if (tid < tail) dst[head + 4u * n_dw + tid] = sh[src + head + 4u * n_dw + tid];
    }
}

}  // namespace

hipError_t launch_reduced(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const ReducedWork *work, int n_work, const DevScanStatus *status,
                          const DevQuantTable *quant_pool, uint8_t *scratch) {
    if (n_work <= 0) return hipSuccess;
    if (scratch == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reduced_kernel, dim3((uint32_t)n_work), dim3(kIslowThreads), 0, stream, coefs, scans, work, status, quant_pool, scratch);
    return hipGetLastError();
}

}  // namespace jpgpu
