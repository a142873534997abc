// jpeglibrary_amd/csrc/k3j_islow.hip -- K3J: the images decoded with libjpeg's integer transform under JPGPU_ARITHMETIC_LIBJPEG (include/jpgpu.h,
// "Arithmetic").
//
// islow_kernel: one launch per decode behind K3's; blockIdx.x = an IslowWork entry (kernels.h): the blocks of up to 256 / blocks_per_mcu
// consecutive MCUs of one MCU row of the window's MCU cover, which lie side by side in the scan's dense store.  A lane takes a block, of any
// component.
//   1. the 128 coefficient bytes of every block go to LDS by DMA (sixteen bytes per lane and instruction, K3's swizzled staging); lanes behind
//      the workgroup's last block fetch that block, so nothing outside the row is read.  The scan components' quantisers go to LDS as they
//      are (DevQuantTable::q, integers);
//   2. behind ONE barrier the lane runs jpeg_idct_islow on its block (k3j_islow.h): 32-bit integers that wrap, no float;
//   3. a block at or behind the block a failing scan threw in, or in an MCU the scan never reached, is zero, as K3 leaves it
//      (DevScanStatus::decoded_mcus, pad[1]; DevScan::first_scan);
//   4. the 64 samples go to the image's scratch slot as INTERLEAVED_U8, where K3's generic class puts them (k3_idct.hip,
//      interleaved_output_from_tile): the block's place by blk_x / blk_y -- (mcu * max + blk) * 8 in a sequential scan, (mcu * h + blk) * hs * 8
//      in a progressive frame's pass --, every sample repeated over hs x vs pixels, clipped to the window by unsigned compares.
//      ASSEMBLED, where the scan names every frame component, every component's blocks fill the MCU's box (h * hs and v * vs are the maxima) and
//      the workgroup's strip of pixels fits the staging: behind a second barrier the lanes lay their samples into the staging as the strip
//      lies in the image -- 8 * max_v rows of n_mcu * 8 * max_h pixels of C bytes --, and behind a third the workgroup copies every row of the
//      strip that the window holds to the slot as one contiguous run: whole aligned dwords, each built from two LDS dwords, single bytes at its
//      two ends.  BYTEWISE otherwise (a scan of one component of three, a strip that does not fit): the lane stores its bytes itself.
// K3C / K3U / K3O / K3Y's luma_plane_kernel / K4 then read the scratch slot as they read K3's.
// (A file of its own so that every other kernel object stays what it was.)
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "k3j_islow.h"

namespace jpgpu {

namespace {

typedef __attribute__((address_space(3))) void islow_lds_void;
typedef const __attribute__((address_space(1))) void islow_gbl_void;

static_assert(kIslowThreads == 256, "eight DMA instructions of 32 blocks per workgroup");
constexpr uint32_t kIslowStaging = kIslowThreads * 128;  // bytes: the coefficient blocks, then the strip of pixels

__global__ __launch_bounds__(kIslowThreads, 4) void islow_kernel(const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans,
                                                                 const IslowWork *__restrict__ work, const DevScanStatus *__restrict__ status,
                                                                 const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) uint8_t sh[kIslowStaging + kMaxScanComponents * 128];
    uint16_t *sh_q = reinterpret_cast<uint16_t *>(sh + kIslowStaging);  // DevQuantTable::q of the scan components

    const IslowWork wk = work[blockIdx.x];
    const DevScan &s = scans[wk.scan];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t bpm = s.blocks_per_mcu, mpl = s.mcus_per_line;
    const uint32_t row_blocks = (uint32_t)s.cov_cols * bpm;
    if (bpm == 0 || bpm > (uint32_t)kMaxBlocksPerMcu || wk.first >= row_blocks || wk.row >= s.cov_rows || wk.first % bpm != 0) return;  // (never listed)
    const uint32_t per_wg = islow_blocks_per_wg(bpm);
    const uint32_t n = row_blocks - wk.first < per_wg ? row_blocks - wk.first : per_wg;  // whole MCUs
    const uint32_t mcu_y = (uint32_t)s.cov_y + wk.row;
    const uint32_t mcu_x0 = (uint32_t)s.cov_x + wk.first / bpm;  // the strip's first MCU
    const uint32_t first_block = (mcu_y * mpl + s.cov_x) * bpm + wk.first;  // in the scan's store (a frame has fewer than 2^32 blocks)

    // ---- 1. DMA: linear 16-byte slot c = k * 256 + tid (block c >> 3, slot c & 7) receives piece (slot ^ swizzle(block)) of its block
    {
        const uint8_t *coef_bytes = reinterpret_cast<const uint8_t *>(coefs + s.coef_off * 64);
        const uint32_t piece_off = ((tid & 7u) ^ ((tid >> 4) & 7u)) * 16u;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            uint32_t blk = k * 32u + (tid >> 3);
            blk = blk < n ? blk : n - 1;
            __builtin_amdgcn_global_load_lds((islow_gbl_void *)(coef_bytes + (uint64_t)(first_block + blk) * 128 + piece_off),
                                             (islow_lds_void *)(sh + (k * kIslowThreads + wave * 64) * 16), 16, 0, 0);
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
    uint32_t px[16];
    islow_block(sh + k_row * 128, (k_row >> 1) & 7u, sh_q + ci * 64, px);

    // ---- 3. what the scan did not reach is zero (K3: idct_output_body)
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

    // ---- 4. the samples, where K3's generic class puts them
    const DevScanComponent comp = s.comp[ci];
    const uint32_t hs = comp.hs, vs = comp.vs;
    const bool flush = s.kind == kScanFrameOnly;
    const uint32_t W = s.win_w, H = s.win_h, C = s.frame_components;
    const uint32_t wx = s.win_x, wy = s.win_y;
    const uint32_t max_h = s.max_h, max_v = s.max_v;
    // the strip: n_mcu MCUs side by side, 8 * max_v rows of `pitch` bytes
    const uint32_t n_mcu = n / bpm;
    const uint32_t rows = 8u * max_v, pitch = n_mcu * 8u * max_h * C;
    bool assembled = s.scan_components == C && rows * pitch <= kIslowStaging, inside = true;
    for (uint32_t c = 0; c < (uint32_t)s.scan_components && c < (uint32_t)kMaxScanComponents; c++) {
        assembled = assembled && (uint32_t)s.comp[c].h * s.comp[c].hs == max_h && (uint32_t)s.comp[c].v * s.comp[c].vs == max_v;
        inside = inside && s.comp[c].component_index < C;
    }
    if (!inside) return;  // (DeviceBatch::islow_taken: never; the whole workgroup leaves, in front of the barriers below)
    uint8_t *img = scratch + s.out_off;

    if (!assembled) {  // (workgroup-uniform)
        if (!active) return;
        const uint32_t x0 = flush ? (mcu_x * comp.h + s.blk_x[b]) * hs * 8 : (mcu_x * max_h + s.blk_x[b]) * 8;
        const uint32_t y0 = flush ? (mcu_y * comp.v + s.blk_y[b]) * vs * 8 : (mcu_y * max_v + s.blk_y[b]) * 8;
        uint8_t *at = img + comp.component_index;
#pragma unroll
        for (uint32_t r = 0; r < 8; r++) {
            for (uint32_t v = 0; v < vs; v++) {  // (one turn but for a replicated component)
                const uint32_t y = y0 + r * vs + v - wy;  // (above the window wraps to a large value)
                if (y >= H) continue;
                uint8_t *line = at + (uint64_t)y * W * C;
#pragma unroll
                for (uint32_t c = 0; c < 8; c++) {
                    const uint8_t u = (uint8_t)(px[2 * r + (c >> 2)] >> (8 * (c & 3u)));
                    for (uint32_t h = 0; h < hs; h++) {
                        const uint32_t x = x0 + c * hs + h - wx;
                        if (x < W) line[(uint64_t)x * C] = u;
                    }
                }
            }
        }
        return;
    }

    // every lane holds its samples: the staging becomes the strip.  (h * hs == max_h and v * vs == max_v: the block's place inside its MCU is
    // (blk_x * hs * 8, blk_y * vs * 8) in both kinds of scan, and the components' blocks cover the MCU's box exactly once each.)
    __syncthreads();
    if (active) {
        uint8_t *at = sh + (s.blk_y[b] * vs * 8u) * pitch + ((ml * max_h + s.blk_x[b] * hs) * 8u) * C + comp.component_index;
#pragma unroll
        for (uint32_t r = 0; r < 8; r++) {
            for (uint32_t v = 0; v < vs; v++) {
                uint8_t *line = at + (r * vs + v) * pitch;
#pragma unroll
                for (uint32_t c = 0; c < 8; c++) {
                    const uint8_t u = (uint8_t)(px[2 * r + (c >> 2)] >> (8 * (c & 3u)));
                    for (uint32_t h = 0; h < hs; h++) line[(c * hs + h) * C] = u;
                }
            }
        }
    }
    __syncthreads();
    // the strip's pixels [xs, xe) of the frame lie in the window; row r of the strip is line (mcu_y * max_v * 8 + r) of the frame
    const uint32_t sx0 = mcu_x0 * max_h * 8u, sx1 = sx0 + n_mcu * max_h * 8u;
    const uint32_t xs = sx0 > wx ? sx0 : wx, xe = sx1 < wx + W ? sx1 : wx + W;
    if (xs >= xe) return;
    const uint32_t len = (xe - xs) * C;  // bytes of a row's run
    const uint32_t* sh32 = reinterpret_cast<const uint32_t *>(sh);
    for (uint32_t r = 0; r < rows; r++) {
        const uint32_t y = mcu_y * max_v * 8u + r - wy;
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

hipError_t launch_islow(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const IslowWork *work, int n_work, const DevScanStatus *status,
                        const DevQuantTable *quant_pool, uint8_t *scratch) {
    if (n_work <= 0) return hipSuccess;
    if (scratch == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(islow_kernel, dim3((uint32_t)n_work), dim3(kIslowThreads), 0, stream, coefs, scans, work, status, quant_pool, scratch);
    return hipGetLastError();
}

}  // namespace jpgpu
