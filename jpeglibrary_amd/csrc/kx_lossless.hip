// jpeglibrary_amd/csrc/kx_lossless.hip -- KX: the turn of an image in the coefficient domain (include/jpgpu.h section (5), "Lossless transform").
// Between the decoder's entropy stage and the encoder's: every block of a turned image moves to its place in the turned MCU grid, and its 64
// coefficients are sign-flipped (a mirrored axis negates the odd frequencies along it) and, for orientations 5..8, transposed.  Nothing is
// dequantised, clamped or rounded: with c[v][u] the source block, the destination holds c'[v][u] = sx(u) sy(v) c[v][u] for 2..4 and
// c'[v][u] = sx(v) sy(u) c[u][v] for 5..8, sx / sy = -1 on the odd frequencies of a mirrored source axis.
//   One launch per run over a work list of kTurnBlocksPerWg destination blocks per entry.  A workgroup of 256 lanes takes 32 blocks at a time,
// eight lanes to a 128-byte block, one 16-byte piece (eight zig-zag positions) per lane: the piece is loaded from the SOURCE block, negated in
// registers against masks over the zig-zag index that are compile-time constants, and
//   2..4: stored as the same piece of the destination block;
//   5..8: parked in LDS at a block stride of kLdsBlockStride = 144 bytes (E1's staging stride), and behind ONE barrier every lane gathers the
//         eight coefficients of its DESTINATION piece from the parked block (the transposition is a fixed permutation of the zig-zag positions)
//         and stores them as one piece.
//   1:    (a window alone, "Window" of the same section) the straight road of 2..4 with an empty sign mask: no LDS, no barrier.
// A window is an offset and nothing else: the destination grid is the window's, and source_block() adds the window's first MCU to the
// destination MCU's place before it maps it to the source -- in the turned grid, so under 5..8 the origin's x runs along the source's y, and
// under a mirrored axis it counts from the far edge of the KEPT grid.  Blocks outside the window are never loaded.
// Every coefficient of the destination is read once and written once.  The source blocks of 5..8 lie a grid row apart (a destination row walks a source column):
// whole 128-byte lines, scattered.  LDS: the park is ds_write_b128 at 16-byte steps inside a block and 144 bytes between blocks -- consecutive
// slots, no conflict; the gather is eight 2-byte reads per lane whose addresses follow the zig-zag, eight lanes per block at 36 dwords between
// blocks (4 banks apart modulo 32): some of a group's 32 lanes meet on a bank, which the kernel, bound by its global bytes, does not pay for
// at the size of the park (one read per coefficient).
#include <hip/hip_runtime.h>

#include "kx_lossless.h"

namespace jpgpu {

namespace {

constexpr uint32_t kLdsBlockStride = 144;  // bytes

// zig-zag position -> natural index (v * 8 + u), ITU-T T.81 Figure A.6
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// bit k: zig-zag position k has an odd horizontal (u) / vertical (v) frequency
constexpr uint64_t odd_mask(bool vertical) {
    uint64_t m = 0;
    for (int k = 0; k < 64; k++)
        if (((vertical ? kNatural[k] >> 3 : kNatural[k]) & 1) != 0) m |= 1ull << k;
    return m;
}
constexpr uint64_t kOddU = odd_mask(false), kOddV = odd_mask(true);
// byte j of entry l: the zig-zag position of (u, v) where 8 l + j is the position of (v, u)
struct TransposeTable {
    uint64_t piece[8];
};
constexpr TransposeTable transpose_table() {
    uint8_t zz[64] = {};
    for (int k = 0; k < 64; k++) zz[kNatural[k]] = (uint8_t)k;
    TransposeTable t = {};
    for (int k = 0; k < 64; k++) {
        const int v = kNatural[k] >> 3, u = kNatural[k] & 7;
        t.piece[k >> 3] |= (uint64_t)zz[u * 8 + v] << (8 * (k & 7));
    }
    return t;
}
__device__ constexpr TransposeTable kTranspose = transpose_table();

// the eight coefficients of a piece, negated where `m` has their bit
__device__ __forceinline__ uint32_t negate_pair(uint32_t w, uint32_t m) {
    int32_t lo = (int32_t)(int16_t)(w & 0xFFFFu), hi = (int32_t)w >> 16;
    if (m & 1u) lo = -lo;
    if (m & 2u) hi = -hi;
    return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
}
__device__ __forceinline__ uint4 negate_piece(uint4 p, uint32_t m) {
    return uint4{negate_pair(p.x, m), negate_pair(p.y, m >> 2), negate_pair(p.z, m >> 4), negate_pair(p.w, m >> 6)};
}

// destination block d of the image -> its source block (the pixel table of the orientation section, in units of blocks)
__device__ __forceinline__ uint32_t source_block(const DevTurnImage &g, uint32_t d, bool transposes, bool flip_x, bool flip_y) {
    const uint32_t mcu = d / g.bpm, b = d - mcu * g.bpm;
    const uint32_t info = g.blk[b], c = info & 3u;
    const uint32_t h = g.src_h[c], v = g.src_v[c];
    const uint32_t dh = transposes ? v : h, dv = transposes ? h : v;
    const uint32_t my = mcu / g.dst_mcus_per_line, mx = mcu - my * g.dst_mcus_per_line;
    const uint32_t X = (mx + g.origin_mx) * dh + ((info >> 2) & 3u), Y = (my + g.origin_my) * dv + ((info >> 4) & 3u);
    const uint32_t ty = transposes ? X : Y, tx = transposes ? Y : X;
    const uint32_t by = flip_y ? g.kept_mcus_per_column * v - 1u - ty : ty;
    const uint32_t bx = flip_x ? g.kept_mcus_per_line * h - 1u - tx : tx;
    const uint32_t smy = by / v, smx = bx / h;
    return (smy * g.src_mcus_per_line + smx) * g.bpm + g.first_blk[c] + (by - smy * v) * h + (bx - smx * h);
}

__global__ __launch_bounds__(256) void lossless_turn_kernel(const DevTurnImage *__restrict__ images, const TurnWork *__restrict__ work,
                                                            const int16_t *__restrict__ src, int16_t *__restrict__ dst) {
    __shared__ __attribute__((aligned(16))) uint8_t park[kTurnBlocksPerWg * kLdsBlockStride];
    const TurnWork wk = work[blockIdx.x];
    const DevTurnImage &g = images[wk.image];
    const uint32_t o = g.orientation;
    const bool transposes = o >= 5u, flip_x = o == 2u || o == 3u || o == 7u || o == 8u, flip_y = o == 3u || o == 4u || o == 6u || o == 7u;
    const uint32_t piece = threadIdx.x & 7u, slot0 = threadIdx.x >> 3;
    const uint64_t mask = (flip_x ? kOddU : 0ull) ^ (flip_y ? kOddV : 0ull);  // (both: the sign of an odd-odd coefficient is kept)
    const uint32_t m = (uint32_t)(mask >> (8u * piece)) & 0xFFu;
    const uint4 *sblocks = reinterpret_cast<const uint4 *>(src) + g.src_off * 8u;
    uint4 *dblocks = reinterpret_cast<uint4 *>(dst) + g.dst_off * 8u;
    constexpr uint32_t kRounds = kTurnBlocksPerWg / 32u;
    uint4 p[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t d = wk.first + r * 32u + slot0;
        p[r] = uint4{0, 0, 0, 0};
        if (d < g.total_blocks) p[r] = sblocks[(uint64_t)source_block(g, d, transposes, flip_x, flip_y) * 8u + piece];
    }
    if (!transposes) {  // (the same for every lane of the workgroup)
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++) {
            const uint32_t d = wk.first + r * 32u + slot0;
            if (d < g.total_blocks) dblocks[(uint64_t)d * 8u + piece] = negate_piece(p[r], m);
        }
        return;
    }
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++)
        *reinterpret_cast<uint4 *>(park + (r * 32u + slot0) * kLdsBlockStride + piece * 16u) = negate_piece(p[r], m);
    __syncthreads();
    const uint64_t from = kTranspose.piece[piece];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint32_t d = wk.first + r * 32u + slot0;
        const uint16_t *blk = reinterpret_cast<const uint16_t *>(park + (r * 32u + slot0) * kLdsBlockStride);
        uint32_t w[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t lo = blk[(uint32_t)(from >> (16u * j)) & 63u], hi = blk[(uint32_t)(from >> (16u * j + 8u)) & 63u];
            w[j] = lo | (hi << 16);
        }
        if (d < g.total_blocks) dblocks[(uint64_t)d * 8u + piece] = uint4{w[0], w[1], w[2], w[3]};
    }
}

}  // namespace

hipError_t launch_lossless_turn(hipStream_t stream, const DevTurnImage *images, const TurnWork *work, int n_work, const int16_t *src, int16_t *dst) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(lossless_turn_kernel, dim3(n_work), dim3(256), 0, stream, images, work, src, dst);
    return hipGetLastError();
}

}  // namespace jpgpu
