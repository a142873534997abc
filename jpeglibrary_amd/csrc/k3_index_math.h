// jpeglibrary_amd/csrc/k3_index_math.h -- the index arithmetic of K3's tile loop without divisions (host + device: tests/test_k3_index_math_cpu.py
// enumerates every claim below against / and % on the CPU)
//
// K3 walks a scan tile by tile (at most 256 blocks = at most kK3MaxTileMcus MCUs of a YCbCr layout, 256 MCUs of a single-component one).
// The place of a tile's first MCU in the image, (gx0, gy0), is wave-uniform state carried from tile to tile by addition and one wrap;
// what a lane needs beyond it are quotients of small numbers, taken with a 24-bit multiply (v_mul_u32_u24) and a shift.
#pragma once
#include <stdint.h>

#ifndef JPGPU_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPGPU_HD __host__ __device__
#else
#define JPGPU_HD
#endif
#endif

namespace jpgpu {

constexpr uint32_t kK3MaxTileMcus = 85;      // MCUs of a tile of a three-component layout: 256 / 3
constexpr uint32_t kK3MaxTileLanes = 256;    // blocks (and, with one block per MCU, MCUs) of any tile
constexpr uint32_t kK3LineRecipBelow = 256;  // lines of fewer MCUs: a tile may wrap more than once, the wraps by reciprocal; others: one compare

// a * b of two values below 2^24 (the callers' ranges keep the product below 2^32)
JPGPU_HD inline uint32_t k3_mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return (a & 0xFFFFFFu) * (b & 0xFFFFFFu);
#endif
}

// task t of a tile of n_mcu MCUs (one task = one pixel row of one MCU): row = t / n_mcu.
// Exact for n_mcu = 1 .. kK3MaxTileMcus and t < 16 * n_mcu.  (Twenty bits: with sixteen, 77 MCUs are wrong from t = 1000 on.)
JPGPU_HD inline uint32_t k3_row_recip(uint32_t n_mcu) { return ((1u << 20) + n_mcu - 1u) / (n_mcu | (n_mcu == 0)); }
JPGPU_HD inline uint32_t k3_task_row(uint32_t t, uint32_t row_recip) { return k3_mul24(t, row_recip) >> 20; }

// MCU x = gx0 + (MCU of the tile) counted from the start of the tile's first MCU line, gx0 < mcus_per_line: the lines it lies below that one.
// Exact for x < mcus_per_line + kK3MaxTileLanes.
JPGPU_HD inline uint32_t k3_line_recip(uint32_t mcus_per_line) {
    return mcus_per_line < kK3LineRecipBelow ? ((1u << 20) + mcus_per_line - 1u) / (mcus_per_line | (mcus_per_line == 0)) : 0u;
}
JPGPU_HD inline uint32_t k3_line_wraps(uint32_t x, uint32_t mcus_per_line, uint32_t line_recip) {
    const uint32_t by_mul = k3_mul24(x, line_recip) >> 20, by_cmp = x >= mcus_per_line ? 1u : 0u;
    return mcus_per_line < kK3LineRecipBelow ? by_mul : by_cmp;
}

// The place of a tile's first MCU, and the step from one tile to the next (one division each per workgroup, none per tile).
struct K3TilePos {
    uint32_t gx0, gy0;
};
JPGPU_HD inline K3TilePos k3_tile_pos(uint32_t first_mcu, uint32_t mcus_per_line) {
    const uint32_t gy0 = first_mcu / mcus_per_line;
    return K3TilePos{first_mcu - gy0 * mcus_per_line, gy0};
}
JPGPU_HD inline void k3_tile_advance(K3TilePos &p, const K3TilePos &step, uint32_t mcus_per_line) {  // step = k3_tile_pos(mcus_per_tile, mcus_per_line)
    p.gx0 += step.gx0;
    p.gy0 += step.gy0;
    if (p.gx0 >= mcus_per_line) {
        p.gx0 -= mcus_per_line;
        p.gy0 += 1;
    }
}

}  // namespace jpgpu
