// jpeglibrary_amd/csrc/kx_lossless.h -- KX (kx_lossless.hip): the descriptor of an image that is turned in the coefficient domain
// (include/jpgpu.h section (5), "Lossless transform") and the launch wrapper
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace jpgpu {

// One turned image.  Blocks are 64 int16 in zig-zag order, MCU after MCU; the source is the decoder's dense store, the destination the
// encoder's layout (DevEncImage.coef_off).  The source grid may be wider than what is turned (JPGPU_EDGE_TRIM drops the last MCU
// column or row of a mirrored axis): src_mcus_per_line is the stride of the store, kept_mcus_* the grid the orientation works on.  The
// destination may be a window of the turned grid ("Window" of the same section): origin_mx / origin_my is its first MCU in the turned grid,
// dst_mcus_* its size; without one the origin is (0, 0) and the destination is the whole turned grid.
struct alignas(16) DevTurnImage {
    uint64_t src_off, dst_off;  // first block of the image in the source / the destination store
    uint32_t orientation;       // 1..8 (1: a window alone -- blocks move, no coefficient changes)
    uint32_t bpm;               // blocks per MCU (the same before and after)
    uint32_t total_blocks;      // of the destination: dst_mcus_per_line * dst_mcus_per_column * bpm
    uint32_t src_mcus_per_line;
    uint32_t kept_mcus_per_line, kept_mcus_per_column;  // source MCUs that take part
    uint32_t dst_mcus_per_line, dst_mcus_per_column;    // = the kept ones, swapped for 5..8; of the window where there is one
    uint32_t origin_mx, origin_my;                      // the window's first MCU in the turned grid (destination MCUs)
    // block b of a DESTINATION MCU: component | x << 2 | y << 4 (its place inside the component's h' x v' blocks)
    uint8_t blk[16];
    uint8_t src_h[4], src_v[4];  // the component's factors in the source (the destination's are these, swapped for 5..8)
    uint8_t first_blk[4];        // the component's first block inside an MCU (the same before and after)
    uint8_t reserved[12];
};
static_assert(sizeof(DevTurnImage) % 16 == 0, "DevTurnImage must be a multiple of 16 bytes");

constexpr uint32_t kTurnBlocksPerWg = 256;  // destination blocks per work entry (a workgroup of 256 lanes takes 32 at a time)

struct TurnWork {
    uint32_t image;
    uint32_t first;  // first destination block
};

// One launch for every turned or cut image of a run: src -> dst, every coefficient of the destination read once and written once (source
// blocks outside a window are never loaded).
hipError_t launch_lossless_turn(hipStream_t stream, const DevTurnImage *images, const TurnWork *work, int n_work, const int16_t *src, int16_t *dst);

}  // namespace jpgpu
