// tools/microbench/k2_pairs/line_order.hip -- is K2 slowed down by the ORDER in which it writes its whole 128-byte lines?
// (round 6: with the pair lookup the wave's symbol steps fell by 37 % and huffman_decode_kernel did not get faster: per-wave
// cycle counters put 36 % of a wave's life into the flush and 12 % into the ring top-up, whose wait also covers the stores.)
// K2's order: a wave owns 64 consecutive restart intervals = one contiguous span of 64 x 24 blocks x 128 B = 192 KB, and every
// block step writes ONE line in each of the 64 intervals -- 64 lines at a stride of 3 KB; the neighbours of a line arrive one block
// step (~6 us) later each, 24 steps to fill the span.  Variants, all writing the same bytes with the same wave / workgroup shape
// (11 waves, a workgroup per CU at a time because of LDS) and the same stand-in for the decode between two steps:
//   k2        the order above
//   stream    every step writes 64 CONSECUTIVE lines (8 KB) of the wave's span
//   pairs     every step writes 2 consecutive lines in each of 32 intervals (what staging two blocks per lane would give)
//   split     the half-line planes: the image's region is a lo plane and a hi plane of 64-byte slots, slot
//             (((i >> 1) * dri + m) * bpm + b) * 2 + (i & 1), so one line holds the same block of intervals 2p and 2p + 1.  Every step
//             writes its 32 whole lo lines (4 passes of 16 blocks x 4 chunks), the hi line of a pair only when a hash of the line
//             falls under `hi_permille` (exec-masked, both halves: whole lines only), and each chunk of 64 intervals ends with one
//             coalesced store of its 24 flag words.  Nothing but stores, like the other variants.
// Build: hipcc --offload-arch=gfx950 -O3 line_order.hip -o line_order ; run: ./line_order [delay] [n_images] [lds_kb] [hi_permille]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>

constexpr int kIntervals = 8100, kBlocksPerInterval = 24, kWaves = 11;

template <int MODE>
__global__ __launch_bounds__(64 * kWaves) void writer(uint8_t *out, int n_images, int delay, int lds_bytes, uint64_t *flags, uint32_t hi_cut) {
    extern __shared__ uint8_t smem[];
    const int wg_per_img = (kIntervals + 64 * kWaves - 1) / (64 * kWaves);
    const int img = blockIdx.x / wg_per_img;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = ((blockIdx.x % wg_per_img) * kWaves + wave) * 64;
    if (first >= kIntervals) return;
    if (lds_bytes > 64 && threadIdx.x == 0) smem[lds_bytes - 1] = 1;  // (touch: the allocation is what limits the CU to one workgroup)
    uint8_t *span = out + ((size_t)img * kIntervals + first) * kBlocksPerInterval * 128;
    const int n_own = kIntervals - first < 64 ? kIntervals - first : 64;
    uint4 v = {threadIdx.x, blockIdx.x, 3, 4};
    for (int step = 0; step < kBlocksPerInterval; step++) {
        float f = (float)v.x;
        for (int i = 0; i < delay; i++) f = f * 1.0001f + 0.5f;  // stand-in for decoding the block
        v.w = (uint32_t)f;
        if (MODE == 3) {
            uint8_t *lo = out + (size_t)img * kIntervals * kBlocksPerInterval * 128, *hi = lo + (size_t)kIntervals * kBlocksPerInterval * 64;
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const int blk = it * 16 + (lane >> 2), chunk = lane & 3;  // blk = 0..63: the interval of the wave; a line = blocks 2p, 2p + 1
                const uint32_t line = (uint32_t)((first + blk) >> 1) * kBlocksPerInterval + step;
                const size_t off = (size_t)line * 128 + (blk & 1) * 64 + chunk * 16;
                if (blk < n_own) *reinterpret_cast<uint4 *>(lo + off) = v;
                if (blk < n_own && (((uint32_t)img * 40503u + line) * 2654435761u >> 22) < hi_cut) *reinterpret_cast<uint4 *>(hi + off) = v;
            }
            continue;
        }
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int idx = it * 8 + (lane >> 3), chunk = lane & 7;  // idx = 0..63: which of the step's 64 lines
            size_t line;
            if (MODE == 0) line = (size_t)idx * kBlocksPerInterval + step;                                    // one line per interval
            else if (MODE == 1) line = (size_t)step * 64 + idx;                                               // 64 consecutive lines
            else line = (size_t)((step & 1) * 32 + (idx >> 1)) * kBlocksPerInterval + (step >> 1) * 2 + (idx & 1);  // 2 lines in 32 intervals
            if (line < (size_t)n_own * kBlocksPerInterval) *reinterpret_cast<uint4 *>(span + line * 128 + chunk * 16) = v;
        }
    }
    if (MODE == 3 && lane < kBlocksPerInterval)  // the chunk's flag words, one per (m, b): one coalesced store
        flags[((size_t)img * ((kIntervals + 63) / 64) + first / 64) * kBlocksPerInterval + lane] = ((uint64_t)v.w << 32) | v.x;
}

int main(int argc, char **argv) {
    const int delay = argc > 1 ? atoi(argv[1]) : 400;
    const int n_images = argc > 2 ? atoi(argv[2]) : 512;
    const size_t bytes = (size_t)n_images * kIntervals * kBlocksPerInterval * 128;
    uint8_t *d;
    if (hipMalloc(&d, bytes + 4096) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const int wg_per_img = (kIntervals + 64 * kWaves - 1) / (64 * kWaves);
    const int lds = argc > 3 ? atoi(argv[3]) * 1024 : 150 * 1024;  // (150 KB: one workgroup per CU, K2's occupancy)
    hipFuncSetAttribute(reinterpret_cast<const void *>(&writer<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void *>(&writer<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void *>(&writer<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void *>(&writer<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const int hi_permille = argc > 4 ? atoi(argv[4]) : 60;  // (97 % of the headline's blocks end inside zig-zag 0..31: ~6 % of the pairs)
    const uint32_t hi_cut = (uint32_t)hi_permille * 1024u / 1000u;
    uint64_t *flags;
    if (hipMalloc(&flags, (size_t)n_images * ((kIntervals + 63) / 64) * kBlocksPerInterval * 8) != hipSuccess) return 1;
    char split_name[64];
    snprintf(split_name, sizeof split_name, "split (lo + %d permille hi)", hi_permille);
    const char *names[4] = {"k2 (64 lines, 3 KB apart)", "stream (64 consecutive lines)", "pairs (2 lines x 32 intervals)", split_name};
    for (int mode = 0; mode < 4; mode++)
        for (int rep = 0; rep < 3; rep++) {
            hipEventRecord(e0);
            if (mode == 0) hipLaunchKernelGGL(writer<0>, dim3(n_images * wg_per_img), dim3(64 * kWaves), lds, 0, d, n_images, delay, lds, flags, hi_cut);
            if (mode == 1) hipLaunchKernelGGL(writer<1>, dim3(n_images * wg_per_img), dim3(64 * kWaves), lds, 0, d, n_images, delay, lds, flags, hi_cut);
            if (mode == 2) hipLaunchKernelGGL(writer<2>, dim3(n_images * wg_per_img), dim3(64 * kWaves), lds, 0, d, n_images, delay, lds, flags, hi_cut);
            if (mode == 3) hipLaunchKernelGGL(writer<3>, dim3(n_images * wg_per_img), dim3(64 * kWaves), lds, 0, d, n_images, delay, lds, flags, hi_cut);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            const double moved = mode == 3 ? bytes * (0.5 + 0.5 * (hi_cut / 1024.0)) + (double)n_images * ((kIntervals + 63) / 64) * kBlocksPerInterval * 8 : (double)bytes;
            if (rep == 2) printf("delay %5d  %-32s %8.3f ms  %7.1f GB/s\n", delay, names[mode], ms, moved / ms / 1e6);
        }
    return 0;
}
