// tools/microbench/k3_store_geometry.hip -- what does the GEOMETRY of K3's output stores cost, everything else held still?
//
// A kernel in the shape of idct_split_kernel<INTERLEAVED_U8, 4:2:0> on the headline (3840 x 2160, tiles of 40 MCUs): 256 threads,
// 49 728 bytes of LDS (three workgroups per CU), 16 tiles per workgroup.  Per tile: the staging's refill by LDS-DMA (30 720 bytes,
// 7.5 global_load_lds_dwordx4 per lane), the wait and a barrier, then 2.5 trips of the task loop -- two 16-byte LDS reads and three
// 16-byte stores per lane, 30 720 bytes out.  No transform, no byte permutes: only the addresses of the stores differ between the modes.
//
//   a         K3's own: a lane owns the 48 bytes of one MCU's pixel row, stores at +0 / +16 / +32; lanes 48 bytes apart
//   b-asc     quads: the four lanes of a quad own 192 contiguous bytes; store s writes pieces 4s .. 4s+3 of them, lane j piece 4s + j
//   b-perm    ... the same blocks, the pieces inside a block in the order of k3_store_quads.h (two lanes keep a register of their own)
//   c         the bound: the tile's 1 920 pieces of a pixel row taken in lane order, a wave writes 1 KB per instruction
//
// Every mode writes exactly the same bytes of the same buffer.  Build: hipcc --offload-arch=gfx950 -O3 k3_store_geometry.hip -o
// k3_store_geometry ; run: ./k3_store_geometry [images = 256] [refill in 2 KB units = 15] ; counters: a rocprofv3 --pmc pass of its own over the same program.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../jpeglibrary_amd/csrc/k3_store_quads.h"

constexpr uint32_t kMpl = 240, kMcuLines = 135, kTileMcus = 40, kTilesPerLine = kMpl / kTileMcus, kTilesPerWg = 16;
constexpr uint32_t kRowBytes = kMpl * 48;                 // one pixel line of the image: 3840 x 3
constexpr uint32_t kTileIn = 30720, kTileOut = kTileMcus * 16 * 48;  // both 30 720
constexpr uint32_t kLds = 49728, kThreads = 256;
static_assert(kTileOut == 30720 && kMpl % kTileMcus == 0, "the headline's geometry");

enum Mode { kLanes48 = 0, kQuadsAscending = 1, kQuadsPermuted = 2, kLaneLinear = 3 };

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

template <int MODE>
__global__ __launch_bounds__(kThreads, 3) void store_geometry(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t n_tiles, uint32_t refill_halves) {
    __shared__ __attribute__((aligned(16))) uint8_t sh[kLds];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t first = blockIdx.x * kTilesPerWg;
    auto dma = [&](uint32_t tile) {
        const uint8_t *src = in + (uint64_t)tile * kTileIn + tid * 16;
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (2 * (uint32_t)k + 1 < refill_halves || (2 * (uint32_t)k < refill_halves && tid < 128))  // (15 halves of 2 KB: K3's 7.5 instructions)
                __builtin_amdgcn_global_load_lds((gbl_void *)(src + (uint32_t)k * 4096), (lds_void *)(sh + ((uint32_t)k * kThreads + wave * 64) * 16), 16, 0, 0);
    };
    for (uint32_t i = 0; i < kTilesPerWg && first + i < n_tiles; i++) {
        const uint32_t tile = first + i;
        dma(tile);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const uint32_t gy0 = tile / kTilesPerLine, gx0 = (tile - gy0 * kTilesPerLine) * kTileMcus;  // (wave-uniform)
        uint8_t *line0 = out + (uint64_t)gy0 * 16 * kRowBytes + gx0 * 48;
        if (MODE == kLaneLinear) {
            for (uint32_t p = tid; p < kTileOut / 16; p += kThreads) {
                const uint32_t row = (p * 8739u) >> 20, col = p - row * 120u;  // p / 120 for p < 1920 (ceil(2^20 / 120): sixteen bits are too few)
                const uint4 v = *reinterpret_cast<const uint4 *>(sh + p * 16);
                *reinterpret_cast<uint4 *>(line0 + row * kRowBytes + col * 16) = v;
            }
        } else {
            for (uint32_t t = tid; t < 16 * kTileMcus; t += kThreads) {
                const uint32_t row = (t * 1639u) >> 16, m = t - row * kTileMcus;  // t / 40 for t < 640
                const uint4 yv = *reinterpret_cast<const uint4 *>(sh + t * 32);
                const uint4 cv = *reinterpret_cast<const uint4 *>(sh + t * 32 + 16);
                const uint4 o0 = yv, o1 = cv, o2 = {yv.x ^ cv.x, yv.y ^ cv.y, yv.z ^ cv.z, yv.w ^ cv.w};
                uint8_t *dst = line0 + row * kRowBytes + m * 48;
                if (MODE == kLanes48) {
                    *reinterpret_cast<uint4 *>(dst) = o0;
                    *reinterpret_cast<uint4 *>(dst + 16) = o1;
                    *reinterpret_cast<uint4 *>(dst + 32) = o2;
                } else {
                    // (40 MCUs, 256 threads: a quad never straddles a pixel row.)  A lane's three offsets from its own 48 bytes: ascending
                    // 16 * (4s + j) - 48 * j, permuted the header's -- a shift and a sign extension either way, nothing fetched
                    const uint32_t j = tid & 3u;
                    const uint32_t q0 = MODE == kQuadsAscending ? 0u - 32u * j : jpgpu::k3_quad_lane_offset(jpgpu::k3_quad_offsets_packed(0), j);
                    const uint32_t q1 = MODE == kQuadsAscending ? 64u - 32u * j : jpgpu::k3_quad_lane_offset(jpgpu::k3_quad_offsets_packed(1), j);
                    const uint32_t q2 = MODE == kQuadsAscending ? 128u - 32u * j : jpgpu::k3_quad_lane_offset(jpgpu::k3_quad_offsets_packed(2), j);
                    *reinterpret_cast<uint4 *>(dst + (int32_t)q0) = o0;
                    *reinterpret_cast<uint4 *>(dst + (int32_t)q1) = o1;
                    *reinterpret_cast<uint4 *>(dst + (int32_t)q2) = o2;
                }
            }
        }
        // (the next refill overwrites what this tile's tasks read)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
}

#define CHECK(x)                                                                 \
    do {                                                                         \
        hipError_t e_ = (x);                                                     \
        if (e_ != hipSuccess) {                                                  \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                  \
            return 1;                                                            \
        }                                                                        \
    } while (0)

template <int MODE>
static int run(const char *name, const uint8_t *in, uint8_t *out, uint32_t n_tiles, uint32_t n_wg, uint32_t refill_halves, hipEvent_t e0, hipEvent_t e1) {
    float ms[4];
    for (int rep = 0; rep < 4; rep++) {  // (the first is the warm-up)
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(store_geometry<MODE>, dim3(n_wg), dim3(kThreads), 0, 0, in, out, n_tiles, refill_halves);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms[rep], e0, e1));
    }
    const double gb = (double)n_tiles * (kTileOut + refill_halves * 2048.0) / 1e9;
    std::printf("%-7s %8.3f %8.3f %8.3f ms   %6.2f TB/s (read + write, best)\n", name, ms[1], ms[2], ms[3],
                gb / (ms[1] < ms[2] ? (ms[1] < ms[3] ? ms[1] : ms[3]) : (ms[2] < ms[3] ? ms[2] : ms[3])));
    return 0;
}

int main(int argc, char **argv) {
    const uint32_t n_images = argc > 1 ? (uint32_t)atoi(argv[1]) : 256u;
    const uint32_t refill_halves = argc > 2 ? (uint32_t)atoi(argv[2]) : 15u;  // the refill in units of 2 KB: 15 = K3's 30 720 bytes, 0 = none
    if (n_images == 0 || n_images > 1024 || refill_halves > 15) return 2;
    const uint32_t n_tiles = n_images * kMcuLines * kTilesPerLine, n_wg = (n_tiles + kTilesPerWg - 1) / kTilesPerWg;
    const size_t out_bytes = (size_t)n_tiles * kTileOut, in_bytes = (size_t)n_tiles * kTileIn;
    uint8_t *in, *out;
    CHECK(hipMalloc(&in, in_bytes));
    CHECK(hipMalloc(&out, out_bytes));
    CHECK(hipMemset(in, 1, in_bytes));
    CHECK(hipMemset(out, 0, out_bytes));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::printf("%u images, %u tiles, %u workgroups, refill %u bytes per tile: %.2f GB in, %.2f GB out\n", n_images, n_tiles, n_wg, refill_halves * 2048, n_tiles * (refill_halves * 2048.0) / 1e9, out_bytes / 1e9);
    for (int round = 0; round < 2; round++) {  // (twice, the modes alternating: the drift of the box over the run shows)
        if (run<kLanes48>("a", in, out, n_tiles, n_wg, refill_halves, e0, e1)) return 1;
        if (run<kQuadsAscending>("b-asc", in, out, n_tiles, n_wg, refill_halves, e0, e1)) return 1;
        if (run<kQuadsPermuted>("b-perm", in, out, n_tiles, n_wg, refill_halves, e0, e1)) return 1;
        if (run<kLaneLinear>("c", in, out, n_tiles, n_wg, refill_halves, e0, e1)) return 1;
    }
    CHECK(hipDeviceSynchronize());
    return 0;
}
