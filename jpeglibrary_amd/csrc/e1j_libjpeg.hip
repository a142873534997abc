// jpeglibrary_amd/csrc/e1j_libjpeg.hip -- encoder stage E1J: pixels -> quantised zig-zag blocks with libjpeg's arithmetic
// (include/jpgpu.h 4d; the arithmetic itself: e1j_islow.h).  It takes the images planned with the integer transform
// (DevEncImage.arithmetic) and writes where stage E1 (encode_kernels.hip) writes for the others: block k of the image in encoding
// order at coef_off + k, so everything behind it -- statistics, code lengths, emit, stuffing -- runs unchanged.
//
// One wave per 16 MCUs, three steps:
//   gather     one MCU per round, lane = one position of the MCU's 8 x 8 chroma block: it reads the H x V pixels behind it (the
//              last column and row of the image replicated), converts them, leaves their luma samples and its own downsampled
//              chroma samples in LDS, one byte each, block by block.  Any address, any of the four pixel forms: byte loads.
//   transform  eight blocks per round, lane = (block, row): row pass in registers, transpose through LDS (72 dwords from block
//              to block: the eight lanes of a column read eight banks, four blocks fill a 32-lane half's 32 banks), then lane =
//              (block, column): column pass, quantisation by the multiply-high factors the workgroup left in LDS, the int16
//              results to their zig-zag places in LDS, and out as one 16-byte store per lane: 1 KB of consecutive records.
//   dummies    the blocks of an MCU outside their component's own grid (libjpeg transforms none of them): zero AC, the DC of the
//              block emitted before them in the MCU.  They are few (the right and bottom MCUs of an image): a pass of their own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpgpu.h"
#include "e1j_islow.h"
#include "encode_kernels.h"

namespace jpgpu {
namespace {

constexpr uint32_t kJMcus = 16;  // MCUs per wave (= workgroup)
constexpr uint32_t kJTs = 72u;   // transpose buffer: dwords from block to block
constexpr uint32_t kJStage = 144u;  // finished blocks on their way out: bytes from block to block (a position of eight blocks on eight banks)
// natural index -> zig-zag position
__device__ constexpr uint8_t kJZig[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                          41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                          46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct E1jLds {
    uint2 quant[2][64];               // {multiply-high factor, d / 2} by natural index: luma, chroma
    uint8_t smp[kJMcus * 6 * 64];     // samples: [MCU][block of the MCU][row][column]
    uint32_t t[8 * kJTs];             // eight blocks behind the row pass
    uint8_t stage[8 * kJStage];       // eight finished blocks, zig-zag int16
    int16_t dc[kJMcus * 6];           // quantised DC of every transformed block
    uint32_t edge[kJMcus];            // per MCU: bit 0 = its second luma column lies outside the grid, bit 1 = its second luma row
};

// The transform rounds and the dummy pass of one wave: n_blk = its MCUs x BPM blocks, `out` = the first of them.
template <int H, int V, int BPM>
__device__ __forceinline__ void e1j_transform(E1jLds &sh, uint32_t lane, uint32_t n_blk, uint4 *__restrict__ out) {
    constexpr uint32_t NY = BPM == 1 ? 1u : (uint32_t)(H * V);
    const uint32_t slot = lane >> 3, r = lane & 7u;
    uint32_t zoff[8];
#pragma unroll
    for (int k = 0; k < 8; k++) zoff[k] = slot * kJStage + 2u * kJZig[k * 8 + r];
    // is block b of MCU m outside the luma grid?  (the first block of an MCU never is)
    auto dummy = [&](uint32_t m, uint32_t b) {
        if (b >= NY || NY == 1) return false;
        const uint32_t e = sh.edge[m];
        return ((e & 1u) != 0 && b % H == 1) || ((e & 2u) != 0 && b / H == 1);
    };
    for (uint32_t base = 0; base < n_blk; base += 8) {
        const bool active = base + slot < n_blk;
        const uint32_t j = active ? base + slot : n_blk - 1;
        const uint32_t m = j / BPM, b = j - m * BPM;
        // ---- row pass: lane = (block, row r)
        const uint2 raw = *reinterpret_cast<const uint2 *>(&sh.smp[j * 64 + r * 8]);
        int32_t d[8];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            d[k] = (int32_t)((raw.x >> (8 * k)) & 0xFFu) - 128;
            d[4 + k] = (int32_t)((raw.y >> (8 * k)) & 0xFFu) - 128;
        }
        e1j_fdct_pass<true>(d);
        uint4 *trow = reinterpret_cast<uint4 *>(&sh.t[slot * kJTs + r * 8]);
        trow[0] = make_uint4((uint32_t)d[0], (uint32_t)d[1], (uint32_t)d[2], (uint32_t)d[3]);
        trow[1] = make_uint4((uint32_t)d[4], (uint32_t)d[5], (uint32_t)d[6], (uint32_t)d[7]);
        __syncthreads();
        // ---- column pass: lane = (block, column r); d[k] = row k of the column
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = (int32_t)sh.t[slot * kJTs + k * 8 + r];
        e1j_fdct_pass<false>(d);
        const uint2 *quant = sh.quant[b < NY ? 0 : 1];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint2 q = quant[k * 8 + r];
            const int32_t v = e1j_quantise(d[k], q.x, q.y);
            *reinterpret_cast<int16_t *>(&sh.stage[zoff[k]]) = (int16_t)v;
            if (k == 0 && r == 0) sh.dc[j] = (int16_t)v;
        }
        __syncthreads();
        // ---- out: lane = (block, 16 bytes of its record)
        const uint4 piece = *reinterpret_cast<const uint4 *>(&sh.stage[slot * kJStage + r * 16]);
        if (active && !dummy(m, b)) out[(size_t)j * 8 + r] = piece;
    }
    if (NY == 1) return;
    __syncthreads();
    for (uint32_t j = lane; j < n_blk; j += 64) {
        const uint32_t m = j / BPM, b = j - m * BPM;
        if (!dummy(m, b)) continue;
        uint32_t src = b - 1;
        while (dummy(m, src)) src--;
        out[(size_t)j * 8] = make_uint4((uint32_t)(uint16_t)sh.dc[m * BPM + src], 0u, 0u, 0u);
#pragma unroll
        for (int k = 1; k < 8; k++) out[(size_t)j * 8 + k] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// H x V = the luma sampling factors of a three-component image; a one-component image is planned 1 x 1 and takes that instance.
template <int H, int V>
__global__ __launch_bounds__(64) void e1j_fdct_kernel(const uint8_t *__restrict__ pixels, const DevEncImage *__restrict__ images,
                                                      const EncWork *__restrict__ work, int16_t *__restrict__ coefs) {
    __shared__ __attribute__((aligned(16))) E1jLds sh;
    constexpr uint32_t kWaves = kEncMcusPerWg / kJMcus;
    const EncWork wk = work[blockIdx.x / kWaves];
    const DevEncImage &im = images[wk.image];
    // (uniform: stage E1, or another instance of this kernel, takes the image)
    if (im.arithmetic != JPGPU_ARITHMETIC_LIBJPEG || im.layout != 0 || im.luma_h != (uint32_t)H || im.luma_v != (uint32_t)V) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t mpl = im.mcus_per_line, total_mcus = mpl * im.mcus_per_column;
    const uint32_t first = wk.first + (blockIdx.x % kWaves) * kJMcus;
    if (first >= total_mcus) return;
    const uint32_t n_mcus = total_mcus - first < kJMcus ? total_mcus - first : kJMcus;
    const uint32_t width = im.width, height = im.height;
    const bool three = im.components == 3, rgb = im.input_rgb != 0;
    const uint32_t bpm = three ? (uint32_t)(H * V + 2) : 1u;

    // the divisors in use, once per workgroup
    for (uint32_t t = 0; t < (three ? 2u : 1u); t++) {
        const uint32_t q = im.quant[t][kJZig[lane]];
        sh.quant[t][lane] = make_uint2(e1j_mulhi_factor(q), (q << 3) >> 1);
    }

    // ---- gather
    const uint8_t *px = pixels + im.px_off;
    // sample c of pixel (x, y) is byte y * row_step + x * pixel_step + c * sample_step
    const uint32_t pixel_step = im.px_planar ? 1u : im.in_components;
    const size_t sample_step = im.px_planar ? (size_t)im.plane_stride : 1u, row_step = (size_t)width * pixel_step;
    const uint32_t cx = lane & 7u, cy = lane >> 3;
    const uint32_t last_chroma_row = (height + V - 1) / V - 1;
    const uint32_t luma_w = (width + 7) / 8, luma_h = (height + 7) / 8;
    uint32_t mx = first % mpl, my = first / mpl;
    for (uint32_t m = 0; m < n_mcus; m++) {
        uint8_t *smp = &sh.smp[m * bpm * 64];
        int32_t cb_sum = 0, cr_sum = 0;
#pragma unroll
        for (int j = 0; j < V; j++) {
            uint32_t y = (my * 8 + cy) * V + j;
            y = y < height ? y : height - 1;
            const uint8_t *row = px + (size_t)y * row_step;
#pragma unroll
            for (int i = 0; i < H; i++) {
                uint32_t x = (mx * 8 + cx) * H + i;
                x = x < width ? x : width - 1;
                const uint8_t *p = row + x * pixel_step;  // (below 2^18: 32 bits)
                int32_t s0 = p[0], s1 = 0, s2 = 0;
                if (three) {
                    s1 = p[sample_step];
                    s2 = p[2 * sample_step];
                    if (rgb) e1j_rgb_to_ycc(s0, s1, s2, s0, s1, s2);
                }
                const uint32_t lx = cx * H + i, ly = cy * V + j;
                smp[((ly >> 3) * H + (lx >> 3)) * 64 + (ly & 7u) * 8 + (lx & 7u)] = (uint8_t)s0;
                cb_sum += s1;
                cr_sum += s2;
            }
        }
        if (three) {
            // h2v2: bias 1, 2, 1, 2 ... along the row; h2v1: 0, 1, 0, 1 ...
            const int32_t bias = H * V == 4 ? 1 + (int32_t)(cx & 1u) : (H * V == 2 ? (int32_t)(cx & 1u) : 0);
            constexpr int kShift = H * V == 4 ? 2 : (H * V == 2 ? 1 : 0);
            smp[(H * V) * 64 + lane] = (uint8_t)((cb_sum + bias) >> kShift);
            smp[(H * V + 1) * 64 + lane] = (uint8_t)((cr_sum + bias) >> kShift);
            if (V == 2 && my * 8 + 7 > last_chroma_row) {
                // the chroma rows below the last one that has pixel rows of its own repeat THAT row, not the last pixel row
                __syncthreads();
                const uint32_t lr = last_chroma_row - my * 8;
                if (cy > lr) {
                    smp[(H * V) * 64 + lane] = smp[(H * V) * 64 + lr * 8 + cx];
                    smp[(H * V + 1) * 64 + lane] = smp[(H * V + 1) * 64 + lr * 8 + cx];
                }
            }
        }
        if (lane == 0) sh.edge[m] = (H == 2 && mx * 2 + 1 >= luma_w ? 1u : 0u) | (V == 2 && my * 2 + 1 >= luma_h ? 2u : 0u);
        if (++mx == mpl) {
            mx = 0;
            my++;
        }
    }
    __syncthreads();

    uint4 *out = reinterpret_cast<uint4 *>(coefs + (im.coef_off + (size_t)first * bpm) * 64);
    if (three) e1j_transform<H, V, H * V + 2>(sh, lane, n_mcus * bpm, out);
    else if (H * V == 1) e1j_transform<1, 1, 1>(sh, lane, n_mcus, out);
}

}  // namespace

hipError_t launch_fdct_libjpeg(hipStream_t stream, const uint8_t *pixels, const DevEncImage *images, const EncWork *work, int n_work,
                               int16_t *coefs, uint32_t shapes) {
    if (n_work <= 0) return hipSuccess;
    const dim3 grid(n_work * (kEncMcusPerWg / kJMcus));
    if (shapes & 1u) hipLaunchKernelGGL((e1j_fdct_kernel<2, 2>), grid, dim3(64), 0, stream, pixels, images, work, coefs);
    if (shapes & 2u) hipLaunchKernelGGL((e1j_fdct_kernel<2, 1>), grid, dim3(64), 0, stream, pixels, images, work, coefs);
    if (shapes & 4u) hipLaunchKernelGGL((e1j_fdct_kernel<1, 1>), grid, dim3(64), 0, stream, pixels, images, work, coefs);
    return hipGetLastError();
}

}  // namespace jpgpu
