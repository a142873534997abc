// jpeglibrary_amd/csrc/k3u_upsample.hip -- K3U: libjpeg's "fancy" (triangle) chroma upsampling for the images that are filtered under
// JPGPU_UPSAMPLE_FANCY (include/jpgpu.h, "Chroma upsampling"; k3u_taps.h has the taps, the biases and the fetch rectangle).  Such an image
// takes K3's generic class, which leaves the replicated INTERLEAVED_U8 samples of its fetch rectangle in the scratch image: native chroma
// sample (i, j) is read back at pixel (i * hs, j * vs) of the frame.  One launch per sink: blockIdx.y = image (its descriptor in HBM, like
// K3C and K3O), blockIdx.x = a tile of kFancyTileW x kFancyTileH pixels of the OUTPUT window.  A workgroup of 256
//   1. loads the native chroma samples its tile's taps touch -- the tile's columns and rows plus one per side, clamped to the plane's REAL
//      extent -- one dword load per sample, and parks them in LDS as Cb | Cr << 16,
//   2. behind a barrier forms the column sums 3 * near + far of every output row ONCE per chroma column (vs == 2; both halves of the dword at
//      once: no sum exceeds 16 * 255 + 8) and parks them, and behind a second barrier
//   3. gives every lane four neighbouring pixels of a row: one 12-byte load for their luma, the sums of their taps from LDS, the horizontal
//      step, the format's own conversion (rgb_pixel(chroma_terms), k3_pixel.h) and one store of 12 or 16 bytes, or four samples per plane
//      (K3C's stores).  The sixth sink stores (Y, Cb', Cr') instead, which K3O converts and turns.
// vs == 1 has no step 2: step 1 parks the samples where step 3 reads.  Scratch and output are different buffers; the staging slot lies behind
// the fetch rectangle in the scratch image, so no step reads what another workgroup writes.
// (A file of its own so that every other kernel object stays what it was.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "k3c_pixel.h"
#include "k3u_taps.h"

namespace jpgpu {

namespace {

constexpr int kSinkStaged = -1;  // SINK: an RGB format, or this
constexpr uint32_t kCols = kFancyTileW;            // chroma columns of a tile at most: hs == 1: 128; hs == 2: 64 + 2
// native rows of a tile at most (only vs == 2 parks them apart from the sums): a tile that starts on an odd line of the frame and ends on an
// even one touches kFancyTileH / 2 + 1 rows, one more lies above it (jbase), one below
constexpr uint32_t kNativeRows = kFancyTileH / 2 + 3;

// four pixels (R | G << 8 | B << 16 each; n of them real) -> the sink's samples of pixels [pixel, pixel + n) of an image of `plane` bytes per plane
template <int FMT>
__device__ __forceinline__ void store_quad(uint8_t *dst, uint64_t plane, uint64_t pixel, const uint32_t (&px)[4], uint32_t n, const OutputAffine &aff) {
    if constexpr (fmt_is_rgb_planes(FMT)) {
        constexpr uint32_t kSampleBytes = (uint32_t)fmt_rgb_plane_sample_bytes(FMT);
        if (n == 4) {
            const uint32_t lo_rg = pick4(px[0], px[1], JPGPU_SEL(0, 4, 1, 5)), hi_rg = pick4(px[2], px[3], JPGPU_SEL(0, 4, 1, 5));
            const uint32_t r = pick4(lo_rg, hi_rg, JPGPU_SEL(0, 1, 4, 5)), gr = pick4(lo_rg, hi_rg, JPGPU_SEL(2, 3, 6, 7));
            const uint32_t b = pick4(pick4(px[0], px[1], JPGPU_SEL(2, 6, 12, 12)), pick4(px[2], px[3], JPGPU_SEL(2, 6, 12, 12)), JPGPU_SEL(0, 1, 4, 5));
            uint8_t *d = dst + pixel * kSampleBytes;
            store_plane4<FMT>(d, r, aff.scale[0], aff.bias[0]);
            store_plane4<FMT>(d + plane, gr, aff.scale[1], aff.bias[1]);
            store_plane4<FMT>(d + 2 * plane, b, aff.scale[2], aff.bias[2]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 3; j++) {
                if (j >= n) break;
#pragma unroll
                for (int c = 0; c < 3; c++) store_plane1<FMT>(dst + (uint64_t)c * plane, pixel + j, (px[j] >> (8 * c)) & 0xFFu, aff.scale[c], aff.bias[c]);
            }
        }
    } else if constexpr (FMT == kFmtRgbaU8) {  // (4 bytes per pixel from a multiple of 256: every pixel is an aligned dword, a quad is not)
        uint8_t *d = dst + pixel * 4;
        if (n == 4) {
            const uint4 w = {px[0] | 0xFF000000u, px[1] | 0xFF000000u, px[2] | 0xFF000000u, px[3] | 0xFF000000u};
            __builtin_memcpy(d, &w, 16);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 3; j++)
                if (j < n) reinterpret_cast<uint32_t *>(d)[j] = px[j] | 0xFF000000u;
        }
    } else {  // RGB_U8 and the staged samples: four pixels -> three dwords, at any byte address
        uint8_t *d = dst + pixel * 3;
        if (n == 4) {
            const uint32_t w[3] = {pick4(px[0], px[1], JPGPU_SEL(0, 1, 2, 4)), pick4(px[1], px[2], JPGPU_SEL(1, 2, 4, 5)), pick4(px[2], px[3], JPGPU_SEL(2, 4, 5, 6))};
            __builtin_memcpy(d, w, 12);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 3; j++) {
                if (j >= n) break;
                d[3 * j] = (uint8_t)px[j];
                d[3 * j + 1] = (uint8_t)(px[j] >> 8);
                d[3 * j + 2] = (uint8_t)(px[j] >> 16);
            }
        }
    }
}

template <int SINK>
__global__ __launch_bounds__(256) void fancy_upsample_kernel(const uint8_t *__restrict__ scratch, uint8_t *__restrict__ out, const FancyImage *__restrict__ images,
                                                             YccRgbFactors kf, OutputAffine aff) {
    __shared__ uint32_t native[kNativeRows][kCols];
    __shared__ uint32_t sums[kFancyTileH][kCols];
    const FancyImage g = images[blockIdx.y];
    if ((g.staged != 0) != (SINK == kSinkStaged)) return;  // (the other launch's image; the whole workgroup leaves)
    const uint32_t tiles_x = (g.win_w + kFancyTileW - 1) / kFancyTileW, tiles_y = (g.win_h + kFancyTileH - 1) / kFancyTileH;
    if (blockIdx.x >= tiles_x * tiles_y) return;  // (the grid is the largest image's)
    const uint32_t ty = blockIdx.x / tiles_x, X0 = (blockIdx.x - ty * tiles_x) * kFancyTileW, Y0 = ty * kFancyTileH;
    const uint32_t tw = min(kFancyTileW, g.win_w - X0), th = min(kFancyTileH, g.win_h - Y0);  // the tile's part of the window
    const uint32_t xf0 = g.win_x + X0, yf0 = g.win_y + Y0;                                    // ... and its place in the frame
    const uint32_t hs = g.hs, vs = g.vs;
    // the native samples of the tile: columns [ibase, ibase + nc), rows [jbase, jbase + nr); an index outside the plane is clamped into it when
    // the sample is loaded, so that the clamped taps of k3u_tap() and the unclamped neighbours name the same value
    const int32_t ibase = hs == 2 ? (int32_t)(xf0 >> 1) - 1 : (int32_t)xf0, jbase = vs == 2 ? (int32_t)(yf0 >> 1) - 1 : (int32_t)yf0;
    const uint32_t nc = hs == 2 ? ((xf0 + tw - 1) >> 1) + 2 - (uint32_t)ibase : tw, nr = vs == 2 ? ((yf0 + th - 1) >> 1) + 2 - (uint32_t)jbase : th;
    const uint8_t *src = scratch + g.src_off;

    // ---- 1: a lane per native column, two rows per pass
    {
        const uint32_t c = threadIdx.x & (kCols - 1), r0 = threadIdx.x / kCols;
        const uint32_t i = (uint32_t)min(max(ibase + (int32_t)c, 0), (int32_t)g.cw - 1);
        const uint8_t *col = src + (uint64_t)(i * hs - g.fetch_x) * 3;
        for (uint32_t r = r0; r < nr && c < nc; r += 256 / kCols) {
            const uint32_t j = (uint32_t)min(max(jbase + (int32_t)r, 0), (int32_t)g.ch - 1);
            uint32_t w;  // Y, Cb, Cr and the next pixel's Y (the byte behind the fetch rectangle's last pixel is the slot's own or its slack)
            __builtin_memcpy(&w, col + (uint64_t)(j * vs - g.fetch_y) * g.fetch_w * 3, 4);
            const uint32_t cbcr = ((w >> 8) & 0xFFu) | ((w >> 16) & 0xFFu) << 16;
            if (vs == 2) native[r][c] = cbcr;
            else sums[r][c] = cbcr;
        }
    }
    __syncthreads();

    // ---- 2: the column sums of every output row of the tile
    if (vs == 2) {
        const uint32_t c = threadIdx.x & (kCols - 1), r0 = threadIdx.x / kCols;
        for (uint32_t r = r0; r < th && c < nc; r += 256 / kCols) {
            const K3uTap t = k3u_tap(yf0 + r, g.ch);
            sums[r][c] = 3u * native[(int32_t)t.near - jbase][c] + native[(int32_t)t.far - jbase][c];
        }
        __syncthreads();
    }

    // ---- 3: four neighbouring pixels of a row per lane; a wave takes two rows of the tile
    uint8_t *dst = out + g.dst_off;
    const uint64_t plane = (uint64_t)g.win_w * g.win_h * (uint64_t)(SINK == kSinkStaged ? 1 : fmt_rgb_plane_sample_bytes(SINK));
    const uint32_t quad = threadIdx.x & 31u, shift = k3u_shift(hs, vs);
#pragma unroll
    for (uint32_t k = 0; k < kFancyTileH / 8; k++) {
        const uint32_t r = (threadIdx.x >> 5) + 8 * k, X = 4 * quad;
        if (r >= th || X >= tw) continue;
        const uint32_t n = min(4u, tw - X), xf = xf0 + X, yf = yf0 + r;
        uint32_t y[3];  // twelve bytes: the luma of four pixels among them (behind the row's last pixel: the next row, or the slot's slack)
        __builtin_memcpy(y, src + ((uint64_t)(yf - g.fetch_y) * g.fetch_w + (xf - g.fetch_x)) * 3, 12);
        const uint32_t luma[4] = {y[0] & 0xFFu, y[0] >> 24, (y[1] >> 16) & 0xFFu, (y[2] >> 8) & 0xFFu};
        const uint32_t *row = sums[r];
        uint32_t px[4];
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) {
            uint32_t v;
            if (hs == 2) {
                const K3uTap t = k3u_tap(xf + m, g.cw);
                v = 3u * row[(int32_t)t.near - ibase] + row[(int32_t)t.far - ibase];
            } else {
                v = row[X + m];
            }
            v = ((v + k3u_bias(hs, vs, xf + m, yf) * 0x00010001u) >> shift) & 0x00FF00FFu;  // Cb' | Cr' << 16
            if (m >= n) v = 0x00800080u;  // (a pixel behind the window: its taps may lie outside the tile's columns; never stored)
            if constexpr (SINK == kSinkStaged) px[m] = luma[m] | (v & 0xFFu) << 8 | (v >> 16) << 16;
            else px[m] = rgb_pixel(luma[m], chroma_terms(v & 0xFFu, v >> 16, kf));
        }
        const uint64_t pixel = (uint64_t)(Y0 + r) * g.win_w + X0 + X;  // of the output window
        store_quad<(SINK == kSinkStaged ? (int)kFmtRgbU8 : SINK)>(dst, plane, pixel, px, n, aff);
    }
}

}  // namespace

hipError_t launch_fancy_upsample(hipStream_t stream, const uint8_t *scratch, uint8_t *out, uint8_t *staging, const FancyImage *images, int n_images,
                                 int n_staged, uint32_t max_tiles, int format, const YccRgbFactors &kf, const OutputAffine &aff) {
    if (n_images <= 0 || max_tiles == 0) return hipSuccess;
    if (!fmt_is_rgb(format)) return hipErrorInvalidValue;
    for (int base = 0; base < n_images; base += 65535) {  // grid.y limit
        const dim3 grid(max_tiles, (uint32_t)std::min(n_images - base, 65535));
        if (n_staged > 0) hipLaunchKernelGGL(fancy_upsample_kernel<kSinkStaged>, grid, dim3(256), 0, stream, scratch, staging, images + base, kf, aff);
        if (n_staged >= n_images) continue;  // (every image is turned afterwards: nothing goes to the output from here)
        switch (format) {
        case kFmtRgbU8: hipLaunchKernelGGL(fancy_upsample_kernel<kFmtRgbU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbaU8: hipLaunchKernelGGL(fancy_upsample_kernel<kFmtRgbaU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbPlanarU8: hipLaunchKernelGGL(fancy_upsample_kernel<kFmtRgbPlanarU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbPlanarF16: hipLaunchKernelGGL(fancy_upsample_kernel<kFmtRgbPlanarF16>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        default: hipLaunchKernelGGL(fancy_upsample_kernel<kFmtRgbPlanarF32>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        }
    }
    return hipGetLastError();
}

}  // namespace jpgpu
