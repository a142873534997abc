// jpeglibrary_amd/csrc/k3o_orient.hip -- K3O: the turn of the images whose orientation is not 1 (include/jpgpu.h, "Orientation").
// Such an image, whatever its colour kind, takes K3's generic class, which leaves the INTERLEAVED_U8 samples of its stored window in the scratch
// image; this kernel converts them like the formats' own paths do (GRAY replicated, YCBCR by the RGB_U8 terms, RGB / CMYK / YCCK by K3C's
// arithmetic) and writes them to the output slot in the five RGB forms, flipped and transposed as the orientation says.  Scratch and output are
// different buffers: the turn is out of place.  One launch per decode: blockIdx.y = image (its descriptor in HBM, like K3C), blockIdx.x = a tile
// of kOrientTile x kOrientTile pixels of the SOURCE window.  A workgroup of 256
//   1. loads its tile row by row -- a wave takes one row, its lanes neighbouring pixels of 1, 3 or 4 bytes --,
//   2. converts each pixel to R | G << 8 | B << 16,
//   3. parks the dwords in an LDS tile of pitch kPitch = 65 dwords, and behind ONE barrier
//   4. reads them in the destination's order, four neighbouring destination pixels per lane, and stores rows of the destination tile: 12 or
//      16 bytes per lane (RGB_U8, RGBA_U8), or four samples of each plane (K3C's stores, aligned for one sample only).
// Orientations 2..4 read the tile along its rows, 5..8 along its columns; the code is the same, with guards for edge tiles and images smaller
// than a tile.  LDS banks (ds_read_b32 / ds_write_b32: groups of 32 lanes, bank = dword address mod 32): step 3 writes 32 consecutive dwords per
// group; step 4 gives a group 4 destination rows x 8 quads, whose dword addresses are, modulo 32, row + 4 * quad + j along rows and
// (4 * quad + j) * 65 + row = 4 * quad + j + row along columns: 32 different banks either way, also when an index runs backwards.
// (A file of its own so that every other kernel object stays what it was.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "k3c_pixel.h"

namespace jpgpu {

namespace {

constexpr uint32_t kPitch = kOrientTile + 1;  // dwords

// Steps 1 to 3 for pixels of BPP bytes: the tile's sixteen loads of a lane are issued together -- a lane outside an edge tile reads the
// tile's last row or column instead and writes nothing -- then converted and parked.
template <uint32_t BPP>
__device__ __forceinline__ void load_tile(uint32_t *tile, const uint8_t *__restrict__ src, uint32_t width, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th,
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
        uint32_t px;
        if constexpr (BPP == 4) px = color_pixel(kind, s[k], kf);
        else if constexpr (BPP == 1) px = s[k] * 0x00010101u;
        else px = kind == kColorRgb ? s[k] : rgb_pixel(s[k] & 0xFFu, chroma_terms((s[k] >> 8) & 0xFFu, s[k] >> 16, kf));
        if (r < th && c < tw) tile[r * kPitch + c] = px;
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void orient_convert_kernel(const uint8_t *__restrict__ scratch, uint8_t *__restrict__ out,
                                                             const OrientImage *__restrict__ images, YccRgbFactors kf, OutputAffine aff) {
    __shared__ uint32_t tile[kOrientTile * kPitch];
    const OrientImage g = images[blockIdx.y];
    const uint32_t tiles_x = (g.width + kOrientTile - 1) / kOrientTile, tiles_y = (g.height + kOrientTile - 1) / kOrientTile;
    if (blockIdx.x >= tiles_x * tiles_y) return;  // (the grid is the largest image's; the whole workgroup leaves)
    const uint32_t ty = blockIdx.x / tiles_x, x0 = (blockIdx.x - ty * tiles_x) * kOrientTile, y0 = ty * kOrientTile;
    const uint32_t tw = min(kOrientTile, g.width - x0), th = min(kOrientTile, g.height - y0);  // the tile's part of the source window
    const uint32_t kind = g.kind;
    const uint32_t bpp = kind == kColorGray ? 1u : (kind == kColorCmyk || kind == kColorYcck ? 4u : 3u);
    const uint8_t *src = scratch + g.src_off;

    // ---- 1..3: a wave per source row, a lane per pixel
    if (bpp == 4) load_tile<4>(tile, src, g.width, x0, y0, tw, th, kind, kf);
    else if (bpp == 3) load_tile<3>(tile, src, g.width, x0, y0, tw, th, kind, kf);
    else load_tile<1>(tile, src, g.width, x0, y0, tw, th, kind, kf);
    __syncthreads();

    // ---- 4: the destination tile.  Along a destination row the source runs along a row (orientations 2..4) or a column (5..8) of the tile,
    // forwards or backwards.
    const uint32_t o = g.orientation;
    const bool transposed = o >= 5, flip_x = o == 2 || o == 3 || o == 7 || o == 8, flip_y = o == 3 || o == 4 || o == 6 || o == 7;
    const uint32_t rows = transposed ? tw : th, cols = transposed ? th : tw;  // of the destination tile
    const uint32_t dst_w = transposed ? g.height : g.width, dst_h = transposed ? g.width : g.height;
    // where the tile lands: a flipped axis counts from the far end
    const uint32_t sx = flip_x ? g.width - x0 - tw : x0, sy = flip_y ? g.height - y0 - th : y0;
    const uint32_t X0 = transposed ? sy : sx, Y0 = transposed ? sx : sy;
    // source index = base + step * (destination index), per axis of the destination
    const int32_t row_step = (int32_t)(transposed ? 1u : kPitch) * ((transposed ? flip_x : flip_y) ? -1 : 1);
    const int32_t col_step = (int32_t)(transposed ? kPitch : 1u) * ((transposed ? flip_y : flip_x) ? -1 : 1);
    const int32_t base = (row_step < 0 ? -row_step * (int32_t)(rows - 1) : 0) + (col_step < 0 ? -col_step * (int32_t)(cols - 1) : 0);
    uint8_t *dst = out + g.dst_off;
    constexpr uint32_t kSampleBytes = (uint32_t)fmt_rgb_plane_sample_bytes(FMT);
    const uint64_t plane = (uint64_t)dst_w * dst_h * kSampleBytes;
    // a group of 32 lanes = 4 destination rows x 8 quads; the wave's other group takes the next 8 quads of the same rows
    const uint32_t lane = threadIdx.x & 63u, quad = (lane & 7u) | ((lane >> 5) << 3), row_in_wave = (lane >> 3) & 3u;
#pragma unroll
    for (uint32_t k = 0; k < kOrientTile / 16; k++) {
        const uint32_t Y = 16 * k + 4 * (threadIdx.x >> 6) + row_in_wave, X = 4 * quad;
        if (Y >= rows || X >= cols) continue;
        const uint32_t n = min(4u, cols - X);
        const int32_t at = base + row_step * (int32_t)Y + col_step * (int32_t)X;
        uint32_t px[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) px[j] = j < n ? tile[at + col_step * (int32_t)j] : 0u;
        const uint64_t pixel = (uint64_t)(Y0 + Y) * dst_w + X0 + X;  // of the oriented output
        if constexpr (fmt_is_rgb_planes(FMT)) {
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
        } else {  // four pixels -> three dwords, at any byte address
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
}

}  // namespace

hipError_t launch_orient_convert(hipStream_t stream, const uint8_t *scratch, uint8_t *out, const OrientImage *images, int n_images, uint32_t max_tiles,
                                 int format, const YccRgbFactors &kf, const OutputAffine &aff) {
    if (n_images <= 0 || max_tiles == 0) return hipSuccess;
    if (!fmt_is_rgb(format)) return hipErrorInvalidValue;
    for (int base = 0; base < n_images; base += 65535) {  // grid.y limit
        const dim3 grid(max_tiles, (uint32_t)std::min(n_images - base, 65535));
        switch (format) {
        case kFmtRgbU8: hipLaunchKernelGGL(orient_convert_kernel<kFmtRgbU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbaU8: hipLaunchKernelGGL(orient_convert_kernel<kFmtRgbaU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbPlanarU8: hipLaunchKernelGGL(orient_convert_kernel<kFmtRgbPlanarU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbPlanarF16: hipLaunchKernelGGL(orient_convert_kernel<kFmtRgbPlanarF16>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        default: hipLaunchKernelGGL(orient_convert_kernel<kFmtRgbPlanarF32>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        }
    }
    return hipGetLastError();
}

}  // namespace jpgpu
