// jpeglibrary_amd/csrc/k3c_pixel.h -- what K3C (k3c_color.hip) and K3O (k3o_orient.hip) share beyond k3_pixel.h: the arithmetic of the colour kinds a
// file can declare, and the stores of one and of four samples of a plane.  Device code only.
#pragma once
#include "k3_pixel.h"

namespace jpgpu {

// round-to-nearest of x / 255 for 0 <= x <= 65025 (tests/test_color_cpu.py checks every x)
__device__ __forceinline__ uint32_t div255(uint32_t x) {
    const uint32_t t = x + 128u;
    return (t + (t >> 8)) >> 8;
}

// one pixel's samples s = s0 | s1 << 8 | s2 << 16 | s3 << 24 -> R | G << 8 | B << 16
__device__ __forceinline__ uint32_t color_pixel(uint32_t kind, uint32_t s, const YccRgbFactors &k) {
    if (kind == kColorRgb) return s & 0x00FFFFFFu;
    uint32_t c0 = s & 0xFFu, c1 = (s >> 8) & 0xFFu, c2 = (s >> 16) & 0xFFu;
    const uint32_t s3 = s >> 24;
    if (kind == kColorYcck) {  // RGB_U8's conversion of (s0, s1, s2), inverted
        // (chroma_terms' arithmetic written out: through the shared helper the five listings come out in another instruction order)
        const int32_t cb = (int32_t)c1 - 128, cr = (int32_t)c2 - 128, y = (int32_t)c0;
        c0 = 255u - clamp_u8_i32(y + ((k.cr_r * cr + 32768) >> 16));
        c1 = 255u - clamp_u8_i32(y + ((k.cb_g * cb + 32768 + k.cr_g * cr) >> 16));
        c2 = 255u - clamp_u8_i32(y + ((k.cb_b * cb + 32768) >> 16));
    }
    return div255(c0 * s3) | (div255(c1 * s3) << 8) | (div255(c2 * s3) << 16);
}

// Four bytes of one plane (w = u0 | u1 << 8 | ...) -> four samples at dst.  A plane starts at c * pixels samples, which is a multiple of
// nothing: the destination is aligned for one sample only, and the stores say so.
template <int FMT>
__device__ __forceinline__ void store_plane4(uint8_t *dst, uint32_t w, float scale, float bias) {
    if constexpr (FMT == kFmtRgbPlanarU8) {
        __builtin_memcpy(dst, &w, 4);
    } else {
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; j++) f[j] = affine_sample((w >> (8 * j)) & 0xFFu, scale, bias);
        if constexpr (FMT == kFmtRgbPlanarF32) {
            __builtin_memcpy(__builtin_assume_aligned(dst, 4), f, 16);
        } else {
            const half2v h[2] = {__builtin_convertvector(float2v{f[0], f[1]}, half2v), __builtin_convertvector(float2v{f[2], f[3]}, half2v)};
            __builtin_memcpy(__builtin_assume_aligned(dst, 2), h, 8);
        }
    }
}

// one sample of one plane (the last one to three pixels of a row or an image whose pixel count is no multiple of four)
template <int FMT>
__device__ __forceinline__ void store_plane1(uint8_t *plane, uint64_t i, uint32_t u, float scale, float bias) {
    if constexpr (FMT == kFmtRgbPlanarU8) plane[i] = (uint8_t)u;
    else if constexpr (FMT == kFmtRgbPlanarF32) reinterpret_cast<float *>(plane)[i] = affine_sample(u, scale, bias);
    else reinterpret_cast<_Float16 *>(plane)[i] = (_Float16)affine_sample(u, scale, bias);
}

}  // namespace jpgpu
