// jpeglibrary_amd/csrc/k3_pixel.h -- the pixel helpers K3 (k3_idct.hip) and K3C (k3c_color.hip) share: byte gathers, the YCbCr -> RGB terms and
// the affine step of the float samples.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace jpgpu {

typedef float float2v __attribute__((ext_vector_type(2)));
typedef short short2v __attribute__((ext_vector_type(2)));
typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// byte gather from the 8 bytes {lo (indices 0-3), hi (indices 4-7)}, index 12 = a zero byte: one v_perm_b32
__device__ __forceinline__ uint32_t pick4(uint32_t lo, uint32_t hi, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#define JPGPU_SEL(a, b, c, d) ((uint32_t)(a) | ((uint32_t)(b) << 8) | ((uint32_t)(c) << 16) | ((uint32_t)(d) << 24))

// ---- YCbCr -> RGB(A) (ref: apps/JpegDecode/JpegYCbCrToRgbConverter.cs:134-206).  The reference looks the terms up in
// tables built by Init (:66-118); with ReferenceBlackWhite = {0,255,128,255,128,255} the tables are exactly
//   yTable[i] = i, crRTable[i] = (cr_r * (i-128) + half) >> 16, cbBTable[i] = (cb_b * (i-128) + half) >> 16,
//   crGTable[i] = cr_g * (i-128), cbGTable[i] = cb_g * (i-128) + half,  and the clamp table is a clamp to [0, 255],
// so the terms are computed instead of fetched (the factors come from the host, derived like Init derives them).
struct ChromaTerms {
    int32_t r, g, b;
};
__device__ __forceinline__ ChromaTerms chroma_terms(uint32_t cb_sample, uint32_t cr_sample, const YccRgbFactors &k) {
    const int32_t cb = (int32_t)cb_sample - 128, cr = (int32_t)cr_sample - 128;
    ChromaTerms t;
    t.r = (k.cr_r * cr + 32768) >> 16;
    t.b = (k.cb_b * cb + 32768) >> 16;
    t.g = (k.cb_g * cb + 32768 + k.cr_g * cr) >> 16;
    return t;
}
__device__ __forceinline__ uint32_t clamp_u8_i32(int32_t v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
// one pixel: R | G << 8 | B << 16
__device__ __forceinline__ uint32_t rgb_pixel(uint32_t y, const ChromaTerms &t) {
    return clamp_u8_i32((int32_t)y + t.r) | (clamp_u8_i32((int32_t)y + t.g) << 8) | (clamp_u8_i32((int32_t)y + t.b) << 16);
}

// RGB_PLANAR_F16 / _F32: a byte u of channel c becomes (float)u * scale[c] + bias[c]: one float32 multiply and one float32 add, each rounded
// to nearest even and never fused (__fmul_rn / __fadd_rn)
__device__ __forceinline__ float affine_sample(uint32_t u, float scale, float bias) { return __fadd_rn(__fmul_rn((float)u, scale), bias); }

}  // namespace jpgpu
