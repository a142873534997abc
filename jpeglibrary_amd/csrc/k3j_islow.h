// jpeglibrary_amd/csrc/k3j_islow.h -- one 8x8 block through libjpeg's integer transform (jidctint.c, jpeg_idct_islow) as K3J (k3j_islow.hip)
// runs it under JPGPU_ARITHMETIC_LIBJPEG: dequantisation as a 32-bit product, the column pass, the row pass, the two descales, the level shift
// and the clamp.  Host + device: tests/test_libjpeg_cpu.py builds a stand-alone program over this header and compares it with
// tests/islow_model.py sample for sample.  (include/jpgpu.h, "Arithmetic", has the function in full.)
//   Every sum and product is 32-bit two's complement and WRAPS: they are written in uint32_t, so neither the device nor the host code has a
// signed overflow.  The descales are arithmetic shifts of the wrapped value.  No float.
#pragma once
#include <stdint.h>

#include "k3_quant_order.h"

#ifndef JPGPU_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPGPU_HD __host__ __device__
#else
#define JPGPU_HD
#endif
#endif

namespace jpgpu {

// libjpeg's CONST_BITS = 13, PASS1_BITS = 2 and its twelve FIX() constants
constexpr uint32_t kIslowFix0_298631336 = 2446u, kIslowFix0_390180644 = 3196u, kIslowFix0_541196100 = 4433u, kIslowFix0_765366865 = 6270u,
                   kIslowFix0_899976223 = 7373u, kIslowFix1_175875602 = 9633u, kIslowFix1_501321110 = 12299u, kIslowFix1_847759065 = 15137u,
                   kIslowFix1_961570560 = 16069u, kIslowFix2_053119869 = 16819u, kIslowFix2_562915447 = 20995u, kIslowFix3_072711026 = 25172u;

// (x + 2^(n-1)) >> n of the wrapped 32-bit value x, the shift arithmetic
template <int N>
JPGPU_HD inline uint32_t islow_descale(uint32_t x) {
    return (uint32_t)((int32_t)(x + (1u << (N - 1))) >> N);
}

// The 1-D pass on eight values in place: the even part from (z2 + z3) * 4433, the odd part in the z1..z5 form, descaled by N bits.
template <int N>
JPGPU_HD inline void islow_pass(uint32_t &d0, uint32_t &d1, uint32_t &d2, uint32_t &d3, uint32_t &d4, uint32_t &d5, uint32_t &d6, uint32_t &d7) {
    uint32_t z1 = (d2 + d6) * kIslowFix0_541196100;
    const uint32_t e2 = z1 - d6 * kIslowFix1_847759065;
    const uint32_t e3 = z1 + d2 * kIslowFix0_765366865;
    const uint32_t e0 = (d0 + d4) << 13, e1 = (d0 - d4) << 13;
    const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    uint32_t t0 = d7, t1 = d5, t2 = d3, t3 = d1;
    z1 = t0 + t3;
    uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const uint32_t z5 = (z3 + z4) * kIslowFix1_175875602;
    t0 *= kIslowFix0_298631336;
    t1 *= kIslowFix2_053119869;
    t2 *= kIslowFix3_072711026;
    t3 *= kIslowFix1_501321110;
    z1 = 0u - z1 * kIslowFix0_899976223;
    z2 = 0u - z2 * kIslowFix2_562915447;
    z3 = 0u - z3 * kIslowFix1_961570560;
    z4 = 0u - z4 * kIslowFix0_390180644;
    z3 += z5;
    z4 += z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    d0 = islow_descale<N>(t10 + t3);
    d7 = islow_descale<N>(t10 - t3);
    d1 = islow_descale<N>(t11 + t2);
    d6 = islow_descale<N>(t11 - t2);
    d2 = islow_descale<N>(t12 + t1);
    d5 = islow_descale<N>(t12 - t1);
    d3 = islow_descale<N>(t13 + t0);
    d4 = islow_descale<N>(t13 - t0);
}

// clamp(v + 128, 0, 255) of the wrapped value v: what libjpeg's SIMD code does (its C code reads a table that wraps at +-512)
JPGPU_HD inline uint32_t islow_sample(uint32_t v) {
    const int32_t s = (int32_t)(v + 128u);
    return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

// One block.  coef: its 64 int16 coefficients in zig-zag order as eight pieces of 16 bytes, piece p at coef + ((p ^ swz) * 16) -- K3's
// swizzled LDS staging; swz = 0: a block as it lies in the store.  q: the component's 64 quantisers in zig-zag order (DevQuantTable::q).
// out[2 * r] = samples (r, 0..3), out[2 * r + 1] = samples (r, 4..7), one byte each, column 0 or 4 in the low byte.
JPGPU_HD inline void islow_block(const uint8_t *coef, uint32_t swz, const uint16_t *q, uint32_t (&out)[16]) {
    uint32_t ws[64];
    // pass 1: columns.  d = (int32)coef * (int32)q, int16 x uint16: no overflow
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; c++) {
        uint32_t d[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int r = 0; r < 8; r++) {
            const uint32_t k = kZigOfNat[r * 8 + c];
            const int16_t cv = *reinterpret_cast<const int16_t *>(coef + (((k >> 3) ^ swz) * 16u) + (k & 7u) * 2u);
            d[r] = (uint32_t)((int32_t)cv * (int32_t)q[k]);
        }
        islow_pass<11>(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int r = 0; r < 8; r++) ws[r * 8 + c] = d[r];
    }
    // pass 2: rows, then the level shift and the clamp
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 8; r++) {
        uint32_t *w = ws + r * 8;
        islow_pass<18>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
        out[2 * r] = islow_sample(w[0]) | (islow_sample(w[1]) << 8) | (islow_sample(w[2]) << 16) | (islow_sample(w[3]) << 24);
        out[2 * r + 1] = islow_sample(w[4]) | (islow_sample(w[5]) << 8) | (islow_sample(w[6]) << 16) | (islow_sample(w[7]) << 24);
    }
}

}  // namespace jpgpu
