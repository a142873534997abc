// jpeglibrary_amd/csrc/k3r_reduced.h -- one 8x8 block of coefficients through libjpeg's reduced transforms (jidctred.c: jpeg_idct_4x4,
// jpeg_idct_2x2, jpeg_idct_1x1) as K3R (k3r_reduced.hip) runs them for an image decoded at 1/2, 1/4 or 1/8 size, and jdmaster.c's choice of a
// transform size per component.  Host + device: tests/test_scaled_cpu.py builds a stand-alone program over this header and compares it with
// tests/scaled_model.py sample for sample.  (include/jpgpu.h, "Scaled decode", has the function in full.)
//   As in k3j_islow.h every sum and product is 32-bit two's complement and WRAPS (written in uint32_t), the descales are arithmetic shifts
// of the wrapped value, and the sample is clamp(v + 128, 0, 255).  No float.
#pragma once
#include <stdint.h>

#include "k3j_islow.h"

namespace jpgpu {

// jidctred.c's FIX() constants that k3j_islow.h does not have already (FIX_0_765366865, FIX_0_899976223, FIX_1_847759065, FIX_2_562915447 are there)
constexpr uint32_t kRedFix0_211164243 = 1730u, kRedFix0_509795579 = 4176u, kRedFix0_601344887 = 4926u, kRedFix0_720959822 = 5906u,
                   kRedFix0_850430095 = 6967u, kRedFix1_061594337 = 8697u, kRedFix1_272758580 = 10426u, kRedFix1_451774981 = 11893u,
                   kRedFix2_172734803 = 17799u, kRedFix3_624509785 = 29692u;

// jdmaster.c (library version 62): the samples per block side of a component with factors h, v under the frame's maxima hmax, vmax, where
// the picture keeps m = 8 / denom of 8 pixels: m, doubled while that still divides the component's share of the reduced MCU both ways
JPGPU_HD inline uint32_t reduced_block_size(uint32_t m, uint32_t h, uint32_t v, uint32_t hmax, uint32_t vmax) {
    uint32_t s = m;
    while (s < 8u && (hmax * m) % (h * s * 2u) == 0u && (vmax * m) % (v * s * 2u) == 0u) s *= 2u;
    return s;
}
// ... and how often each of those samples is then repeated along an axis (max = hmax and f = h, or vmax and v)
JPGPU_HD inline uint32_t reduced_replication(uint32_t m, uint32_t s, uint32_t f, uint32_t max) { return max * m / (f * s); }

// the dequantised coefficient at row r, column c: (int32)coef * (int32)q, int16 x uint16; the block as islow_block takes it
JPGPU_HD inline uint32_t reduced_dequant(const uint8_t *coef, uint32_t swz, const uint16_t *q, int r, int c) {
    const uint32_t k = kZigOfNat[r * 8 + c];
    const int16_t cv = *reinterpret_cast<const int16_t *>(coef + (((k >> 3) ^ swz) * 16u) + (k & 7u) * 2u);
    return (uint32_t)((int32_t)cv * (int32_t)q[k]);
}

// jpeg_idct_4x4's 1-D pass: inputs 0, 1, 2, 3, 5, 6, 7 of a column or row (input 4 is never read) -> four outputs descaled by N bits
template <int N>
JPGPU_HD inline void reduced_pass4(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t d5, uint32_t d6, uint32_t d7, uint32_t (&o)[4]) {
    const uint32_t t0 = d0 << 14;
    const uint32_t t2 = d2 * kIslowFix1_847759065 - d6 * kIslowFix0_765366865;
    const uint32_t t10 = t0 + t2, t12 = t0 - t2;
    const uint32_t a = d5 * kRedFix1_451774981 + d1 * kRedFix1_061594337 - d7 * kRedFix0_211164243 - d3 * kRedFix2_172734803;
    const uint32_t b = d3 * kIslowFix0_899976223 + d1 * kIslowFix2_562915447 - d7 * kRedFix0_509795579 - d5 * kRedFix0_601344887;
    o[0] = islow_descale<N>(t10 + b);
    o[1] = islow_descale<N>(t12 + a);
    o[2] = islow_descale<N>(t12 - a);
    o[3] = islow_descale<N>(t10 - b);
}

// jpeg_idct_2x2's 1-D pass: inputs 0, 1, 3, 5, 7 -> two outputs descaled by N bits
template <int N>
JPGPU_HD inline void reduced_pass2(uint32_t d0, uint32_t d1, uint32_t d3, uint32_t d5, uint32_t d7, uint32_t (&o)[2]) {
    const uint32_t t10 = d0 << 15;
    const uint32_t t0 = d5 * kRedFix0_850430095 + d1 * kRedFix3_624509785 - d7 * kRedFix0_720959822 - d3 * kRedFix1_272758580;
    o[0] = islow_descale<N>(t10 + t0);
    o[1] = islow_descale<N>(t10 - t0);
}

#if defined(__HIP_DEVICE_COMPILE__)
#define JPGPU_K3R_UNROLL _Pragma("unroll")
#else
#define JPGPU_K3R_UNROLL
#endif

// The three transforms.  coef, swz, q: as islow_block takes them.  out[2 * r] = samples (r, 0..3) of the s x s block, one byte each, column 0
// in the low byte -- islow_block's layout, of which a 4 x 4 block fills the even entries 0..6, a 2 x 2 block half of entries 0 and 2, a 1 x 1
// block a byte of entry 0.  Entries the block does not fill are not written.
JPGPU_HD inline void reduced_block4(const uint8_t *coef, uint32_t swz, const uint16_t *q, uint32_t (&out)[16]) {
    uint32_t ws[4][8];  // workspace rows 0..3; column 4 stays unused
    JPGPU_K3R_UNROLL
    for (int c = 0; c < 8; c++) {
        if (c == 4) continue;
        uint32_t o[4];
        reduced_pass4<12>(reduced_dequant(coef, swz, q, 0, c), reduced_dequant(coef, swz, q, 1, c), reduced_dequant(coef, swz, q, 2, c),
                          reduced_dequant(coef, swz, q, 3, c), reduced_dequant(coef, swz, q, 5, c), reduced_dequant(coef, swz, q, 6, c),
                          reduced_dequant(coef, swz, q, 7, c), o);
        JPGPU_K3R_UNROLL
        for (int r = 0; r < 4; r++) ws[r][c] = o[r];
    }
    JPGPU_K3R_UNROLL
    for (int r = 0; r < 4; r++) {
        uint32_t o[4];
        reduced_pass4<19>(ws[r][0], ws[r][1], ws[r][2], ws[r][3], ws[r][5], ws[r][6], ws[r][7], o);
        out[2 * r] = islow_sample(o[0]) | (islow_sample(o[1]) << 8) | (islow_sample(o[2]) << 16) | (islow_sample(o[3]) << 24);
    }
}

JPGPU_HD inline void reduced_block2(const uint8_t *coef, uint32_t swz, const uint16_t *q, uint32_t (&out)[16]) {
    uint32_t ws[2][8];  // workspace rows 0, 1; columns 0, 1, 3, 5, 7 are used
    JPGPU_K3R_UNROLL
    for (int c = 0; c < 8; c++) {
        if (c == 2 || c == 4 || c == 6) continue;
        uint32_t o[2];
        reduced_pass2<13>(reduced_dequant(coef, swz, q, 0, c), reduced_dequant(coef, swz, q, 1, c), reduced_dequant(coef, swz, q, 3, c),
                          reduced_dequant(coef, swz, q, 5, c), reduced_dequant(coef, swz, q, 7, c), o);
        ws[0][c] = o[0];
        ws[1][c] = o[1];
    }
    JPGPU_K3R_UNROLL
    for (int r = 0; r < 2; r++) {
        uint32_t o[2];
        reduced_pass2<20>(ws[r][0], ws[r][1], ws[r][3], ws[r][5], ws[r][7], o);
        out[2 * r] = islow_sample(o[0]) | (islow_sample(o[1]) << 8);
    }
}

JPGPU_HD inline void reduced_block1(const uint8_t *coef, uint32_t swz, const uint16_t *q, uint32_t (&out)[16]) {
    out[0] = islow_sample(islow_descale<3>(reduced_dequant(coef, swz, q, 0, 0)));
}

// A block of a component whose transform size is s (8: jpeg_idct_islow itself)
JPGPU_HD inline void reduced_block(uint32_t s, const uint8_t *coef, uint32_t swz, const uint16_t *q, uint32_t (&out)[16]) {
    if (s == 8u) islow_block(coef, swz, q, out);
    else if (s == 4u) reduced_block4(coef, swz, q, out);
    else if (s == 2u) reduced_block2(coef, swz, q, out);
    else reduced_block1(coef, swz, q, out);
}

}  // namespace jpgpu
