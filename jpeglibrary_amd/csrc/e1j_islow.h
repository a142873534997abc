// jpeglibrary_amd/csrc/e1j_islow.h -- the arithmetic of encoder stage E1J (e1j_libjpeg.hip): libjpeg's colour conversion, its forward
// transform jpeg_fdct_islow (jfdctint.c, CONST_BITS = 13, PASS1_BITS = 2) and its quantisation, as include/jpgpu.h (4d) states them.
// Every sum and product is a 32-bit integer; 8-bit samples keep all of them inside 32 bits (tests/test_libjpeg_encode_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPGPU_E1J_FN __host__ __device__ __forceinline__
#else
#define JPGPU_E1J_FN inline
#endif

namespace jpgpu {

// A product of the transform: both factors fit 24 bits with room to spare (the constants are below 2^15; what they multiply is a
// sum of at most four values of a pass, below 2^12 in the row pass and below 2^17 in the column pass:
// tests/test_libjpeg_encode_cpu.py), so on the device it is the full-rate 24-bit multiply, whose low 32 bits are the product.
JPGPU_E1J_FN int32_t e1j_mul(int32_t a, int32_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, k);
#else
    return a * k;
#endif
}

// R,G,B -> Y,Cb,Cr (jccolor.c: the table entries are products with these constants, the rounding terms folded into one of them)
JPGPU_E1J_FN void e1j_rgb_to_ycc(int32_t r, int32_t g, int32_t b, int32_t &y, int32_t &cb, int32_t &cr) {
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// DESCALE: an arithmetic shift of the rounded value
template <int N>
JPGPU_E1J_FN int32_t e1j_descale(int32_t x) {
    return (x + (1 << (N - 1))) >> N;
}

// One pass over eight values: FIRST = the row pass (results scaled up by 4), else the column pass (that factor taken out again).
template <bool FIRST>
JPGPU_E1J_FN void e1j_fdct_pass(int32_t (&d)[8]) {
    constexpr int N = FIRST ? 11 : 15;
    const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7];
    const int32_t t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5];
    const int32_t t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * 4;
        d[4] = (t10 - t11) * 4;
    } else {
        d[0] = e1j_descale<2>(t10 + t11);
        d[4] = e1j_descale<2>(t10 - t11);
    }
    int32_t z1 = e1j_mul(t12 + t13, 4433);
    d[2] = e1j_descale<N>(z1 + e1j_mul(t13, 6270));
    d[6] = e1j_descale<N>(z1 - e1j_mul(t12, 15137));
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = e1j_mul(z3 + z4, 9633);
    const int32_t m4 = e1j_mul(t4, 2446), m5 = e1j_mul(t5, 16819), m6 = e1j_mul(t6, 25172), m7 = e1j_mul(t7, 12299);
    z1 = e1j_mul(z1, -7373);
    z2 = e1j_mul(z2, -20995);
    z3 = e1j_mul(z3, -16069) + z5;
    z4 = e1j_mul(z4, -3196) + z5;
    d[7] = e1j_descale<N>(m4 + z1 + z3);
    d[5] = e1j_descale<N>(m5 + z2 + z4);
    d[3] = e1j_descale<N>(m6 + z2 + z3);
    d[1] = e1j_descale<N>(m7 + z1 + z4);
}

// Quantisation (jcdctmgr.c): the divisor is d = Q << 3 (the transform's factor of 8), m = (|c| + d / 2) / d, the sign put back.
// Without a division: m = mulhi(|c| + d / 2, floor(2^32 / d) + 1), exact for every numerator below 2^32 / d -- the transform stays
// below 2^15 and d below 2^11.  The factor is exact too: 2^32 / d has a fraction of at least 1 / d where it has one, far above
// what the double quotient can be off by.
JPGPU_E1J_FN uint32_t e1j_mulhi_factor(uint32_t q) { return (uint32_t)(4294967296.0 / (double)(q << 3)) + 1u; }
JPGPU_E1J_FN int32_t e1j_quantise(int32_t c, uint32_t factor, uint32_t half) {
    const uint32_t n = (uint32_t)(c < 0 ? -c : c) + half;
    const int32_t m = (int32_t)(((uint64_t)n * factor) >> 32);
    return c < 0 ? -m : m;
}

}  // namespace jpgpu
