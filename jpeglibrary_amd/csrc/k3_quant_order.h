// jpeglibrary_amd/csrc/k3_quant_order.h -- the float form of a quantisation table that K3 multiplies by (host + device:
// tests/test_k3_float_dequant_cpu.py enumerates the order below against the zig-zag table on the CPU)
//
// K3 dequantises in float: (float)coefficient * qf, where qf = (float)q * 0.125f carries the 1/8 that ends the reference's
// TransformIDCT (MultiplyInplace(C_0_125)).  Both are exact: q < 2^16, and a power of two scales every rounding of the butterfly
// with it.  The floats lie in the order pass 1 of the transform takes them in: the pass runs on PAIRS of rows
// (rows 2 * r2 and 2 * r2 + 1 of column c in the two halves of one packed register), so
//     qf[2 * (r2 * 8 + c) + h]  belongs to natural position (2 * r2 + h) * 8 + c,     r2 = 0..3, c = 0..7, h = 0..1
// and one 16-byte read holds the multiplier pairs of two neighbouring columns.
#pragma once
#include <stdint.h>

namespace jpgpu {

// zig-zag index of natural position n (the inverse of JpegZigZag.cs:27-38's table, which k3_idct.hip holds as kNat)
constexpr uint8_t kZigOfNat[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                   10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// natural position of entry e of the pair order
constexpr int k3_pair_order_nat(int e) { return (2 * (e >> 4) + (e & 1)) * 8 + ((e >> 1) & 7); }

// q: 64 quantisers in zig-zag order (JpegQuantizationTable.Elements) -> qf: (float)q / 8 in pair order
inline void k3_quant_pair_floats(const uint16_t (&q)[64], float (&qf)[64]) {
    for (int e = 0; e < 64; e++) qf[e] = (float)q[kZigOfNat[k3_pair_order_nat(e)]] * 0.125f;
}

}  // namespace jpgpu
