// jpeglibrary_amd/csrc/k3_block_idct.h -- one 8x8 block through K3's transform, as K3 (k3_idct.hip) and K3Y (k3y_luma.hip) run it: the block
// out of the LDS staging as packed words, the dequantisation in float with the table prescaled by 1/8, the two butterfly passes, rounding and
// level shift, and the saturating pack to bytes.  Stated once, so the two kernels agree bit for bit.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k3_pixel.h"
#include "k3_quant_order.h"

namespace jpgpu {

// This lane's 64 int16 coefficients (zig-zag) out of the swizzled LDS staging (8 chunks of 16 B, chunk p at c_lds + ((p ^ swz) * 16)),
// as they lie: word w holds coefficients 2 * w and 2 * w + 1.  They are held packed across the staging barrier -- 32 registers, not the
// 64 of a dequantised block -- and dequantised inside the transform (block_idct).  (swz = 0: a block as it lies in the store.)
__device__ __forceinline__ void block_load(const uint8_t *c_lds, uint32_t swz, uint32_t (&cw)[32]) {
#pragma unroll
    for (int piece = 0; piece < 8; piece++) {
        const uint4 cv = *reinterpret_cast<const uint4 *>(c_lds + ((piece ^ swz) * 16));
        cw[piece * 4] = cv.x;
        cw[piece * 4 + 1] = cv.y;
        cw[piece * 4 + 2] = cv.z;
        cw[piece * 4 + 3] = cv.w;
    }
}
// coefficient at natural position n of a block held as packed words, as a float (sign-extending word select: v_cvt_f32_i32_sdwa)
__device__ __forceinline__ float coef_at(const uint32_t (&cw)[32], int n) {
    const int k = kZigOfNat[n];
    const uint32_t w = cw[k >> 1];
    return (float)((k & 1) ? ((int32_t)w >> 16) : (int32_t)(int16_t)(w & 0xFFFFu));
}

// The 8-point butterfly of IDCT8x4_LeftPart/RightPart (ref: FastFloatingPointDCT.cs:79-127) on T = float or a pair of
// floats (two independent columns at once: v_pk_add_f32 / v_pk_mul_f32, each component one IEEE operation, never fused).
// Operation order and parenthesisation are normative.
template <typename T>
__device__ __forceinline__ void idct8(T &y0, T &y1, T &y2, T &y3, T &y4, T &y5, T &y6, T &y7) {
    T mz0 = y1 + y7;
    T mz2 = y3 + y7;
    T mz1 = y3 + y5;
    T mz3 = y1 + y5;
    T mz4 = (mz0 + mz1) * 1.175875602f;
    mz2 = (mz2 * -1.961570560f) + mz4;
    mz3 = (mz3 * -0.390180644f) + mz4;
    mz0 = mz0 * -0.899976223f;
    mz1 = mz1 * -2.562915447f;
    const T mb3 = ((y7 * 0.298631336f) + mz0) + mz2;
    const T mb2 = ((y5 * 2.053119869f) + mz1) + mz3;
    const T mb1 = ((y3 * 3.072711026f) + mz1) + mz2;
    const T mb0 = ((y1 * 1.501321110f) + mz0) + mz3;
    mz4 = (y2 + y6) * 0.541196100f;
    mz0 = y0 + y4;
    mz1 = y0 - y4;
    mz2 = mz4 + (y6 * -1.847759065f);
    mz3 = mz4 + (y2 * 0.765366865f);
    const T a0 = mz0 + mz3;
    const T a3 = mz0 - mz3;
    const T a1 = mz1 + mz2;
    const T a2 = mz1 - mz2;
    y0 = a0 + mb0;
    y7 = a0 - mb0;
    y1 = a1 + mb1;
    y6 = a1 - mb1;
    y2 = a2 + mb2;
    y5 = a2 - mb2;
    y3 = a3 + mb3;
    y4 = a3 - mb3;
}

// TransformIDCT + ShiftDataLevel (ref: FastFloatingPointDCT.cs:54-70, ScanDecoder/JpegScanDecoder.cs:64-73), two lanes of the
// butterfly per instruction, on a block that carries the transform's closing 1/8 (MultiplyInplace(C_0_125)) already: the dequantised
// coefficients times 2^-3.  A power of two scales every product, sum and rounding of the two passes with it (nothing underflows:
// DESIGN.md 3, K3), so the results are the reference's, bit for bit, without the 64 multiplications at the end.
// Pass 1 is the caller's: the 1-D IDCT along each ROW (the reference transposes, runs the column butterfly, transposes back);
// a[r2][c] holds rows 2*r2 and 2*r2+1 of column c.
// out[r * 4 + c2] = samples (r, 2*c2) | (r, 2*c2 + 1) << 16 as int16: (short)(Round(v) + levelShift), unclamped.
__device__ __forceinline__ void idct_columns_out(const float2v (&a)[4][8], int32_t level_shift, uint32_t (&out)[32]) {
    // pass 2: along each COLUMN; b[r][c2] holds columns 2*c2 and 2*c2+1 of row r
    float2v b[8][4];
#pragma unroll
    for (int r2 = 0; r2 < 4; r2++)
#pragma unroll
        for (int c2 = 0; c2 < 4; c2++) {
            // b[2 * r2][c2] = {a[r2][2 * c2].x, a[r2][2 * c2 + 1].x}, b[2 * r2 + 1][c2] = the two .y: one two-register move each (the low
            // halves of both sources, the high halves of both), where hipcc builds the pairs from single v_mov_b32
            asm("v_pk_mov_b32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,0]" : "=v"(b[2 * r2][c2]) : "v"(a[r2][2 * c2]), "v"(a[r2][2 * c2 + 1]));
            asm("v_pk_mov_b32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,1]" : "=v"(b[2 * r2 + 1][c2]) : "v"(a[r2][2 * c2]), "v"(a[r2][2 * c2 + 1]));
        }
#pragma unroll
    for (int c2 = 0; c2 < 4; c2++) idct8(b[0][c2], b[1][c2], b[2][c2], b[3][c2], b[4][c2], b[5][c2], b[6][c2], b[7][c2]);
    const uint32_t shift2 = ((uint32_t)level_shift & 0xFFFFu) * 0x00010001u;
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
        for (int c2 = 0; c2 < 4; c2++) {
            const float2v v = b[r][c2];
            // MathF.Round: half to even (v_rndne_f32).  Outside int32 the conversion saturates (v_cvt_i32_f32), where the x64
            // reference gives INT_MIN: a fence, pinned by tests/test_idct_stage_gpu.py
            const int32_t x = (int32_t)__builtin_rintf(v.x);
            const int32_t y = (int32_t)__builtin_rintf(v.y);
            const uint32_t pk = ((uint32_t)x & 0xFFFFu) | ((uint32_t)y << 16);
            // (short)(Round + levelShift): 16-bit wrap-around add on both halves (v_pk_add_u16)
            const short2v sum = __builtin_bit_cast(short2v, pk) + __builtin_bit_cast(short2v, shift2);
            out[r * 4 + c2] = __builtin_bit_cast(uint32_t, sum);
        }
}

// DequantizeBlockAndUnZigZag (ref: ScanDecoder/JpegScanDecoder.cs:50-62) + the transform above on a block held as packed words
// (block_load).  q_lds: the component's table as floats that carry the 1/8, in pair order (k3_quant_order.h).  The reference
// multiplies ushort * short as integers and converts the product; (float)c * qf rounds the same exact product c * q / 8 once
// (|c| <= 2^15 and q / 8 < 2^13 are exact floats), so the two agree bit for bit.
// Row pair by row pair, directly in front of its pass-1 butterfly: sixteen conversions, eight packed multiplications whose
// results are the register pairs the butterfly takes -- a block dequantised as a whole first costs moves and registers.
__device__ __forceinline__ void block_idct(const uint32_t (&cw)[32], const float *q_lds, int32_t level_shift, uint32_t (&out)[32]) {
    float2v a[4][8];
#pragma unroll
    for (int r2 = 0; r2 < 4; r2++) {
#pragma unroll
        for (int c = 0; c < 8; c += 2) {
            const float4 q = reinterpret_cast<const float4 *>(q_lds)[r2 * 4 + (c >> 1)];
            a[r2][c] = float2v{coef_at(cw, (2 * r2) * 8 + c), coef_at(cw, (2 * r2 + 1) * 8 + c)} * float2v{q.x, q.y};
            a[r2][c + 1] = float2v{coef_at(cw, (2 * r2) * 8 + c + 1), coef_at(cw, (2 * r2 + 1) * 8 + c + 1)} * float2v{q.z, q.w};
        }
#if !defined(JPGPU_K3_PRICE)
        idct8(a[r2][0], a[r2][1], a[r2][2], a[r2][3], a[r2][4], a[r2][5], a[r2][6], a[r2][7]);
#endif
    }
#if defined(JPGPU_K3_PRICE)
    // (pricing build only, tools/trace/ab_k3_price.sh: the butterflies left out -- wrong samples, the time of everything else)
#pragma unroll
    for (int i = 0; i < 32; i++)
        out[i] = (__builtin_bit_cast(uint32_t, a[i >> 3][i & 7].x) >> 16) | (__builtin_bit_cast(uint32_t, a[i >> 3][i & 7].y) & 0xFFFF0000u) | (uint32_t)level_shift;
    return;
#endif
    idct_columns_out(a, level_shift, out);
}

// the signed clamp of two int16 samples to [0, 255] (JpegBufferOutputWriter8Bit.ClampTo8Bit) and the packing into bytes 0 and 1 in one
// instruction (v_sat_pk_u8_i16: {sat_u8(S.i16[1]), sat_u8(S.i16[0])}; no builtin names it; the upper half of the result is not used)
__device__ __forceinline__ uint32_t sat2_u8(uint32_t pk) {
    uint32_t r;
    asm("v_sat_pk_u8_i16 %0, %1" : "=v"(r) : "v"(pk));
    return r;
}
// four clamped samples (two packed pairs) -> four bytes: three instructions
__device__ __forceinline__ uint32_t pack4_u8(uint32_t pk01, uint32_t pk23) {
    return __builtin_amdgcn_perm(sat2_u8(pk23), sat2_u8(pk01), 0x05040100u);  // bytes 0,1 of pk01's then 0,1 of pk23's
}

}  // namespace jpgpu
