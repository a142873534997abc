// jpeglibrary_amd/csrc/k3_idct.hip -- K3: dequantise + float32 IDCT + level shift + block output in the requested layout; the literal Dispose() pass
//
// MUST be compiled with -ffp-contract=off: the reference's Vector4 arithmetic never fuses a*b+c
// (FastFloatingPointDCT.cs:79-185).  No fast-math.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "common.h"
#include "kernels.h"
#include "encode_kernels.h"
#include "kernels_device.h"
#include "k3_block_idct.h"
#include "k3_index_math.h"
#include "k3_pixel.h"
#include "k3_quant_order.h"
#include "k3_store_quads.h"

namespace jpgpu {

// ------------------------------------------------------------------------------------------------
// K3: dequantise + IDCT + level shift + block output.  One lane per block.
// ------------------------------------------------------------------------------------------------

// ref: JpegZigZag.cs:27-38
__device__ constexpr uint8_t kNat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ceil(65536 / n), n = 1 .. kMaxBlocksPerMcu (the split form's block -> MCU arithmetic)
// The split form divides by multiplying (idct_output_body: sp_rb, sp_rd, sp_rw); the ranges those reciprocals are exact for rest on these:
// a tile is at most 256 blocks (block and MCU numbers inside it < 256, its lines < 128) of at most 16 per MCU.
static_assert(kIdctBlocksPerWg == 256, "the split form's reciprocals are exact for tiles of up to 256 blocks");
static_assert(kMaxBlocksPerMcu == 16, "kRecip16 and the 16-bit reciprocals of the split form cover 1..16 blocks per MCU");
__device__ constexpr uint32_t kRecip16[kMaxBlocksPerMcu + 1] = {0, 65536, 32768, 21846, 16384, 13108, 10923, 9363, 8192, 7282, 6554, 5958, 5462, 5042, 4682, 4370, 4096};

constexpr bool zig_of_nat_inverts_nat() {
    for (int k = 0; k < 64; k++)
        if (kZigOfNat[kNat[k]] != k) return false;
    return true;
}
static_assert(zig_of_nat_inverts_nat(), "k3_quant_order.h's kZigOfNat is the inverse of kNat");

// (block_load, coef_at, idct8, idct_columns_out, block_idct, sat2_u8 and pack4_u8: k3_block_idct.h, shared with K3Y)

// The same as block_idct on a block dequantised the reference's way, f[natural position] = (float)(q * c) (dispose_pass_kernel): the 1/8 is
// multiplied in here.
__device__ __forceinline__ void block_idct_dequantised(const float (&f)[64], int32_t level_shift, uint32_t (&out)[32]) {
    float2v a[4][8];
#pragma unroll
    for (int r2 = 0; r2 < 4; r2++) {
#pragma unroll
        for (int c = 0; c < 8; c++) a[r2][c] = float2v{f[(2 * r2) * 8 + c], f[(2 * r2 + 1) * 8 + c]} * 0.125f;
        idct8(a[r2][0], a[r2][1], a[r2][2], a[r2][3], a[r2][4], a[r2][5], a[r2][6], a[r2][7]);
    }
    idct_columns_out(a, level_shift, out);
}

// signed clamp of two int16 samples to [0, 255] (JpegBufferOutputWriter8Bit.ClampTo8Bit): v_pk_max_i16 + v_pk_min_i16
__device__ __forceinline__ uint32_t clamp2_u8(uint32_t pk) {
    short2v v = __builtin_bit_cast(short2v, pk);
    v = __builtin_elementwise_max(v, short2v{0, 0});
    v = __builtin_elementwise_min(v, short2v{255, 255});
    return __builtin_bit_cast(uint32_t, v);
}
// INTERLEAVED_U8_SCALED: the sample-to-byte step of the reference's other two stock writers, chosen by the frame's precision P
// the way apps/JpegDecode/DecodeAction.cs:41-54 chooses the writer.  Wave-uniform: the terms live in scalar registers, derived from DevScan::precision.
//   P >= 8  (byte)Clamp(sample >> (P - 8), 0, 255), an arithmetic shift (JpegBufferOutputWriterGreaterThan8Bit.cs:57,64-67); P = 8 is
//           the 8-bit writer
//   P <  8  v = Clamp(sample, 0, 2^P - 1), signed, then ExpandBits(v, P) (JpegBufferOutputWriterLessThan8Bit.cs:59-60, 67-93): its
//           loop ORs copies of v at multiples of P until at least 8 bits are filled, drops the last copy when that went past 8,
//           and FastExpandBits fills the rem = 8 % P bits left with the LOW bits of what it holds:
//             r = v * M,  M = 1 + 2^P + ... (8 / P terms);   byte = (r << rem) | (r & (2^rem - 1))
//           Nothing exceeds 255 on the way, so the two halves of a packed pair never carry into each other.
struct ScaleTo8 {
    uint32_t shift2, max2, mul2, rem2, mask2;  // the same 16-bit value in both halves
    bool expand;                               // P < 8
};
__device__ __forceinline__ ScaleTo8 scale_to_8(uint32_t precision) {
    // (the host refuses precisions outside 1..16 for this format, DeviceBatch::plan_image_geometry; the clamp keeps the shifts defined)
    const uint32_t p = precision < 1u ? 1u : (precision > 16u ? 16u : precision);
    ScaleTo8 k;
    k.expand = p < 8u;
    const uint32_t pe = k.expand ? p : 1u;  // (1..7: the terms below are only used then)
    const uint32_t m = (uint32_t)(0x010101110955FFull >> (8u * (pe - 1u))) & 0xFFu;  // M of P = 1..7: 255, 0x55, 9, 0x11, 1, 1, 1
    const uint32_t rem = 8u % pe;
    k.shift2 = (k.expand ? 0u : p - 8u) * 0x00010001u;
    k.max2 = ((1u << pe) - 1u) * 0x00010001u;
    k.mul2 = m * 0x00010001u;
    k.rem2 = rem * 0x00010001u;
    k.mask2 = ((1u << rem) - 1u) * 0x00010001u;
    return k;
}
// P >= 8, two int16 samples -> two bytes in the low half: v_pk_ashrrev_i16, then the 8-bit writer's signed clamp of both halves
// and the packing in one instruction (v_sat_pk_u8_i16: {sat_u8(S.i16[1]), sat_u8(S.i16[0])}; no builtin names it).  With the
// v_perm_b32 that joins two such results, four samples take as many instructions as INTERLEAVED_U8's four clamps and one v_perm.
__device__ __forceinline__ uint32_t shift_sat2_u8(uint32_t pk, const ScaleTo8 &k) {
    const uint32_t t = __builtin_bit_cast(uint32_t, __builtin_bit_cast(short2v, pk) >> __builtin_bit_cast(short2v, k.shift2));
    uint32_t r;
    asm("v_sat_pk_u8_i16 %0, %1" : "=v"(r) : "v"(t));
    return r;  // (bytes 0 and 1; the upper half is not used)
}
// P < 8, two int16 samples -> two bytes, each in the low byte of its half: v_pk_max_i16, v_pk_min_i16, v_pk_mul_lo_u16,
// v_pk_lshlrev_b16, v_and_or
__device__ __forceinline__ uint32_t expand2_u8(uint32_t pk, const ScaleTo8 &k) {
    short2v v = __builtin_bit_cast(short2v, pk);
    v = __builtin_elementwise_max(v, short2v{0, 0});
    v = __builtin_elementwise_min(v, __builtin_bit_cast(short2v, k.max2));
    const ushort2v r = __builtin_bit_cast(ushort2v, v) * __builtin_bit_cast(ushort2v, k.mul2);
    const ushort2v hi = r << __builtin_bit_cast(ushort2v, k.rem2);
    return __builtin_bit_cast(uint32_t, hi) | (__builtin_bit_cast(uint32_t, r) & k.mask2);
}

constexpr int kIdctThreads = 256;
constexpr uint32_t kPxRowStride = kIdctThreads * 8;  // bytes between sample rows in the LDS pixel tile

// (YCbCr -> RGB(A): chroma_terms / rgb_pixel, k3_pixel.h)
__device__ __forceinline__ uint32_t byte_of(uint32_t lo, uint32_t hi, int i) { return ((i < 4 ? lo : hi) >> (8 * (i & 3))) & 0xFFu; }
// N pixels (R | G << 8 | B << 16 each) -> interleaved bytes at dst (16-byte aligned for N = 16, 8-byte aligned for N = 8)
template <int N, int BPP>
__device__ __forceinline__ void store_rgb_pixels(uint8_t *dst, const uint32_t (&p)[N]) {
    if (BPP == 4) {
#pragma unroll
        for (int i = 0; i < N; i += 4) {
            const uint4 v = {p[i] | 0xFF000000u, p[i + 1] | 0xFF000000u, p[i + 2] | 0xFF000000u, p[i + 3] | 0xFF000000u};
            *reinterpret_cast<uint4 *>(dst + i * 4) = v;
        }
    } else {
        uint32_t w[N * 3 / 4];
#pragma unroll
        for (int i = 0; i < N; i += 4) {  // four pixels -> three dwords
            w[i * 3 / 4 + 0] = p[i] | (p[i + 1] << 24);
            w[i * 3 / 4 + 1] = (p[i + 1] >> 8) | (p[i + 2] << 16);
            w[i * 3 / 4 + 2] = (p[i + 2] >> 16) | (p[i + 3] << 8);
        }
        if (N == 16) {
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const uint4 v = {w[i * 4], w[i * 4 + 1], w[i * 4 + 2], w[i * 4 + 3]};
                *reinterpret_cast<uint4 *>(dst + i * 16) = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < N * 3 / 8; i++) {
                const uint2 v = {w[i * 2], w[i * 2 + 1]};
                *reinterpret_cast<uint2 *>(dst + i * 8) = v;
            }
        }
    }
}

// RGB_PLANAR_U8: rgb_pixel's three clamped sums of four pixels, kept apart instead of packed per pixel: one dword of four bytes per plane,
// gathered with byte permutes (three v_perm_b32 per dword; packing the pixels first and separating them again took sixteen more
// instructions per four pixels, and the output assembly is bound by what it issues)
constexpr int kConvPlanar = 1;
__device__ __forceinline__ uint32_t bytes4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {  // the low bytes of four registers
    return pick4(pick4(a, b, JPGPU_SEL(0, 4, 0, 4)), pick4(c, d, JPGPU_SEL(0, 4, 0, 4)), JPGPU_SEL(0, 1, 4, 5));
}
__device__ __forceinline__ void rgb_planes4(uint32_t y0, uint32_t y1, uint32_t y2, uint32_t y3, const ChromaTerms &t0, const ChromaTerms &t1,
                                            const ChromaTerms &t2, const ChromaTerms &t3, uint32_t &r, uint32_t &g, uint32_t &b) {
    r = bytes4(clamp_u8_i32((int32_t)y0 + t0.r), clamp_u8_i32((int32_t)y1 + t1.r), clamp_u8_i32((int32_t)y2 + t2.r), clamp_u8_i32((int32_t)y3 + t3.r));
    g = bytes4(clamp_u8_i32((int32_t)y0 + t0.g), clamp_u8_i32((int32_t)y1 + t1.g), clamp_u8_i32((int32_t)y2 + t2.g), clamp_u8_i32((int32_t)y3 + t3.g));
    b = bytes4(clamp_u8_i32((int32_t)y0 + t0.b), clamp_u8_i32((int32_t)y1 + t1.b), clamp_u8_i32((int32_t)y2 + t2.b), clamp_u8_i32((int32_t)y3 + t3.b));
}

// RGB_PLANAR_F16 / _F32: the same planes with a wider sample.  A byte u of channel c becomes (float)u * scale[c] + bias[c]: one float32
// multiply and one float32 add, each rounded to nearest even and never fused (affine_sample, k3_pixel.h), then for F16 one more rounding to
// nearest even to binary16 (a float -> _Float16 conversion: subnormals kept, overflow to infinity; never the round-toward-zero packed form).
constexpr int kConvPlanarF16 = 16, kConvPlanarF32 = 32;
constexpr bool conv_is_planar(int conv) { return conv == kConvPlanar || conv == kConvPlanarF16 || conv == kConvPlanarF32; }
constexpr uint32_t conv_plane_sample_bytes(int conv) { return conv == kConvPlanarF16 ? 2 : (conv == kConvPlanarF32 ? 4 : 1); }
// N packed bytes of one plane's row (N = 8 or 16: one or two blocks wide; v_cvt_f32_ubyte0..3 unpack them) -> N samples at dst, which is
// 16-byte aligned: 16 / 32 bytes as F16 (one or two dwordx4 stores), 32 / 64 as F32 (two or four).  Called plane by plane: at most 16 floats
// are alive.
template <int CONV, int N>
__device__ __forceinline__ void store_affine_row(uint8_t *dst, const uint32_t (&w)[N / 4], float scale, float bias) {
    float f[N];
#pragma unroll
    for (int j = 0; j < N; j++) f[j] = affine_sample((w[j >> 2] >> (8 * (j & 3))) & 0xFFu, scale, bias);
    if (CONV == kConvPlanarF32) {
#pragma unroll
        for (int q = 0; q < N / 4; q++) *reinterpret_cast<float4 *>(dst + q * 16) = float4{f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
    } else {
#pragma unroll
        for (int q = 0; q < N / 8; q++) {
            uint32_t h[4];
#pragma unroll
            for (int j = 0; j < 4; j++) h[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(float2v{f[8 * q + 2 * j], f[8 * q + 2 * j + 1]}, half2v));
            *reinterpret_cast<uint4 *>(dst + q * 16) = uint4{h[0], h[1], h[2], h[3]};
        }
    }
}
// One task's row of the three planes (N = 8 or 16 bytes of each, as dwords) at p0, p1, p2: as the bytes they are (RGB_PLANAR_U8; p is 8- / 16-byte
// aligned), or plane by plane through the affine step
template <int CONV, int N>
__device__ __forceinline__ void store_plane_rows(uint8_t *p0, uint8_t *p1, uint8_t *p2, const uint32_t (&r)[N / 4], const uint32_t (&g)[N / 4],
                                                 const uint32_t (&b)[N / 4], const OutputAffine &aff) {
    if constexpr (CONV != kConvPlanar) {
        store_affine_row<CONV, N>(p0, r, aff.scale[0], aff.bias[0]);
        store_affine_row<CONV, N>(p1, g, aff.scale[1], aff.bias[1]);
        store_affine_row<CONV, N>(p2, b, aff.scale[2], aff.bias[2]);
    } else if constexpr (N == 16) {
        *reinterpret_cast<uint4 *>(p0) = uint4{r[0], r[1], r[2], r[3]};
        *reinterpret_cast<uint4 *>(p1) = uint4{g[0], g[1], g[2], g[3]};
        *reinterpret_cast<uint4 *>(p2) = uint4{b[0], b[1], b[2], b[3]};
    } else {
        *reinterpret_cast<uint2 *>(p0) = uint2{r[0], r[1]};
        *reinterpret_cast<uint2 *>(p1) = uint2{g[0], g[1]};
        *reinterpret_cast<uint2 *>(p2) = uint2{b[0], b[1]};
    }
}

// Stand-alone conversion of an interleaved u8 image (C = 3: Y,Cb,Cr; C = 1: Y with Cb = Cr = 128 like
// apps/JpegDecode/DecodeAction.cs:57-65) for the layouts the writer kernel has no fused path for.
// bpp = 3 / 4: interleaved R,G,B(,A) pixels; bpp = 1: RGB_PLANAR_U8, three planes of n_pixels bytes each (a wave writes 64 consecutive
// bytes of each plane).
__global__ __launch_bounds__(256) void ycc_to_rgb_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t n_pixels, int comps,
                                                         int bpp, YccRgbFactors k) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_pixels; i += (uint64_t)gridDim.x * 256) {
        const uint32_t y = src[i * comps];
        const uint32_t cb = comps == 3 ? src[i * 3 + 1] : 128u, cr = comps == 3 ? src[i * 3 + 2] : 128u;
        const uint32_t px = rgb_pixel(y, chroma_terms(cb, cr, k));
        if (bpp == 1) {
            dst[i] = (uint8_t)px;
            dst[n_pixels + i] = (uint8_t)(px >> 8);
            dst[2 * n_pixels + i] = (uint8_t)(px >> 16);
            continue;
        }
        uint8_t *d = dst + i * bpp;
        d[0] = (uint8_t)px;
        d[1] = (uint8_t)(px >> 8);
        d[2] = (uint8_t)(px >> 16);
        if (bpp == 4) d[3] = 255;
    }
}

// The same for RGB_PLANAR_F16 / _F32 (T = _Float16 / float): ycc_to_rgb_kernel's bpp = 1 form, the same conversion, then the affine step of
// the fused path.  W x H is arbitrary here, so a plane's start is aligned for one sample only: one sample per store (a wave still writes 128 /
// 256 consecutive bytes of each plane).
template <typename T>
__global__ __launch_bounds__(256) void ycc_to_rgb_planes_kernel(const uint8_t *__restrict__ src, T *__restrict__ dst, uint64_t n_pixels, int comps,
                                                                YccRgbFactors k, OutputAffine aff) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_pixels; i += (uint64_t)gridDim.x * 256) {
        const uint32_t y = src[i * comps];
        const uint32_t cb = comps == 3 ? src[i * 3 + 1] : 128u, cr = comps == 3 ? src[i * 3 + 2] : 128u;
        const uint32_t px = rgb_pixel(y, chroma_terms(cb, cr, k));
        dst[i] = (T)affine_sample(px & 0xFFu, aff.scale[0], aff.bias[0]);  // (float -> _Float16: round to nearest even)
        dst[n_pixels + i] = (T)affine_sample((px >> 8) & 0xFFu, aff.scale[1], aff.bias[1]);
        dst[2 * n_pixels + i] = (T)affine_sample((px >> 16) & 0xFFu, aff.scale[2], aff.bias[2]);
    }
}

// "O3", the xunit tests' sink (ref: tests/JpegLibrary.Tests/Utils/JpegExtendingOutputWriter.cs:30-112) as a device format:
// out[(y * W + x) * 4 + c] (componentCount = 4, the way every test constructs it), uint16.  Input: the PLANAR_I16 planes K3
// wrote = WriteBlock's arguments before chroma expansion.  WriteBlockSlow replicates with shifts (:238-268), so pixel (x, y)
// of component c is plane_c[y >> vshift][x >> hshift] -- for a sampling factor that is the frame's maximum or 1.  Any other
// factor (round 6: H = 2 under a maximum of 4 ...) meets the decoder's `(offsetX + x) * 8` placement (...BaselineScanDecoder.cs:104,
// 134): block x of the MCU lands 8 pixels behind block x - 1 and is hs * 8 wide, so the blocks of one MCU overlap, the later call
// winning, and the MCU's last (hs - 1) * (h - 1) * 8 columns are never written (they keep the buffer's zero); the same downwards.
// The writer then takes (ushort)sample -- a negative sample becomes a large value -- clamps to 2^P - 1 and spreads the P bits
// over 16 (FastExpandBits for P >= 8, ExpandBits below).
// One launch for the whole batch: blockIdx.y = image (its descriptor in HBM), blockIdx.x strides over the image's pixels.
__global__ __launch_bounds__(256) void extend_u16_kernel(const uint8_t *__restrict__ planes, uint8_t *__restrict__ out_base,
                                                         const ExtendPlanes *__restrict__ images) {
    const ExtendPlanes g = images[blockIdx.y];
    uint16_t *out = reinterpret_cast<uint16_t *>(out_base + g.out_off);
    for (uint64_t px = (uint64_t)blockIdx.x * 256 + threadIdx.x; px < (uint64_t)g.width * g.height; px += (uint64_t)gridDim.x * 256) {
    const uint32_t y = (uint32_t)(px / g.width), x = (uint32_t)(px - (uint64_t)y * g.width);
    // (the host refuses precisions outside 1..16 for this format, DeviceBatch::plan_image_geometry; the clamp keeps the shifts
    // below 32 and the ExpandBits loop finite whatever reaches the kernel)
    const uint32_t p = g.precision < 1u ? 1u : (g.precision > 16u ? 16u : g.precision), mx = (1u << p) - 1u;
    uint16_t v4[4] = {0, 0, 0, 0};
#pragma unroll  // (compile-time component index: the descriptor's arrays stay in registers, no scratch)
    for (uint32_t c = 0; c < 4u; c++) {
        if (c >= g.ncomp) continue;
        const int16_t *pl = reinterpret_cast<const int16_t *>(planes + g.plane_off[c]);
        // the LAST block of the MCU whose replicated samples cover the pixel: x* = min(px >> 3, h - 1), covered while px < 8 x* + 8 hs
        const uint32_t mw = 8u * (g.max_h | (g.max_h == 0)), mh = 8u * (g.max_v | (g.max_v == 0));
        const uint32_t mcx = x / mw, pxm = x - mcx * mw, mcy = y / mh, pym = y - mcy * mh;
        const uint32_t bx = (pxm >> 3) < g.hcnt[c] - 1u ? (pxm >> 3) : g.hcnt[c] - 1u, by = (pym >> 3) < g.vcnt[c] - 1u ? (pym >> 3) : g.vcnt[c] - 1u;
        const uint32_t dx = pxm - 8u * bx, dy = pym - 8u * by;
        if (g.max_h != 0 && (dx >= (8u << g.hshift[c]) || dy >= (8u << g.vshift[c]))) continue;  // never written: the fresh buffer's zero
        const uint32_t s = g.max_h == 0 ? (uint32_t)(uint16_t)pl[(uint64_t)(y >> g.vshift[c]) * g.pitch[c] + (x >> g.hshift[c])]  // (a progressive frame: the allocator's Flush)
                                        : (uint32_t)(uint16_t)pl[(uint64_t)((mcy * g.vcnt[c] + by) * 8u + (dy >> g.vshift[c])) * g.pitch[c] + (mcx * g.hcnt[c] + bx) * 8u + (dx >> g.hshift[c])];
        uint32_t bits = s < mx ? s : mx;  // Clamp((ushort)sample, max)
        if (p >= 8u) {
            const uint32_t rem = 16u - p;
            bits = (bits << rem) | (bits & ((1u << rem) - 1u));  // FastExpandBits, as written
        } else {
            uint32_t cur = p;
            while (cur < 16u) {
                bits = (bits << p) | bits;
                cur += p;
            }
            if (cur > 16u) {
                bits >>= p;
                cur -= p;
                const uint32_t rem = 16u - cur;
                bits = (bits << rem) | (bits & ((1u << rem) - 1u));
            }
        }
        v4[c] = (uint16_t)bits;
    }
    // channels the frame does not have keep what the caller's (fresh, zeroed) buffer held: the batch owns the buffer, so zero
    *reinterpret_cast<uint2 *>(out + px * 4) = uint2{(uint32_t)v4[0] | ((uint32_t)v4[1] << 16), (uint32_t)v4[2] | ((uint32_t)v4[3] << 16)};
    }
}

// The quad exchange of k3_store_quads.h: d0, d1, d2 = what the lane writes in stores 0, 1, 2, out of the quad's o0, o1, o2.  A selected move is
// one v_cndmask_b32_dpp -- the lanes of `keep` (vcc) take the second source, the lane the move is aimed at the first, read from lane `src` of
// its quad -- which takes inline assembly: from the builtins hipcc makes a v_mov_b32_dpp and a v_cndmask_b32 of it.  Two per output dword.
// In a tile whose quads do not exchange every mask is all lanes: every lane has its vcc bit set and takes the second source, its own
// register, so d = o and what the DPP source reads never matters.  (bound_ctrl is what makes that hold beside lanes that are switched off,
// as such a tile has them inside a quad: without it a lane whose DPP source lane is off would not be written at all.)
struct QuadKeepMasks {
    uint64_t ne0, ne1, ne2, ne3;  // every lane but lane j of each quad
};
__device__ __forceinline__ QuadKeepMasks quad_keep_masks(bool exchange) {
    return QuadKeepMasks{exchange ? 0xEEEEEEEEEEEEEEEEull : ~0ull, exchange ? 0xDDDDDDDDDDDDDDDDull : ~0ull, exchange ? 0xBBBBBBBBBBBBBBBBull : ~0ull,
                         exchange ? 0x7777777777777777ull : ~0ull};
}
constexpr bool quad_move_is(uint32_t store, uint32_t lane, uint32_t src_lane, uint32_t src_reg) {
    return k3_quad_move(store, lane).src_lane == src_lane && k3_quad_move(store, lane).src_reg == src_reg;
}
static_assert(quad_move_is(0, 0, 0, 0) && quad_move_is(0, 1, 1, 0) && quad_move_is(0, 2, 0, 1) && quad_move_is(0, 3, 0, 2), "store 0 of the assembly below");
static_assert(quad_move_is(1, 0, 1, 2) && quad_move_is(1, 1, 1, 1) && quad_move_is(1, 2, 2, 1) && quad_move_is(1, 3, 2, 0), "store 1 of the assembly below");
static_assert(quad_move_is(2, 0, 3, 0) && quad_move_is(2, 1, 3, 1) && quad_move_is(2, 2, 2, 2) && quad_move_is(2, 3, 3, 2), "store 2 of the assembly below");
#define JPGPU_QSEL(d, from, keep, src) \
    "v_cndmask_b32_dpp " d ", " from ", " keep ", vcc quad_perm:[" src "," src "," src "," src "] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define JPGPU_QSEL4(d, from, keep, src) \
    JPGPU_QSEL("%[" d "x]", "%[" from "x]", "%[" keep "x]", src) JPGPU_QSEL("%[" d "y]", "%[" from "y]", "%[" keep "y]", src) \
    JPGPU_QSEL("%[" d "z]", "%[" from "z]", "%[" keep "z]", src) JPGPU_QSEL("%[" d "w]", "%[" from "w]", "%[" keep "w]", src)
__device__ __forceinline__ void quad_exchange(const uint4 &o0, const uint4 &o1, const uint4 &o2, const QuadKeepMasks &k, uint4 &d0, uint4 &d1, uint4 &d2) {
    // (hipcc's hazard recogniser does not read inline assembly: the wait states a DPP read needs behind a vector write of its source, and
    // behind a vector write of exec, are spent here.  No move reads through DPP what a move before it wrote.)
    asm volatile("s_nop 4\n\t"
        "s_mov_b64 vcc, %[ne2]\n\t"                       // lane 2 <- lane 0's o1
        JPGPU_QSEL4("d0", "o1", "o0", "0")
        "s_mov_b64 vcc, %[ne0]\n\t"                       // lane 0 <- lane 1's o2; lane 0 <- lane 3's o0
        JPGPU_QSEL4("d1", "o2", "o1", "1") JPGPU_QSEL4("d2", "o0", "o2", "3")
        "s_mov_b64 vcc, %[ne3]\n\t"                       // lane 3 <- lane 0's o2; lane 3 <- lane 2's o0
        JPGPU_QSEL4("d0", "o2", "d0", "0") JPGPU_QSEL4("d1", "o0", "d1", "2")
        "s_mov_b64 vcc, %[ne1]\n\t"                       // lane 1 <- lane 3's o1
        JPGPU_QSEL4("d2", "o1", "d2", "3")
        : [d0x] "=&v"(d0.x), [d0y] "=&v"(d0.y), [d0z] "=&v"(d0.z), [d0w] "=&v"(d0.w), [d1x] "=&v"(d1.x), [d1y] "=&v"(d1.y), [d1z] "=&v"(d1.z),
          [d1w] "=&v"(d1.w), [d2x] "=&v"(d2.x), [d2y] "=&v"(d2.y), [d2z] "=&v"(d2.z), [d2w] "=&v"(d2.w)
        : [o0x] "v"(o0.x), [o0y] "v"(o0.y), [o0z] "v"(o0.z), [o0w] "v"(o0.w), [o1x] "v"(o1.x), [o1y] "v"(o1.y), [o1z] "v"(o1.z), [o1w] "v"(o1.w),
          [o2x] "v"(o2.x), [o2y] "v"(o2.y), [o2z] "v"(o2.z), [o2w] "v"(o2.w), [ne0] "s"(k.ne0), [ne1] "s"(k.ne1), [ne2] "s"(k.ne2), [ne3] "s"(k.ne3)
        : "vcc");
}
#undef JPGPU_QSEL4
#undef JPGPU_QSEL

// Output assembly of the INTERLEAVED_U8 format from the LDS sample tile [8 rows][256 blocks][8 B] (phase C).
// CONV: 0 = the samples as they are (Y,Cb,Cr), 3 / 4 = converted to R,G,B / R,G,B,A bytes (fast layouts only), kConvPlanar = converted and
// written as three planes of one byte per pixel (RGB_PLANAR_U8; fast layouts, and kLayGray as a layout of one-block MCUs without chroma),
// kConvPlanarF16 / kConvPlanarF32 = those planes with every byte as a float sample (RGB_PLANAR_F16 / _F32, `aff`).
// The fast layouts take the tile's place from wave-uniform state (k3_index_math.h): pos = its first MCU, mpl / line_recip = the MCUs of a
// line and their reciprocal, row_recip = that of n_mcu, img_h = the frame's lines, img = the image in the output buffer.  Nothing in their
// task loop divides.
// WIN: the image is a window of the frame (DevScan::win_*).  The generic layout gets the MCU's place in the frame and stores at (x - win_x,
// y - win_y), clipped to the window by unsigned compares.  The fast layouts get the tile's place in the window's MCU cover instead: pos / mpl /
// line_recip are the cover's (its first MCU column starts at the window's first pixel column, and the window is whole MCUs wide:
// idct_window_layout_class, so the pitch mpl * 8 * max_h is the window's), img_h = the window's lines, and win_yoff = the lines of the cover's
// first MCU row above the window; a row outside the window's lines is dropped.
template <int LAY, int CONV, bool WIN = false>
__device__ __forceinline__ void interleaved_output_from_tile(const uint8_t *sh_px, const DevScan &s, const K3TilePos &pos, uint32_t mpl,
                                                             uint32_t line_recip, uint32_t row_recip, uint32_t img_h, uint32_t n_mcu,
                                                             uint32_t tid, bool have_block, const DevScanComponent &comp, uint32_t mcu_x,
                                                             uint32_t mcu_y, uint32_t b, uint8_t *img, const YccRgbFactors &kf, bool reached,
                                                             uint32_t mcu, uint32_t fail_block, const OutputAffine &aff, uint32_t win_yoff = 0) {
    if (LAY == kLayGeneric) {
        const uint32_t W = WIN ? s.win_w : s.width, H = WIN ? s.win_h : s.height, C = s.frame_components;
        const uint32_t wx = WIN ? s.win_x : 0u, wy = WIN ? s.win_y : 0u;
        // any component count / sampling: bytewise stores with WriteBlockSlow's replication
        // (ref: ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:238-268) and the sink's clipping (x < W, y < H)
        if (have_block) {
            const uint32_t hs = comp.hs, vs = comp.vs;
            // (a progressive frame's Dispose(): JpegBlockAllocator.Flush places block (col, row) of the component's own grid at
            // (col * hs * 8, row * vs * 8), JpegBlockAllocator.cs:120-149 -- the same place for a factor that is the maximum or 1)
            const bool flush = s.kind == kScanFrameOnly;
            const uint32_t x0 = flush ? (mcu_x * comp.h + s.blk_x[b]) * hs * 8 : (mcu_x * s.max_h + s.blk_x[b]) * 8;
            const uint32_t y0 = flush ? (mcu_y * comp.v + s.blk_y[b]) * vs * 8 : (mcu_y * s.max_v + s.blk_y[b]) * 8;
            const uint32_t hshift = 31 - __builtin_clz(hs | 1), vshift = 31 - __builtin_clz(vs | 1);
            // A sampling factor that is neither the frame's maximum nor 1 (round 6): the decoder places block x of the MCU at
            // (offsetX + x) * 8 (:104, 134) whatever the block's replicated width hs * 8 is, so the blocks of one MCU OVERLAP and the
            // later WriteBlock wins: a block owns a replicated pixel unless the next block that covers it -- block x + 1 of its
            // row from column 8 on, else from row 8 on the first covering block of the row below -- has reached the writer too.
            // (What no block covers keeps the buffer's content: the host clears the outputs of such frames, plan_work.)
            const uint32_t bx = s.blk_x[b], by = s.blk_y[b];
            const bool overlap_h = !flush && comp.h > 1 && hs > 1, overlap_v = !flush && comp.v > 1 && vs > 1;
            const uint32_t base = b - (by * comp.h + bx);  // the component's first block in the MCU
            if ((overlap_h || overlap_v) && !reached) return;
            for (uint32_t v = 0; v < vs; v++)
                for (uint32_t i = 0; i < 8; i++) {
                    const uint32_t y = y0 + 8 * v + i - wy;  // (WIN: above the window wraps to a large value)
                    if (y >= H) continue;
                    const uint8_t *srow = sh_px + ((8 * v + i) >> vshift) * kPxRowStride + tid * 8;
                    for (uint32_t h = 0; h < hs; h++) {
                        if (overlap_h || overlap_v) {
                            uint32_t later = 0xFFFFFFFFu;  // the earliest later block that covers these eight pixels
                            if (overlap_h && bx + 1 < comp.h && h >= 1) later = base + by * comp.h + bx + 1;
                            else if (overlap_v && by + 1 < comp.v && v >= 1) {
                                const int32_t xf = (int32_t)bx + (int32_t)h - (int32_t)hs + 1;
                                later = base + (by + 1) * comp.h + (uint32_t)(xf < 0 ? 0 : xf);
                            }
                            if (later != 0xFFFFFFFFu && (uint64_t)mcu * s.blocks_per_mcu + later < fail_block) continue;
                        }
                        for (uint32_t j = 0; j < 8; j++) {
                            const uint32_t x = x0 + 8 * h + j - wx;
                            if (x < W) img[((size_t)y * W + x) * C + comp.component_index] = srow[(8 * h + j) >> hshift];
                        }
                    }
                }
        }
    } else {
    // YCbCr fast paths: one task = one pixel row of one MCU (8*max_h pixels); consecutive lanes take consecutive MCUs of
    // the same row, so a wave writes one contiguous run of the output row per store instruction group.
    constexpr bool planar = conv_is_planar(CONV);
    constexpr bool gray = LAY == kLayGray;  // (the planar sinks only: the other sinks write a gray block from its own lane)
    constexpr uint32_t max_h = (LAY == kLayYccH1V1 || (gray && planar)) ? 1 : 2;
    constexpr uint32_t max_v = (LAY == kLayYccH2V2) ? 2 : 1;
    constexpr uint32_t rows_per_mcu = 8 * max_v;
    constexpr uint32_t vshift = max_v >> 1;
    constexpr uint32_t kbpm = (gray && planar) ? 1 : max_h * max_v + 2;
    constexpr uint32_t bpp = CONV == 4 ? 4 : (planar ? conv_plane_sample_bytes(CONV) : 3);  // bytes from a pixel to the next of its row
    const uint32_t n_tasks = rows_per_mcu * n_mcu;
    const uint32_t W = mpl * (8 * max_h);  // (whole MCUs: idct_layout_class)
    // wave-uniform: the first pixel line of the tile's first MCU line; a lane adds a 32-bit offset (a tile spans few lines, or short ones)
    const uint32_t y0 = pos.gy0 * rows_per_mcu;
    uint8_t *line0 = img + (uint64_t)y0 * W * bpp;
    if (WIN) line0 -= (uint64_t)win_yoff * W * bpp;  // (the cover's first MCU row may begin above the window: such rows are dropped below)
    // RGB_PLANAR_U8: the same line in the G and B planes.  A plane is W * H bytes, which can pass 2^32: wave-uniform 64-bit bases like line0,
    // and the lane's 32-bit offset `at` serves all three.  (W is a multiple of the store width and so is every plane: idct_layout_class.)
    // RGB_PLANAR_F16 / _F32: a plane is W * H * 2 / 4 bytes and a lane stores 16-byte pieces.  The fast classes have W a whole number of MCUs
    // (a multiple of 8), so a line is a multiple of 16 bytes in either type, and so is a plane; an image starts on a multiple of 256 in the
    // batch's output buffer (plan_image): every plane, line and lane start is 16-byte aligned.
    uint8_t *line1 = line0 + (uint64_t)W * img_h * (planar ? bpp : 1), *line2 = line1 + (uint64_t)W * img_h * (planar ? bpp : 1);
    // Sample bytes of two-block-wide MCUs: the four lanes of a quad exchange 16-byte pieces so that every store instruction writes whole
    // 64-byte blocks (k3_store_quads.h).  Wave-uniform per tile; a tile whose quads are not four MCUs side by side -- a clipped range, tiles
    // that are not line-aligned, a line that is no multiple of four MCUs -- takes the same loop with its own registers at +0 / +16 / +32.
    constexpr bool kQuads = CONV == 0 && max_h == 2;
    const bool exchange = kQuads && k3_quad_eligible(n_mcu, mpl, pos.gx0);
    const QuadKeepMasks keep = quad_keep_masks(exchange);
    uint32_t q_off[kK3QuadStores];
#pragma unroll
    for (uint32_t st = 0; st < kK3QuadStores; st++) q_off[st] = exchange ? k3_quad_lane_offset(k3_quad_offsets_packed(st), tid) : st * kK3QuadPieceBytes;
    for (uint32_t t = tid; t < n_tasks; t += kIdctThreads) {
        const uint32_t row = k3_task_row(t, row_recip), m = t - k3_mul24(row, n_mcu);
        const uint32_t x = pos.gx0 + m, wraps = k3_line_wraps(x, mpl, line_recip);
        uint32_t back = k3_mul24(wraps, mpl);
        asm("" : "+v"(back));  // (kept a 24-bit product: folded into the subtraction it becomes a full 32-bit multiply-add by -mpl)
        const uint32_t gx = x - back;
        const uint32_t yl = wraps * rows_per_mcu + row;  // pixel line below line0
        if (y0 + yl - win_yoff >= img_h) continue;  // (WIN: a line above the window wraps to a large value)
        const uint32_t mb = k3_mul24(m, kbpm);
        const uint8_t *yrow = sh_px + (row & 7) * kPxRowStride + (mb + (row >> 3) * max_h) * 8;
        const uint8_t *crow = sh_px + (row >> vshift) * kPxRowStride + (mb + max_h * max_v) * 8;
        const uint32_t at = k3_mul24(yl, W * bpp) + k3_mul24(gx, 8 * max_h * bpp);  // (W * bpp < 2^18; the sum is far below 2^32)
        uint8_t *dst_px = line0 + at;
        if (planar) {
            // three stores per task, one per plane: consecutive lanes write consecutive 8 / 16 bytes of one plane row
            // (float samples: the same bytes, plane by plane through the affine step -- consecutive lanes write consecutive 16 / 32 bytes as
            // F16 and 32 / 64 as F32 of one plane row, in 16-byte stores)
            if (gray) {
                const uint2 yv = *reinterpret_cast<const uint2 *>(yrow);  // R = G = B = Y (Cb = Cr = 128 contribute nothing, DecodeAction.cs:57-65)
                if (CONV != kConvPlanar) {
                    const uint32_t w[2] = {yv.x, yv.y};
                    store_plane_rows<CONV, 8>(line0 + at, line1 + at, line2 + at, w, w, w, aff);
                    continue;
                }
                *reinterpret_cast<uint2 *>(line0 + at) = yv;
                *reinterpret_cast<uint2 *>(line1 + at) = yv;
                *reinterpret_cast<uint2 *>(line2 + at) = yv;
            } else if (max_h == 2) {
                const uint4 yv = *reinterpret_cast<const uint4 *>(yrow);  // 16 luma samples (two adjacent blocks)
                const uint4 cv = *reinterpret_cast<const uint4 *>(crow);  // 8 Cb (x,y) + 8 Cr (z,w)
                uint32_t r[4], g[4], bl[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {  // four pixels under two chroma sample pairs
                    const uint32_t y4 = q == 0 ? yv.x : (q == 1 ? yv.y : (q == 2 ? yv.z : yv.w));
                    const ChromaTerms t0 = chroma_terms(byte_of(cv.x, cv.y, 2 * q), byte_of(cv.z, cv.w, 2 * q), kf);
                    const ChromaTerms t1 = chroma_terms(byte_of(cv.x, cv.y, 2 * q + 1), byte_of(cv.z, cv.w, 2 * q + 1), kf);
                    rgb_planes4(y4 & 0xFFu, (y4 >> 8) & 0xFFu, (y4 >> 16) & 0xFFu, y4 >> 24, t0, t0, t1, t1, r[q], g[q], bl[q]);
                }
                store_plane_rows<CONV, 16>(line0 + at, line1 + at, line2 + at, r, g, bl, aff);
            } else {
                const uint2 yv = *reinterpret_cast<const uint2 *>(yrow);
                const uint2 bv = *reinterpret_cast<const uint2 *>(crow);
                const uint2 rv = *reinterpret_cast<const uint2 *>(crow + 8);
                ChromaTerms t[8];
#pragma unroll
                for (int j = 0; j < 8; j++) t[j] = chroma_terms(byte_of(bv.x, bv.y, j), byte_of(rv.x, rv.y, j), kf);
                uint32_t r[2], g[2], bl[2];
                rgb_planes4(byte_of(yv.x, yv.y, 0), byte_of(yv.x, yv.y, 1), byte_of(yv.x, yv.y, 2), byte_of(yv.x, yv.y, 3), t[0], t[1], t[2], t[3], r[0], g[0], bl[0]);
                rgb_planes4(byte_of(yv.x, yv.y, 4), byte_of(yv.x, yv.y, 5), byte_of(yv.x, yv.y, 6), byte_of(yv.x, yv.y, 7), t[4], t[5], t[6], t[7], r[1], g[1], bl[1]);
                store_plane_rows<CONV, 8>(line0 + at, line1 + at, line2 + at, r, g, bl, aff);
            }
        } else if (max_h == 2 && CONV != 0) {
            const uint4 yv = *reinterpret_cast<const uint4 *>(yrow);  // 16 luma samples (two adjacent blocks)
            const uint4 cv = *reinterpret_cast<const uint4 *>(crow);  // 8 Cb (x,y) + 8 Cr (z,w)
            uint32_t px[16];
#pragma unroll
            for (int j = 0; j < 8; j++) {  // one chroma sample pair covers two pixels
                const ChromaTerms t = chroma_terms(byte_of(cv.x, cv.y, j), byte_of(cv.z, cv.w, j), kf);
                px[2 * j] = rgb_pixel(byte_of(j < 4 ? yv.x : yv.z, j < 4 ? yv.y : yv.w, (2 * j) & 7), t);
                px[2 * j + 1] = rgb_pixel(byte_of(j < 4 ? yv.x : yv.z, j < 4 ? yv.y : yv.w, (2 * j + 1) & 7), t);
            }
            store_rgb_pixels<16, bpp>(dst_px, px);
        } else if (CONV != 0) {
            const uint2 yv = *reinterpret_cast<const uint2 *>(yrow);
            const uint2 bv = *reinterpret_cast<const uint2 *>(crow);
            const uint2 rv = *reinterpret_cast<const uint2 *>(crow + 8);
            uint32_t px[8];
#pragma unroll
            for (int j = 0; j < 8; j++) px[j] = rgb_pixel(byte_of(yv.x, yv.y, j), chroma_terms(byte_of(bv.x, bv.y, j), byte_of(rv.x, rv.y, j), kf));
            store_rgb_pixels<8, bpp>(dst_px, px);
        } else if (max_h == 2) {
            const uint4 yv = *reinterpret_cast<const uint4 *>(yrow);  // 16 luma samples (two adjacent blocks)
            const uint4 cv = *reinterpret_cast<const uint4 *>(crow);  // 8 Cb (x,y) + 8 Cr (z,w)
            const uint32_t cc0 = pick4(cv.x, cv.z, JPGPU_SEL(0, 4, 1, 5)), cc1 = pick4(cv.x, cv.z, JPGPU_SEL(2, 6, 3, 7));
            const uint32_t cc2 = pick4(cv.y, cv.w, JPGPU_SEL(0, 4, 1, 5)), cc3 = pick4(cv.y, cv.w, JPGPU_SEL(2, 6, 3, 7));
            uint4 o0, o1, o2;
            o0.x = pick4(yv.x, cc0, JPGPU_SEL(0, 4, 5, 1));
            o0.y = pick4(yv.x, cc0, JPGPU_SEL(4, 5, 2, 6));
            o0.z = pick4(yv.x, cc0, JPGPU_SEL(7, 3, 6, 7));
            o0.w = pick4(yv.y, cc1, JPGPU_SEL(0, 4, 5, 1));
            o1.x = pick4(yv.y, cc1, JPGPU_SEL(4, 5, 2, 6));
            o1.y = pick4(yv.y, cc1, JPGPU_SEL(7, 3, 6, 7));
            o1.z = pick4(yv.z, cc2, JPGPU_SEL(0, 4, 5, 1));
            o1.w = pick4(yv.z, cc2, JPGPU_SEL(4, 5, 2, 6));
            o2.x = pick4(yv.z, cc2, JPGPU_SEL(7, 3, 6, 7));
            o2.y = pick4(yv.w, cc3, JPGPU_SEL(0, 4, 5, 1));
            o2.z = pick4(yv.w, cc3, JPGPU_SEL(4, 5, 2, 6));
            o2.w = pick4(yv.w, cc3, JPGPU_SEL(7, 3, 6, 7));
            if (kQuads) {
                uint4 d0, d1, d2;
                quad_exchange(o0, o1, o2, keep, d0, d1, d2);
                *reinterpret_cast<uint4 *>(line0 + (at + q_off[0])) = d0;
                *reinterpret_cast<uint4 *>(line0 + (at + q_off[1])) = d1;
                *reinterpret_cast<uint4 *>(line0 + (at + q_off[2])) = d2;
            } else {
                uint4 *dst = reinterpret_cast<uint4 *>(dst_px);
                dst[0] = o0;
                dst[1] = o1;
                dst[2] = o2;
            }
        } else {
            const uint2 yv = *reinterpret_cast<const uint2 *>(yrow);
            const uint2 bv = *reinterpret_cast<const uint2 *>(crow);
            const uint2 rv = *reinterpret_cast<const uint2 *>(crow + 8);
            uint2 o0, o1, o2;
            {
                const uint32_t lo = pick4(bv.x, rv.x, JPGPU_SEL(0, 4, 1, 5)), hi = pick4(bv.x, rv.x, JPGPU_SEL(2, 6, 3, 7));
                const uint32_t mid = pick4(lo, hi, JPGPU_SEL(2, 3, 4, 5));
                o0.x = pick4(yv.x, lo, JPGPU_SEL(0, 4, 5, 1));
                o0.y = pick4(yv.x, mid, JPGPU_SEL(4, 5, 2, 6));
                o1.x = pick4(yv.x, hi, JPGPU_SEL(5, 3, 6, 7));
            }
            {
                const uint32_t lo = pick4(bv.y, rv.y, JPGPU_SEL(0, 4, 1, 5)), hi = pick4(bv.y, rv.y, JPGPU_SEL(2, 6, 3, 7));
                const uint32_t mid = pick4(lo, hi, JPGPU_SEL(2, 3, 4, 5));
                o1.y = pick4(yv.y, lo, JPGPU_SEL(0, 4, 5, 1));
                o2.x = pick4(yv.y, mid, JPGPU_SEL(4, 5, 2, 6));
                o2.y = pick4(yv.y, hi, JPGPU_SEL(5, 3, 6, 7));
            }
            uint2 *dst = reinterpret_cast<uint2 *>(dst_px);
            dst[0] = o0;
            dst[1] = o1;
            dst[2] = o2;
        }
    }
    }  // YCbCr fast paths
}

// Each workgroup walks a run of consecutive tiles (kIdctThreads / blocks_per_mcu MCUs each) of one scan.
// Pipeline per tile:  lanes dequantise their block out of the LDS staging into registers -> barrier -> the staging is
// refilled for tile i+1 by LDS-DMA (global_load_lds_dwordx4: no VGPRs, asynchronous; the XOR swizzle is applied to the
// per-lane SOURCE address because the LDS side of the DMA is lane-linear) -> IDCT in registers while the DMA is in
// flight -> clamped samples to the LDS tile -> wait for the DMA -> barrier -> output assembly + global stores.
// All LDS lives in one array: staging 32 KiB | u8 sample tile [8 rows][256 blocks][8 B] 16 KiB | quant tables 512 B.
typedef __attribute__((address_space(3))) void jpgpu_lds_void;
typedef const __attribute__((address_space(1))) void jpgpu_gbl_void;

// PRE: the store already holds SAMPLES (the generic Dispose() pass of a progressive frame whose component slots do not map one
// to one onto its components, dispose_pass_kernel below): no dequantisation, no transform -- the block goes to the writer as it lies
// SPLIT: the scans of this launch were handed over as half-line planes (dma_tile below); a kernel name of its own, because the sixteen
// dense variants have no register to spare for a branch
// WIN: the scans of this launch belong to images decoded through a window (DevScan::win_*, cov_*): the work entries count MCUs of the
// window's cover, a raster of cov_cols x cov_rows MCUs of its own; a tile's coefficients are fetched MCU by MCU from the frame's store, the
// limits of a failing or short scan are compared in the scan's own numbering, and the stores go to the window.  Always dense.
template <int FMT, int LAY, bool PRE, bool SPLIT = false, bool WIN = false>
__device__ __forceinline__ void idct_output_body(
    const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans, const IdctWork *__restrict__ work,
    const DevScanStatus *__restrict__ status, const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ out, YccRgbFactors kf,
    OutputAffine aff = kOutputAffineIdentity) {
    constexpr int CONV = FMT == kFmtRgbU8 ? 3 : (FMT == kFmtRgbaU8 ? 4 : (FMT == kFmtRgbPlanarU8 ? kConvPlanar : (FMT == kFmtRgbPlanarF16 ? kConvPlanarF16 : (FMT == kFmtRgbPlanarF32 ? kConvPlanarF32 : 0))));  // fused YCbCr -> RGB(A), fast layouts and gray only
    constexpr bool kSampleBytes = fmt_is_sample_bytes(FMT);  // INTERLEAVED_U8 / _SCALED: one path, two sample-to-byte steps
    __shared__ __attribute__((aligned(16))) uint8_t sh_all[kIdctThreads * 128 + kIdctThreads * 64 + kMaxScanComponents * 256 + (SPLIT && !PRE ? 64 : 0)];
    uint8_t *sh = sh_all;
    uint8_t *sh_px = sh_all + kIdctThreads * 128;
    float(*sh_q)[64] = reinterpret_cast<float(*)[64]>(sh_all + kIdctThreads * 128 + kIdctThreads * 64);  // DevQuantTable::qf of the scan components
    uint8_t *sh_flag = sh_all + kIdctThreads * 128 + kIdctThreads * 64 + kMaxScanComponents * 256;  // split scans: two sets of eight flag words

    const IdctWork wk = work[blockIdx.x];
    const DevScan &s = scans[wk.scan];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = tid >> 6;
    const uint32_t bpm = s.blocks_per_mcu;
    const uint32_t mcus_per_tile = wk.mcus_per_tile;
    // MCUs the scan never reached (EOI met in a restart check, :144-150): the reference leaves their samples as the caller's
    // buffer held them -- zero in the buffer the batch owns -- so they go through the same output code with zero samples
    uint32_t decoded = status ? status[wk.scan].decoded_mcus : s.total_mcus;
    if (decoded > s.total_mcus) decoded = s.total_mcus;
    // ... and the same BLOCK by block for a scan that fails (round 5): the reference has called WriteBlock for every block in
    // front of the one it threw in and for none behind it (:99-134, 153; JpegHuffmanScanDecoder.cs:103-110), and a scan behind a
    // failed scan of the image was never started (Decode() left with the exception).
    uint32_t fail_block = 0xFFFFFFFFu;
    if (status != nullptr && s.kind == kScanSequential) {
        const uint32_t fb = status[wk.scan].pad[1];
        if (fb != 0) fail_block = kFailBlockBase - fb;
        for (uint32_t j = s.first_scan; j < wk.scan; j++)
            if (scans[j].image_index == s.image_index && status[j].first_error != kNoError) fail_block = 0;
    }
    // keep: the caller's canvas (jpgpu_decode_scan), or a scan ordered behind another scan of its image that wrote the same
    // component -- what this scan does not reach is not touched.  The YCbCr fast layouts assemble whole pixels of whole MCUs:
    // there the MCU the scan failed in is left to a launch of the bytewise form (first_mcu == kIdctPartialMcu).
    const bool keep = (s.shadow_mask & kKeepUnreachedMcus) != 0;
    constexpr bool kPerMcuLayout = fmt_is_interleaved(FMT) && (LAY == kLayYccH1V1 || LAY == kLayYccH2V1 || LAY == kLayYccH2V2);
    uint32_t first_mcu = wk.first_mcu;
    uint32_t range_end = wk.first_mcu + wk.n_mcus;
    // (WIN: the ranges below are in the scan's numbering, which is the cover's only where the cover is the whole scan; elsewhere the lanes'
    // own `reached` decides, as it does for every scan that keeps nothing)
    const bool win_whole = !WIN || (s.cov_x == 0 && s.cov_y == 0 && s.cov_cols == s.mcus_per_line);
    if (!WIN && first_mcu == kIdctPartialMcu) {
        if (fail_block == 0xFFFFFFFFu || fail_block % bpm == 0 || fail_block / bpm >= decoded) return;
        first_mcu = fail_block / bpm;
        range_end = first_mcu + 1;
    } else if (keep && win_whole) {
        const uint32_t reach = kPerMcuLayout ? fail_block / bpm : (fail_block == 0xFFFFFFFFu ? fail_block : (fail_block + bpm - 1) / bpm);
        if (range_end > decoded) range_end = decoded;
        if (range_end > reach) range_end = reach;
        if (first_mcu >= range_end) return;
    }

    // quantisation tables of the scan components: the floats the host made of them (they carry the transform's 1/8, in pair order)
    static_assert(kMaxScanComponents * 64 <= kIdctThreads, "one lane per table entry");
    if (tid < (uint32_t)s.scan_components * 64) {
        const uint32_t c = tid >> 6, i = tid & 63;
        sh_q[c][i] = quant_pool[s.quant_pool[s.comp[c].quant_slot]].qf[i];
    }

    const uint32_t mcu_local = tid / bpm;
    const uint32_t b = tid - mcu_local * bpm;
    const uint32_t ci_early = s.blk_comp[b < kMaxBlocksPerMcu ? b : 0];
    const uint8_t *coef_bytes = reinterpret_cast<const uint8_t *>(coefs + s.coef_off * 64);

    auto tile_mcus = [&](uint32_t first) { return (range_end - first) < mcus_per_tile ? (range_end - first) : mcus_per_tile; };
    // LDS-DMA of one tile: linear 16-byte slot c = k * 256 + tid (block c >> 3, slot c & 7) receives piece
    // (slot ^ swizzle(block)); the swizzle term ((block >> 1) & 7) does not depend on k, so every lane's source is
    // one fixed offset plus k * 4096.  Always a full tile: the coefficient buffer has a tile of slack behind it.
    const uint32_t tile_blocks = mcus_per_tile * bpm;
    // A scan handed over as half-line planes (common.h: kScanSplitHandoff).  The LDS side is the same; a lane's source is a 64-byte slot
    // -- lo plane for pieces 0..3, hi plane for pieces 4..7 of a flagged block; the hi pieces of an unflagged block are zeros, fetched
    // from the scan's zero line or written by the lane (dma_tile).  The flag bytes of a tile are fetched two tiles ahead, behind the
    // transform, and arrive under the wait the DMA has anyway (fetched as the byte that holds the block's bit, kept as one bit per block).
    static_assert(!(WIN && SPLIT), "a windowed image's scans are handed over dense");
    constexpr bool split = SPLIT && !PRE;
    if (split && (s.reserved0 & kScanSplitHandoff) == 0) return;  // (the host lists split scans apart: never taken)
    const uint32_t sp_dri = split ? s.dri : 1u;
    // Reciprocals for the block -> (MCU, interval) arithmetic.  (Wave-uniform, but a division leaves its result in a vector register: moved
    // to scalar ones, none is held across the transform.  The first from a table: a division of such small numbers is done in float, with
    // a fused multiply-add the parity claim's ISA test would count.)
    const uint32_t sp_rb = kRecip16[bpm <= (uint32_t)kMaxBlocksPerMcu ? bpm : 0];  // blk / bpm == blk * sp_rb >> 16 for blk < 256, bpm <= 16
    const uint32_t sp_rd = __builtin_amdgcn_readfirstlane(sp_dri <= 256u ? ((1u << 20) + sp_dri - 1) / sp_dri : 0u);  // x / dri == x * sp_rd >> 20 for x < dri + 256 <= 512
    // Tiles of whole PAIRS of intervals (the headline: 40 MCUs = five pairs of DRI = 4) are one contiguous run of slots in either plane: the
    // DMA then takes them in slot order -- a base plus constants, as the dense form does -- and the lane finds ITS block in the staging
    // instead (sp_own_block).  Other tiles gather block by block (sp_locate).
    const uint32_t sp_w = sp_dri * bpm;  // blocks of one interval
    const bool sp_fast = split && mcus_per_tile % (2 * sp_dri) == 0 && first_mcu % (2 * sp_dri) == 0;
    const uint32_t sp_rw = __builtin_amdgcn_readfirstlane((65536u + sp_w - 1) / sp_w);  // x / sp_w == x * sp_rw >> 16 for x < 128, sp_w <= 128
    const uint8_t *sp_hi = coef_bytes + split_plane_lines(s.n_intervals, sp_dri, bpm) * 128;
    const uint8_t *sp_flags = reinterpret_cast<const uint8_t *>(reinterpret_cast<const uint64_t *>(coefs) + (s.reserved0 >> kSplitFlagShift));
    // block k * 32 + (t >> 3) of the tile at tile_first: its line in either plane, its restart interval, its flag word.  No branches: the
    // sixteen DMAs of a tile are to be issued back to back
    auto sp_locate = [&](uint32_t tile_first, uint32_t t, uint32_t k, uint32_t &line, uint32_t &iv, uint32_t &word) {
        const uint32_t i0 = __builtin_amdgcn_readfirstlane(tile_first / sp_dri), m0 = tile_first - i0 * sp_dri;  // (wave-uniform)
        const uint32_t blk = k * 32 + (t >> 3);
        uint32_t q = (blk * sp_rb) >> 16;
        const uint32_t bb = blk - q * bpm;
        const uint32_t last = s.total_mcus - 1 - tile_first;  // lanes behind the scan's last MCU fetch that MCU's blocks: never past the region
        q = q < last ? q : last;
        const uint32_t mm = m0 + q;
        const uint32_t by_mul = (mm * sp_rd) >> 20, by_cmp = mm >= sp_dri ? 1u : 0u;
        const uint32_t qi = sp_dri > 256u ? by_cmp : by_mul;
        const uint32_t m = mm - qi * sp_dri;
        iv = i0 + qi;
        line = ((iv >> 1) * sp_dri + m) * bpm + bb;
        word = ((iv >> 6) * sp_dri + m) * bpm + bb;
    };
    // tiles of whole pairs: every DMA instruction takes 16 lines = 32 slots, the even intervals' slots into staging blocks k * 32 + 0..15 and
    // the odd intervals' into k * 32 + 16..31 -- the blocks of one interval, which neighbouring lanes dequantise, then lie side by side as
    // they do in the dense form, and the staging's swizzle keeps their reads apart.  Staging block k * 32 + (t >> 3): its interval, flag word
    auto sp_locate_fast = [&](uint32_t i0, uint32_t t, uint32_t k, uint32_t &iv, uint32_t &word) {  // i0: the tile's first interval (even)
        const uint32_t ll = k * 16 + ((t >> 3) & 15u);                  // line of the tile
        const uint32_t pp = (ll * sp_rw) >> 16;
        iv = i0 + 2 * pp + ((t >> 7) & 1u);
        iv = iv < s.n_intervals ? iv : s.n_intervals - 1;  // (slots behind the scan's last interval: any flag will do, inside the scan's words)
        word = (iv >> 6) * sp_w + (ll - pp * sp_w);
    };
    // ... and where the lane's own block (MCU t / bpm of the tile, block t % bpm) lies in that staging
    auto sp_own_block = [&](uint32_t t) {
        const uint32_t ml = (t * sp_rb) >> 16, bb = t - ml * bpm;
        const uint32_t ir = (ml * sp_rd) >> 20, m = ml - ir * sp_dri;  // (2 * dri <= MCUs per tile: the reciprocal holds)
        const uint32_t ll = ((ir >> 1) * sp_dri + m) * bpm + bb;
        return ((ll >> 4) << 5) | ((ir & 1u) << 4) | (ll & 15u);
    };
    // (the first interval of a tile of whole pairs, without a division per tile: sp_i0 is that of the tile in the staging)
    const uint32_t sp_ipt = __builtin_amdgcn_readfirstlane(mcus_per_tile / sp_dri);
    uint32_t sp_i0 = __builtin_amdgcn_readfirstlane(first_mcu / sp_dri);
    // One look-up per staging block: lane j looks up block j of the tile's staging (DMA instruction j >> 5, its slot j & 31), fetched as the
    // byte that holds the block's bit.  Behind the wait a ballot makes 64 bits per wave: the wave's two DMA instructions' 32 slots each, so
    // dword k of the eight in LDS is DMA instruction k's.  Written in front of a barrier the tile has anyway, read behind it.
    auto sp_load_flag = [&](uint32_t tile_first, uint32_t tile_i0, uint32_t &fb, uint32_t &bit_at) {
        uint32_t t_ = tid;
        asm volatile("" : "+v"(t_));
        const uint32_t k = t_ >> 5, t8 = (t_ & 31u) << 3;
        uint32_t line, iv, word;
        if (sp_fast) sp_locate_fast(tile_i0, t8, k, iv, word);
        else sp_locate(tile_first, t8, k, line, iv, word);
        fb = sp_flags[word * 8 + ((iv >> 3) & 7u)];  // (a scan's flag words are fewer than 2^29)
        bit_at = iv & 7u;
    };
    // The waits of the tile loop are inline assembly, which hipcc's wait-count pass does not read: it would take the flag byte's load -- issued
    // under one `if`, consumed under another -- for pending still, and guard the next write of its register with a vmcnt(0) of its own, behind
    // the task loop: a wait for the tile's own output stores (vmcnt retires in order).  The same wait again as an instruction it does read.
    auto sp_wait_seen = [&]() {
        if (split) __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0), expcnt untouched (gfx9 encoding)
    };
    auto sp_publish_flags = [&](uint32_t fb, uint32_t bit_at, uint32_t set) {
        asm volatile("" : "+v"(fb));  // (stays behind the wait in front of it)
        const uint64_t w = __builtin_amdgcn_ballot_w64(((fb >> bit_at) & 1u) != 0);
        if ((tid & 63u) == 0) *reinterpret_cast<uint2 *>(sh_flag + set * 32 + wave * 8) = uint2{(uint32_t)w, (uint32_t)(w >> 32)};
    };
    // -> bit k: block k * 32 + (tid >> 3) of the tile is flagged (one register from here to the tile's DMA)
    auto sp_read_flags = [&](uint32_t set) {
        const uint4 lo = *reinterpret_cast<const uint4 *>(sh_flag + set * 32), hi = *reinterpret_cast<const uint4 *>(sh_flag + set * 32 + 16);
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const uint32_t at = tid >> 3;
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) bits |= ((w[k] >> at) & 1u) << k;
        return bits;
    };
    auto dma_tile = [&](uint32_t tile_first, uint32_t tile_i0, uint32_t hi_bits) {
        // (recomputed per tile, three instructions, rather than kept in a register across the transform)
        uint32_t t_ = tid;
        asm volatile("" : "+v"(t_));
        if (split && sp_fast) {
            // every lane fetches: an unflagged block's hi pieces come from the 128 zero bytes in front of the scan's flag words (a line that
            // never leaves the L1), so the sixteen DMAs go out without a branch between them and nothing is written to the staging by hand
            const uint32_t piece = (t_ & 7) ^ ((t_ >> 4) & 7);
            const uint32_t slot = ((t_ >> 3) & 15u) * 2 + (t_ >> 7);  // of the instruction's 32
            const uint8_t *src = (piece < 4 ? coef_bytes : sp_hi) + (uint64_t)(tile_i0 >> 1) * sp_w * 128 + (slot * 64 + (piece & 3u) * 16);
            const uint8_t *zeros = sp_flags - 128 + (piece & 3u) * 16;
            const uint32_t fetch_bits = piece < 4 ? 0xFFu : hi_bits;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint8_t *from = ((fetch_bits >> k) & 1u) ? src + (uint32_t)(k * 2048) : zeros;
                if (k < 6 || (uint32_t)k * 32 + slot < tile_blocks)  // slots behind the tile's last block are not fetched
                    __builtin_amdgcn_global_load_lds((jpgpu_gbl_void *)from, (jpgpu_lds_void *)(sh + ((uint32_t)k * kIdctThreads + wave * 64) * 16), 16, 0, 0);
            }
            return;
        }
        if (split) {
            const uint32_t piece = (t_ & 7) ^ ((t_ >> 4) & 7);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                uint32_t line, iv, word;
                sp_locate(tile_first, t_, k, line, iv, word);
                const bool wanted = k < 6 || (uint32_t)k * 32 + (t_ >> 3) < tile_blocks;  // blocks behind the tile's last MCU are not fetched
                const bool fetch = wanted && (piece < 4 || ((hi_bits >> k) & 1u) != 0);
                const uint8_t *src = (piece < 4 ? coef_bytes : sp_hi) + ((uint64_t)line * 128 + (iv & 1u) * 64 + (piece & 3u) * 16);
                if (fetch)
                    __builtin_amdgcn_global_load_lds((jpgpu_gbl_void *)src, (jpgpu_lds_void *)(sh + ((uint32_t)k * kIdctThreads + wave * 64) * 16), 16, 0, 0);
                if (wanted && !fetch) *reinterpret_cast<uint4 *>(sh + ((uint32_t)k * kIdctThreads + t_) * 16) = uint4{0, 0, 0, 0};
            }
            return;
        }
        const uint32_t dma_lane_off = (t_ >> 3) * 128 + (((t_ & 7) ^ ((t_ >> 4) & 7)) * 16);
        const uint8_t *src = coef_bytes + (uint64_t)tile_first * bpm * 128;  // wave-uniform
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < 6 || (uint32_t)k * 32 + (tid >> 3) < tile_blocks)  // blocks behind the tile's last MCU are not fetched
                __builtin_amdgcn_global_load_lds((jpgpu_gbl_void *)(src + (uint32_t)(k * 4096) + dma_lane_off),
                                                 (jpgpu_lds_void *)(sh + ((uint32_t)k * kIdctThreads + wave * 64) * 16), 16, 0, 0);
    };

    // WIN: the tile's MCUs are consecutive in the cover, not in the store: every 16-byte piece is fetched from its own MCU -- MCU q of the
    // tile at tp (the tile's first MCU in the cover) is MCU (cov_x + column, cov_y + line) of the frame, found without a division
    // (k3_index_math.h).  Lanes behind the cover's last MCU fetch that MCU's blocks: never outside the scan's region.
    // (its 16-bit range hidden from the compiler: a division of such small numbers is done in float, with a fused multiply-add the parity
    // claim's ISA test would count)
    uint32_t win_mpl_ = WIN ? __builtin_amdgcn_readfirstlane((uint32_t)s.cov_cols) : 0u;
    if (WIN) asm("" : "+s"(win_mpl_));
    const uint32_t win_mpl = win_mpl_;
    const uint32_t win_recip = WIN ? __builtin_amdgcn_readfirstlane(k3_line_recip(win_mpl)) : 0u;
    auto dma_tile_win = [&](const K3TilePos &tp, uint32_t tile_first) {
        uint32_t t_ = tid;
        asm volatile("" : "+v"(t_));
        const uint32_t piece_off = ((t_ & 7) ^ ((t_ >> 4) & 7)) * 16;
        const uint32_t last = (uint32_t)s.cov_cols * s.cov_rows - 1 - tile_first;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t blk = (uint32_t)k * 32 + (t_ >> 3);
            uint32_t q = (blk * sp_rb) >> 16;
            const uint32_t bb = blk - q * bpm;
            q = q < last ? q : last;
            const uint32_t cx = tp.gx0 + q, wr = k3_line_wraps(cx, win_mpl, win_recip);
            const uint32_t mx = s.cov_x + cx - k3_mul24(wr, win_mpl), my = s.cov_y + tp.gy0 + wr;
            const uint32_t block = (my * s.mcus_per_line + mx) * bpm + bb;  // (a frame has fewer than 2^32 blocks)
            if (k < 6 || blk < tile_blocks)  // blocks behind the tile's last MCU are not fetched
                __builtin_amdgcn_global_load_lds((jpgpu_gbl_void *)(coef_bytes + (uint64_t)block * 128 + piece_off),
                                                 (jpgpu_lds_void *)(sh + ((uint32_t)k * kIdctThreads + wave * 64) * 16), 16, 0, 0);
        }
    };

    uint32_t hi_next = 0;  // split scans: the flag bits of the tile behind the one in the staging
    if (WIN) {
        dma_tile_win(k3_tile_pos(first_mcu, win_mpl), first_mcu);
    } else if (split) {
        // the first two tiles' flags, into the two sets of words (one look-up site for both: once per workgroup, not worth its code twice)
        const uint32_t n_sets = first_mcu + mcus_per_tile < range_end ? 2u : 1u;
#pragma nounroll
        for (uint32_t set = 0; set < n_sets; set++) {
            uint32_t fb, at;
            sp_load_flag(first_mcu + set * mcus_per_tile, sp_i0 + set * sp_ipt, fb, at);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            sp_wait_seen();
            sp_publish_flags(fb, at, set);
        }
        __syncthreads();
        const uint32_t hi_first = sp_read_flags(0);
        if (n_sets == 2) hi_next = sp_read_flags(1);
        dma_tile(first_mcu, sp_i0, hi_first);
    } else {
        dma_tile(first_mcu, sp_i0, 0);
    }
    // The place of the tile's first MCU in the image and what the output assembly divides by, wave-uniform (k3_index_math.h): one
    // division each per workgroup, none in the tile loop
    // (WIN: the place in the window's cover, whose lines are cov_cols MCUs long, and the window's lines)
    const uint32_t mpl = WIN ? win_mpl : __builtin_amdgcn_readfirstlane(s.mcus_per_line);
    const uint32_t line_recip = WIN ? win_recip : __builtin_amdgcn_readfirstlane(k3_line_recip(mpl));
    const uint32_t img_h = __builtin_amdgcn_readfirstlane(WIN ? (uint32_t)s.win_h : (uint32_t)s.height);
    uint8_t *const img = out + s.out_off;  // (read here: the waits of the tile loop keep a load inside it from being moved out)
    K3TilePos pos = k3_tile_pos(first_mcu, mpl);
    pos.gx0 = __builtin_amdgcn_readfirstlane(pos.gx0);
    pos.gy0 = __builtin_amdgcn_readfirstlane(pos.gy0);
    K3TilePos pos_step = k3_tile_pos(mcus_per_tile, mpl);
    pos_step.gx0 = __builtin_amdgcn_readfirstlane(pos_step.gx0);
    pos_step.gy0 = __builtin_amdgcn_readfirstlane(pos_step.gy0);
    // (a run's last tile may be shorter: its reciprocal apart)
    const uint32_t row_recip_full = __builtin_amdgcn_readfirstlane(k3_row_recip(mcus_per_tile));
    const uint32_t row_recip_last = __builtin_amdgcn_readfirstlane(k3_row_recip((range_end - first_mcu - 1) % mcus_per_tile + 1));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

  for (uint32_t tile_first = first_mcu; tile_first < range_end; tile_first += mcus_per_tile) {
    const uint32_t n_mcu = tile_mcus(tile_first);
    const uint32_t n_blk = n_mcu * bpm;
    const uint32_t next_first = tile_first + mcus_per_tile;
    const bool have_next = next_first < range_end;

    uint32_t mcu = tile_first + mcu_local;  // (WIN: in the cover's numbering until the transform is done)
    const bool have_block = tid < n_blk;
    // a scan component whose frame component a LATER scan component also resolves to: the reference writes its blocks first
    // and the later component's over them (WriteBlock by ComponentIndex, :118-134), so only the later ones reach the output
    bool writes = have_block && ((s.shadow_mask >> ci_early) & 1u) == 0;

    // phase B1: this lane's block out of the staging into registers, as packed words
    uint32_t cw[32];  // int16 coefficient pairs, zig-zag
    uint32_t px[32];  // int16 sample pairs
    if (PRE) {
        if (have_block) {
#pragma unroll
            for (int piece = 0; piece < 8; piece++) {  // (block_load, written out: through it the six flush listings come out in another order)
                const uint4 cv = *reinterpret_cast<const uint4 *>(sh + tid * 128 + ((piece ^ ((tid >> 1) & 7)) * 16));
                px[piece * 4] = cv.x;
                px[piece * 4 + 1] = cv.y;
                px[piece * 4 + 2] = cv.z;
                px[piece * 4 + 3] = cv.w;
            }
        }
    } else {
        // The lane's eight swizzled staging addresses do not change from tile to tile; hipcc computes them in front of the tile
        // loop -- and in the three variants with the most state in their output assembly spills five of them to scratch for
        // the length of the transform.  There they are derived again in every tile (sixteen instructions) from a copy of the
        // lane id the compiler cannot see through.
        constexpr bool kPerTile = split || (FMT == kFmtRgbU8 && (LAY == kLayYccH2V1 || LAY == kLayYccH2V2)) || (kSampleBytes && LAY == kLayGeneric);
        uint32_t t_ = tid;
        if (kPerTile) asm volatile("" : "+v"(t_));
        if (split && sp_fast) t_ = sp_own_block(t_);  // (the staging is in slot order)
        if (have_block) block_load(sh + t_ * 128, (t_ >> 1) & 7, cw);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every lane holds its coefficients: the staging can be refilled
    if (WIN) {
        K3TilePos pos_next = pos;
        k3_tile_advance(pos_next, pos_step, mpl);
        if (have_next) dma_tile_win(pos_next, next_first);
    } else if (have_next) dma_tile(next_first, sp_i0 + sp_ipt, hi_next);  // in flight during the whole transform below
    hi_next = 0;  // (dead from here to the flag bytes behind the transform)

    // phase B2: dequantisation + IDCT entirely in registers
    if (!PRE && have_block) block_idct(cw, sh_q[ci_early], (int32_t)s.level_shift, px);
    // split scans: the flag bytes of the tile after the next one, fetched behind the transform (its registers are dead) and waited for where the DMA is
    uint32_t sp_fb = 0, sp_at = 0;
    const bool sp_ahead = split && next_first + mcus_per_tile < range_end;
    if (sp_ahead) sp_load_flag(next_first + mcus_per_tile, sp_i0 + 2 * sp_ipt, sp_fb, sp_at);
    sp_i0 += sp_ipt;
    // WIN: the MCU's place in the frame, and with it its number in the scan, which `decoded` and `fail_block` count in
    uint32_t win_mx = 0, win_my = 0;
    if (WIN) {
        uint32_t ml_win = mcu_local;
        asm volatile("" : "+v"(ml_win));
        const uint32_t wr = k3_line_wraps(pos.gx0 + ml_win, mpl, line_recip);
        win_mx = s.cov_x + pos.gx0 + ml_win - k3_mul24(wr, mpl);
        win_my = s.cov_y + pos.gy0 + wr;
        mcu = win_my * s.mcus_per_line + win_mx;
    }
    // (a frame has fewer than 2^32 blocks: 32-bit arithmetic; computed behind the transform, nothing more alive across it)
    const bool reached = mcu < decoded && mcu * bpm + b < fail_block;
    if ((s.shadow_mask & 0xFu) == 0) {
        writes = writes && (reached || !keep);
    } else {
        // A scan that names a frame component twice (a corrupted selector; uniform branch): the reference writes the blocks in scan
        // order, so at every place the LAST block that reached the writer stands -- the later duplicate's wherever the scan got to
        // it, the earlier one's in the MCU the scan failed in BETWEEN the two (:118-134), zeros (in the batch's own buffer) where
        // neither got.  Exactly one lane writes each place: a reached block unless the later duplicate's block at its place is
        // reached too; an unreached block only if it is the last duplicate and no earlier duplicate's block is there either.
        const uint32_t bb = b < kMaxBlocksPerMcu ? b : 0u, me = s.blk_comp[bb], fc = s.comp[me & 3u].component_index;
        uint32_t later = 0xFFu, earlier = 0xFFu;  // scan components: the nearest duplicates of this block's
        for (uint32_t cc = 0; cc < s.scan_components && cc < (uint32_t)kMaxScanComponents; cc++) {
            if (cc == me || s.comp[cc].component_index != fc) continue;
            if (cc > me && later == 0xFFu) later = cc;
            if (cc < me) earlier = cc;
        }
        uint32_t first_me = 0xFFu, first_later = 0xFFu, first_earlier = 0xFFu;  // their first blocks in the MCU
        for (uint32_t k = 0; k < bpm && k < (uint32_t)kMaxBlocksPerMcu; k++) {
            const uint32_t ck = s.blk_comp[k];
            if (ck == me && first_me == 0xFFu) first_me = k;
            if (ck == later && first_later == 0xFFu) first_later = k;
            if (ck == earlier && first_earlier == 0xFFu) first_earlier = k;
        }
        const bool later_reached = later != 0xFFu && mcu < decoded && mcu * bpm + (b - first_me + first_later) < fail_block;
        const bool earlier_reached = earlier != 0xFFu && mcu < decoded && mcu * bpm + (b - first_me + first_earlier) < fail_block;
        writes = have_block && (reached ? !later_reached : (!keep && later == 0xFFu && !earlier_reached));
    }
    if (!reached) {
#pragma unroll
        for (int i = 0; i < 32; i++) px[i] = 0;
    }
    bool synced = false;
    // the MCU's place in the image is only needed from here on: computed behind the transform (an empty asm the compiler may not
    // move across keeps it from being hoisted in front of it), two registers fewer are alive while those of the
    // transform are -- what four of the sixteen variants spilled when it held 64 + 32 (profiles/r03_kernel_resources.txt)
    uint32_t ml_late = mcu_local, b_late = b;
    asm volatile("" : "+v"(ml_late), "+v"(b_late));
    const uint32_t mcu_wraps = k3_line_wraps(pos.gx0 + ml_late, mpl, line_recip);  // (lines below the tile's first MCU line: no division per lane)
    uint32_t mcu_back = k3_mul24(mcu_wraps, mpl);
    asm("" : "+v"(mcu_back));  // (kept a 24-bit product, as in the task loop)
    const uint32_t mcu_y = WIN ? win_my : pos.gy0 + mcu_wraps, mcu_x = WIN ? win_mx : pos.gx0 + ml_late - mcu_back;
    const uint32_t ci = s.blk_comp[b_late < kMaxBlocksPerMcu ? b_late : 0];  // (again: one byte from the L1-resident descriptor)
    const DevScanComponent comp = s.comp[ci];
    // (the split form indexes the block's place with the late copy: an address derived from `b` would be held across the whole tile loop)
    const uint32_t b_out = split ? b_late : b;

    if (FMT == kFmtPlanarI16) {
        // "O1": unclamped int16 at component-native resolution, planes padded to whole MCUs
        if (writes) {
            int16_t *plane = reinterpret_cast<int16_t *>(out + s.out_off + s.plane_off[ci]);
            const uint32_t pitch = s.plane_pitch[ci];
            const uint32_t x0 = (mcu_x * comp.h + s.blk_x[b_out]) * 8, y0 = (mcu_y * comp.v + s.blk_y[b_out]) * 8;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint4 v = {px[r * 4 + 0], px[r * 4 + 1], px[r * 4 + 2], px[r * 4 + 3]};
                *reinterpret_cast<uint4 *>(plane + (size_t)(y0 + r) * pitch + x0) = v;
            }
        }
    } else {
    // u8 formats: clamp (signed, like JpegBufferOutputWriter8Bit.ClampTo8Bit) and pack 8 samples per row
    uint2 rows[8];
    if constexpr (FMT == kFmtInterleavedU8Scaled) {
        const ScaleTo8 k8 = scale_to_8(s.precision);  // (wave-uniform: scalar registers)
        if (k8.expand) {
#pragma unroll
            for (int r = 0; r < 8; r++) {  // bytes 0, 2 of one pair, then 0, 2 of the next
                rows[r].x = __builtin_amdgcn_perm(expand2_u8(px[r * 4 + 1], k8), expand2_u8(px[r * 4 + 0], k8), 0x06040200u);
                rows[r].y = __builtin_amdgcn_perm(expand2_u8(px[r * 4 + 3], k8), expand2_u8(px[r * 4 + 2], k8), 0x06040200u);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) {  // bytes 0, 1 of one pair, then 0, 1 of the next
                rows[r].x = __builtin_amdgcn_perm(shift_sat2_u8(px[r * 4 + 1], k8), shift_sat2_u8(px[r * 4 + 0], k8), 0x05040100u);
                rows[r].y = __builtin_amdgcn_perm(shift_sat2_u8(px[r * 4 + 3], k8), shift_sat2_u8(px[r * 4 + 2], k8), 0x05040100u);
            }
        }
    } else {
#pragma unroll
    for (int r = 0; r < 8; r++) {
        rows[r].x = pack4_u8(px[r * 4 + 0], px[r * 4 + 1]);
        rows[r].y = pack4_u8(px[r * 4 + 2], px[r * 4 + 3]);
    }
    }

    if (CONV != 0 && !conv_is_planar(CONV) && LAY == kLayGray) {
        // a single-component image as R = G = B = Y (Cb = Cr = 128 contribute nothing, DecodeAction.cs:57-65)
        if (writes) {
            // (WIN: the block's place in the window -- its column is inside, idct_window_layout_class; a line above the window wraps)
            const uint32_t x0 = (mcu_x * comp.h + s.blk_x[b_out]) * 8 - (WIN ? s.win_x : 0u), y0 = (mcu_y * comp.v + s.blk_y[b_out]) * 8 - (WIN ? s.win_y : 0u);
#pragma unroll
            for (int r = 0; r < 8; r++) {
                if (y0 + r >= (WIN ? s.win_h : s.height)) continue;
                uint32_t px[8];
#pragma unroll
                for (int j = 0; j < 8; j++) px[j] = byte_of(rows[r].x, rows[r].y, j) * 0x010101u;
                store_rgb_pixels<8, (CONV == 4 ? 4 : 3)>(out + s.out_off + ((size_t)(y0 + r) * (WIN ? s.win_w : s.width) + x0) * (CONV == 4 ? 4 : 3), px);
            }
        }
    } else if (FMT == kFmtPlanarU8 || (kSampleBytes && LAY == kLayGray)) {
        static_assert(!WIN || !(FMT == kFmtPlanarU8 || (kSampleBytes && LAY == kLayGray)), "no window form: such work takes the generic layout");
        // planar u8 (planes padded to whole MCUs), or a single-component interleaved image (same addressing,
        // pitch = W, clipped at the bottom; the host only picks kLayGray when W is a multiple of 8)
        if (writes) {
            const bool gray = kSampleBytes;
            uint8_t *plane = out + s.out_off + (gray ? 0 : s.plane_off[ci]);
            const uint32_t pitch = gray ? s.width : s.plane_pitch[ci];
            const uint32_t x0 = (mcu_x * comp.h + s.blk_x[b_out]) * 8, y0 = (mcu_y * comp.v + s.blk_y[b_out]) * 8;
#pragma unroll
            for (int r = 0; r < 8; r++)
                if (!gray || y0 + r < s.height) *reinterpret_cast<uint2 *>(plane + (size_t)(y0 + r) * pitch + x0) = rows[r];
        }
    } else {
    // ---- interleaved u8 ("O2", JpegBufferOutputWriter8Bit semantics): stage the clamped samples in LDS, tile[r][block]
    if (have_block) {
#pragma unroll
        for (int r = 0; r < 8; r++) *reinterpret_cast<uint2 *>(sh_px + r * kPxRowStride + tid * 8) = rows[r];
    }
    // The DMA of the next tile has had the whole transform to land.  Wait for it BEFORE this tile's global stores are
    // issued (vmcnt retires in order: waiting later would also wait for those stores to drain), then one barrier
    // publishes both the sample tile and the refilled staging.
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    sp_wait_seen();
    if (sp_ahead) sp_publish_flags(sp_fb, sp_at, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    synced = true;

    // (tile_mcus clamps at range_end only, so at most the run's LAST tile is short: two reciprocals cover every n_mcu; a tile walk that
    // shortens another tile needs its own)
    if constexpr (WIN)
        interleaved_output_from_tile<LAY, CONV, true>(sh_px, s, pos, mpl, line_recip, n_mcu == mcus_per_tile ? row_recip_full : row_recip_last, img_h, n_mcu, tid,
                                                      writes, comp, mcu_x, mcu_y, b, img, kf, reached, mcu, fail_block, aff,
                                                      (uint32_t)s.win_y - (uint32_t)s.cov_y * 8u * s.max_v);
    else
    interleaved_output_from_tile<LAY, CONV>(sh_px, s, pos, mpl, line_recip, n_mcu == mcus_per_tile ? row_recip_full : row_recip_last, img_h, n_mcu, tid,
                                            writes, comp, mcu_x, mcu_y, b, img, kf, reached, mcu, fail_block, aff);
    }  // interleaved
    }  // u8 formats

    if (!synced) {  // planar / gray paths: publish the refilled staging
        asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
        sp_wait_seen();
        if (sp_ahead) sp_publish_flags(sp_fb, sp_at, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    // (behind the output assembly, off the path from the barrier to the tile's stores; the words are next written behind the next tile's first barrier)
    if (sp_ahead) hi_next = sp_read_flags(0);
    k3_tile_advance(pos, pos_step, mpl);
  }  // tile loop
}


hipError_t launch_extend_u16(hipStream_t stream, const uint8_t *planes, uint8_t *out_base, const ExtendPlanes *images, int n_images,
                             uint32_t max_pixels) {
    if (n_images <= 0 || max_pixels == 0) return hipSuccess;
    const uint32_t bx = (uint32_t)std::min<uint64_t>(((uint64_t)max_pixels + 255) / 256, 4096);
    for (int base = 0; base < n_images; base += 65535) {  // grid.y limit
        const int n = n_images - base < 65535 ? n_images - base : 65535;
        hipLaunchKernelGGL(extend_u16_kernel, dim3(bx, (uint32_t)n), dim3(256), 0, stream, planes, out_base, images + base);
    }
    return hipGetLastError();
}


// A scan handed over as half-line planes, written out as the dense int16[blocks][64] every reader outside K3 expects (coefficient
// download, the device pointer, a caller about to overwrite coefficients): lo slot + hi slot of a flagged block, zeros for the hi half of
// an unflagged one.  Same offsets in both buffers; eight lanes per block.
__global__ __launch_bounds__(256) void expand_handoff_kernel(const int16_t *__restrict__ coefs, int16_t *__restrict__ dense,
                                                             const DevScan *__restrict__ scans, const uint32_t *__restrict__ scan_ids) {
    const DevScan &s = scans[scan_ids[blockIdx.y]];
    const uint32_t bpm = s.blocks_per_mcu, dri = s.dri;
    const uint32_t n_blocks = s.total_mcus * bpm;
    const uint8_t *lo = reinterpret_cast<const uint8_t *>(coefs + s.coef_off * 64);
    const uint8_t *hi = lo + split_plane_lines(s.n_intervals, dri, bpm) * 128;
    const uint64_t *flags = reinterpret_cast<const uint64_t *>(coefs) + (s.reserved0 >> kSplitFlagShift);
    const uint32_t piece = threadIdx.x & 7;
    for (uint32_t g = blockIdx.x * 32 + (threadIdx.x >> 3); g < n_blocks; g += gridDim.x * 32) {
        const uint32_t mcu = g / bpm, b = g - mcu * bpm;
        const uint32_t i = mcu / dri, m = mcu - i * dri;
        const uint64_t off = split_slot(i, m, b, dri, bpm) * 64 + (piece & 3) * 16;
        uint4 v = {0, 0, 0, 0};
        if (piece < 4) v = *reinterpret_cast<const uint4 *>(lo + off);
        else if ((flags[split_flag_word(i, m, b, dri, bpm)] >> (i & 63u)) & 1u) v = *reinterpret_cast<const uint4 *>(hi + off);
        *reinterpret_cast<uint4 *>(dense + (s.coef_off + g) * 64 + piece * 8) = v;
    }
}
hipError_t launch_expand_handoff(hipStream_t stream, const int16_t *coefs, int16_t *dense, const DevScan *scans, const uint32_t *scan_ids, int n_scans,
                                 uint32_t max_blocks) {
    if (n_scans <= 0 || max_blocks == 0) return hipSuccess;
    const uint32_t bx = (uint32_t)std::min<uint64_t>(((uint64_t)max_blocks + 31) / 32, 2048);
    for (int base = 0; base < n_scans; base += 65535) {  // grid.y limit
        const int n = n_scans - base < 65535 ? n_scans - base : 65535;
        hipLaunchKernelGGL(expand_handoff_kernel, dim3(bx, (uint32_t)n), dim3(256), 0, stream, coefs, dense, scans, scan_ids + base);
    }
    return hipGetLastError();
}

template <int FMT, int LAY>
__global__ __launch_bounds__(kIdctThreads, (FMT == kFmtPlanarI16 ? 2 : 3)) void idct_output_kernel(
    const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans, const IdctWork *__restrict__ work,
    const DevScanStatus *__restrict__ status, const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ out, YccRgbFactors kf, OutputAffine aff) {
    idct_output_body<FMT, LAY, false>(coefs, scans, work, status, quant_pool, out, kf, aff);
}
template <int FMT, int LAY>
__global__ __launch_bounds__(kIdctThreads, (FMT == kFmtPlanarI16 ? 2 : 3)) void idct_split_kernel(
    const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans, const IdctWork *__restrict__ work,
    const DevScanStatus *__restrict__ status, const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ out, YccRgbFactors kf, OutputAffine aff) {
    idct_output_body<FMT, LAY, false, true>(coefs, scans, work, status, quant_pool, out, kf, aff);
}
template <int FMT>
__global__ __launch_bounds__(kIdctThreads, 2) void flush_output_kernel(
    const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans, const IdctWork *__restrict__ work,
    const DevScanStatus *__restrict__ status, const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ out, YccRgbFactors kf) {
    idct_output_body<FMT, kLayGeneric, true>(coefs, scans, work, status, quant_pool, out, kf);
}

// The window forms (idct_output_body's WIN): kernels of their own, launched for the work of windowed images only, so that whole-frame work
// pays nothing for the window.  The generic layout of the two sample-byte formats (which is also where the RGB formats' generic class writes
// its scratch image), the four fast layouts of RGB_U8 and RGB_PLANAR_U8 / _F16 / _F32, and the flush of a store that holds samples.
template <int FMT, int LAY>
__global__ __launch_bounds__(kIdctThreads, 3) void idct_window_kernel(
    const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans, const IdctWork *__restrict__ work,
    const DevScanStatus *__restrict__ status, const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ out, YccRgbFactors kf, OutputAffine aff) {
    idct_output_body<FMT, LAY, false, false, true>(coefs, scans, work, status, quant_pool, out, kf, aff);
}
template <int FMT>
__global__ __launch_bounds__(kIdctThreads, 2) void flush_window_kernel(
    const int16_t *__restrict__ coefs, const DevScan *__restrict__ scans, const IdctWork *__restrict__ work,
    const DevScanStatus *__restrict__ status, const DevQuantTable *__restrict__ quant_pool, uint8_t *__restrict__ out, YccRgbFactors kf) {
    idct_output_body<FMT, kLayGeneric, true, false, true>(coefs, scans, work, status, quant_pool, out, kf);
}

// The reference's Dispose() as it is written (ScanDecoder/JpegHuffmanProgressiveScanDecoder.cs:421-470): every component SLOT of
// the scan decoder, as the last scans left it, dequantises + transforms + level-shifts the blocks of its component IN PLACE.  For
// files in the usual scan order that is one transform per component and K3 does it on the way to the writer.  When the slots
// do not map one to one onto the components (a file whose last scan of slot 0 is not the first component: e.g. slots
// {Cb, Cb, Cr}) a component is transformed twice -- the second time reading its own samples as zig-zag coefficients -- and
// another never (its quantised coefficients reach the writer as samples); a file without any scan flushes zeros.  This kernel
// does literally that to the frame's store, one lane per block, `n` transforms with the slots' tables in slot order;
// flush_output_kernel then writes the store out.  (Both also serve the partial flush of a progressive file that failed.)
__global__ __launch_bounds__(64) void dispose_pass_kernel(int16_t *__restrict__ coefs, const DisposeJob *__restrict__ jobs,
                                                          const DevQuantTable *__restrict__ quant_pool) {
    const DisposeJob &j = jobs[blockIdx.y];
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= j.n_blocks) return;
    const uint32_t c = j.blk_comp[g % j.bpm];
    const uint32_t n = j.n[c];
    if (n == 0) return;
    int16_t *blk = coefs + (j.coef_off + g) * 64;
    uint32_t w[32];
    block_load(reinterpret_cast<const uint8_t *>(blk), 0, w);  // (from the store itself: no swizzle)
    for (uint32_t t = 0; t < n; t++) {
        const uint16_t *q = quant_pool[j.quant[c][t]].q;
        float f[64];
#pragma unroll
        for (int k = 0; k < 64; k++) {
            const int32_t cv = (k & 1) ? ((int32_t)w[k >> 1] >> 16) : (int32_t)(int16_t)(w[k >> 1] & 0xFFFFu);
            f[kNat[k]] = (float)((int32_t)q[k] * cv);  // ushort * short -> int -> float (DequantizeBlockAndUnZigZag)
        }
        block_idct_dequantised(f, (int32_t)j.level_shift, w);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) reinterpret_cast<uint4 *>(blk)[i] = make_uint4(w[i * 4], w[i * 4 + 1], w[i * 4 + 2], w[i * 4 + 3]);
}

// What every launch of one call shares.
struct K3LaunchArgs {
    hipStream_t stream;
    const int16_t *coefs;
    const DevScan *scans;
    const DevScanStatus *status;
    const DevQuantTable *quant_pool;
    uint8_t *out, *generic_out;
    YccRgbFactors kf;
    OutputAffine aff;
};

// Kernel <FMT, LAY> of FORM, if that is the one the rule names (v) -- instantiated exactly where the rule reaches it from some (format, class):
// kernels.h, k3_variant_compiled.  The formats whose kernels read neither kf nor aff get the caller's all the same.
template <int FORM, int FMT, int LAY>
static bool launch_k3_variant_if(const K3Variant &v, const K3LaunchArgs &a, const IdctWork *w, int n) {
    if (v.fmt != FMT || v.lay != LAY) return false;
    uint8_t *const dst = v.to_scratch ? a.generic_out : a.out;
    if constexpr (k3_variant_compiled(FORM, false, FMT, LAY)) {
        if (!v.pre) {
            if constexpr (FORM == kK3Dense)
                hipLaunchKernelGGL((idct_output_kernel<FMT, LAY>), dim3(n), dim3(kIdctThreads), 0, a.stream, a.coefs, a.scans, w, a.status, a.quant_pool, dst, a.kf, a.aff);
            else if constexpr (FORM == kK3Split)
                hipLaunchKernelGGL((idct_split_kernel<FMT, LAY>), dim3(n), dim3(kIdctThreads), 0, a.stream, a.coefs, a.scans, w, a.status, a.quant_pool, dst, a.kf, a.aff);
            else
                hipLaunchKernelGGL((idct_window_kernel<FMT, LAY>), dim3(n), dim3(kIdctThreads), 0, a.stream, a.coefs, a.scans, w, a.status, a.quant_pool, dst, a.kf, a.aff);
            return true;
        }
    }
    if constexpr (k3_variant_compiled(FORM, true, FMT, LAY)) {
        static_assert(LAY == kLayGeneric && FORM != kK3Split, "the flush kernels: one per format, dense or window");
        if (v.pre) {
            if constexpr (FORM == kK3Dense)
                hipLaunchKernelGGL((flush_output_kernel<FMT>), dim3(n), dim3(kIdctThreads), 0, a.stream, a.coefs, a.scans, w, a.status, a.quant_pool, dst, a.kf);
            else
                hipLaunchKernelGGL((flush_window_kernel<FMT>), dim3(n), dim3(kIdctThreads), 0, a.stream, a.coefs, a.scans, w, a.status, a.quant_pool, dst, a.kf);
            return true;
        }
    }
    return false;
}
// The run-time (format, class) of n > 0 workgroups to the compile-time <FMT, LAY> of the rule's answer, over every format and layout.
// false: the rule has no kernel for such work (the planner lists none: a missing kernel is an error).
template <int FORM, int... I>
static bool launch_k3_variant(int format, int layout_class, const K3LaunchArgs &a, const IdctWork *w, int n, std::integer_sequence<int, I...>) {
    const K3Variant v = k3_variant(format, layout_class, FORM);
    return v.exists && (launch_k3_variant_if<FORM, I / kNumIdctLayouts, I % kNumIdctLayouts>(v, a, w, n) || ...);
}

// work is sorted by layout class; class_begin[c]..class_begin[c+1] are the workgroups of class c, in form `form` up to split_begin[c] (where
// given) and from there on those of scans handed over as half-line planes.
static hipError_t launch_k3_classes(const K3LaunchArgs &a, const IdctWork *work, const int *class_begin, const int *split_begin, int format, K3Form form) {
    constexpr auto kVariants = std::make_integer_sequence<int, kNumOutputFormats * kNumIdctLayouts>();
    for (int c = 0; c < kNumIdctLayoutClasses; c++) {
        const int n = class_begin[c + 1] - class_begin[c];
        if (n <= 0) continue;
        const int nd = split_begin ? split_begin[c] - class_begin[c] : n;
        const IdctWork *w = work + class_begin[c];
        if (nd > 0 && !(form == kK3Window ? launch_k3_variant<kK3Window>(format, c, a, w, nd, kVariants) : launch_k3_variant<kK3Dense>(format, c, a, w, nd, kVariants)))
            return hipErrorInvalidValue;
        if (n > nd && !launch_k3_variant<kK3Split>(format, c, a, w + nd, n - nd, kVariants)) return hipErrorInvalidValue;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The work of windowed images (the planner lists it apart, by the class idct_window_layout_class gives; never split).  Work under a format
// that is not assembled from whole pixels, or of a class without a window kernel: hipErrorInvalidValue.
hipError_t launch_idct_window(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const IdctWork *work,
                              const int class_begin[kNumIdctLayoutClasses + 1], const DevScanStatus *status, const DevQuantTable *quant_pool, uint8_t *out,
                              int format, const YccRgbFactors &kf, uint8_t *generic_out, const OutputAffine &aff) {
    return launch_k3_classes({stream, coefs, scans, status, quant_pool, out, generic_out, kf, aff}, work, class_begin, nullptr, format, kK3Window);
}

hipError_t launch_idct(hipStream_t stream, const int16_t *coefs, const DevScan *scans, const IdctWork *work,
                       const int class_begin[kNumIdctLayoutClasses + 1], const DevScanStatus *status,
                       const DevQuantTable *quant_pool, uint8_t *out, int format, const YccRgbFactors &kf, uint8_t *generic_out,
                       const int *split_begin, const OutputAffine &aff) {
    return launch_k3_classes({stream, coefs, scans, status, quant_pool, out, generic_out, kf, aff}, work, class_begin, split_begin, format, kK3Dense);
}

// INTERLEAVED_U8 image (comps = 1 or 3) -> RGB / RGBA (bpp = 3 / 4) or the three planes of RGB_PLANAR_U8 (bpp = 1), for the layouts without a fused path;
// sample_bytes = 2 / 4 (with bpp = 1): the planes of RGB_PLANAR_F16 / _F32
hipError_t launch_ycc_to_rgb(hipStream_t stream, const uint8_t *src, uint8_t *dst, uint64_t n_pixels, int comps, int bpp, const YccRgbFactors &kf,
                             int sample_bytes, const OutputAffine &aff) {
    if (n_pixels == 0) return hipSuccess;
    const uint64_t want = (n_pixels + 255) / 256;
    const int grid = (int)(want < 65536 ? want : 65536);
    if (sample_bytes == 2) {
        hipLaunchKernelGGL(ycc_to_rgb_planes_kernel<_Float16>, dim3(grid), dim3(256), 0, stream, src, reinterpret_cast<_Float16 *>(dst), n_pixels, comps, kf, aff);
        return hipGetLastError();
    }
    if (sample_bytes == 4) {
        hipLaunchKernelGGL(ycc_to_rgb_planes_kernel<float>, dim3(grid), dim3(256), 0, stream, src, reinterpret_cast<float *>(dst), n_pixels, comps, kf, aff);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(ycc_to_rgb_kernel, dim3(grid), dim3(256), 0, stream, src, dst, n_pixels, comps, bpp, kf);
    return hipGetLastError();
}


hipError_t launch_dispose_pass(hipStream_t stream, int16_t *coefs, const DisposeJob *jobs, int n_jobs, uint32_t max_blocks, const DevQuantTable *quant_pool) {
    if (n_jobs <= 0 || max_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(dispose_pass_kernel, dim3((max_blocks + 63u) / 64u, n_jobs), dim3(64), 0, stream, coefs, jobs, quant_pool);
    return hipGetLastError();
}

// Layout class of a scan for the formats K3 assembles from whole pixels (fmt_is_interleaved; 0 = generic bytewise path).
// RGB_PLANAR_U8 stores 8 (kLayGray, kLayYccH1V1) or 16 bytes (kLayYccH2V1 / H2V2) per lane and plane, at plane c's base out_off + c * W * H plus
// y * W + 8 or 16 * (MCU column): with W and out_off multiples of 8 / 16, as the conditions below ask, every plane base and every row start
// is aligned for that store.  RGB_PLANAR_F16 / _F32 store 16-byte pieces at out_off + c * W * H * sizeof(T) + (y * W + 8 or 16 * (MCU column)) * sizeof(T):
// W a multiple of 8 makes every term but out_off a multiple of 16 in both types, and out_off is a multiple of 256 (DeviceBatch::plan_image; 0 for a
// single job).
int idct_layout_class(const DevScan &s) {
    const uint32_t W = s.width;
    if (s.frame_components == 1 && s.scan_components == 1 && s.comp[0].h == 1 && s.comp[0].v == 1 && (W % 8) == 0 && (s.out_off % 8) == 0)
        return kLayGray;
    const bool ycc = s.frame_components == 3 && s.scan_components == 3 && s.comp[0].component_index == 0 &&
                     s.comp[1].component_index == 1 && s.comp[2].component_index == 2 && s.comp[0].hs == 1 && s.comp[0].vs == 1 &&
                     s.comp[1].h == 1 && s.comp[1].v == 1 && s.comp[2].h == 1 && s.comp[2].v == 1;
    if (!ycc) return kLayGeneric;
    if (s.max_h == 1 && s.max_v == 1 && (W % 8) == 0 && (s.out_off % 8) == 0) return kLayYccH1V1;
    if (s.max_h == 2 && (W % 16) == 0 && (s.out_off % 16) == 0) {
        if (s.max_v == 1) return kLayYccH2V1;
        if (s.max_v == 2) return kLayYccH2V2;
    }
    return kLayGeneric;
}

// Layout class of a scan of a windowed image: today's rule with the window's width in place of the frame's, and the window's first column on
// an MCU boundary -- so the cover's first MCU column starts at the window's first pixel, the window is whole MCUs wide, and every store address
// of the fast classes keeps the alignment it has for a whole frame (a line is win_w samples, an image starts on a multiple of 256).  win_y and
// win_h are free.  A format without a window kernel for the fast class (k3_variant: all but RGB_U8 and RGB_PLANAR_U8 / _F16 / _F32) takes the
// generic class under a window (RGBA_U8 through the scratch image and the converter).
int idct_window_layout_class(const DevScan &s, int format) {
    if (s.max_h == 0 || s.win_x % (8u * s.max_h) != 0) return kLayGeneric;
    DevScan w = s;
    w.width = s.win_w;
    const int cls = idct_layout_class(w);
    return k3_variant(format, cls, kK3Window).exists ? cls : kLayGeneric;
}

}  // namespace jpgpu
