// jpeglibrary_amd/csrc/k4_resample_body.h -- the body of K4's kernels, for NP tight uint8 planes per image: three for the RGB planes
// (k4_resample.hip), one for the grey plane of JPGPU_CHANNELS_LUMA (k4y_resample_luma.hip).  The function per plane is the same: the
// description at the head of k4_resample.hip holds for both.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpgpu.h"
#include "common.h"
#include "kernels.h"

namespace jpgpu {

constexpr int kResizeTapGroup = 8;  // horizontal taps whose weights a lane fetches together
constexpr int kResizePieceVecs = kResizePieceBytes / 16 + 2;  // a piece begins up to 15 bytes behind a 16-byte boundary and ends as far in front of one

template <typename T>
__device__ __forceinline__ T resize_sample(float v, float scale, float bias);
template <>
__device__ __forceinline__ uint8_t resize_sample<uint8_t>(float v, float, float) {
    return (uint8_t)(int)fminf(fmaxf(__builtin_rintf(v), 0.0f), 255.0f);  // (v_rndne_f32: ties to even)
}
template <>
__device__ __forceinline__ float resize_sample<float>(float v, float scale, float bias) {
    return __fadd_rn(__fmul_rn(v, scale), bias);
}
template <>
__device__ __forceinline__ _Float16 resize_sample<_Float16>(float v, float scale, float bias) {
    return (_Float16)__fadd_rn(__fmul_rn(v, scale), bias);  // (round to nearest even: subnormals kept, overflow to infinity)
}

// One workgroup of 256: image blockIdx.x / bands, band blockIdx.x % bands of its output rows.  The image's NP planes lie w_in * h_in bytes
// apart from src_off; its slab in dst is NP planes of oh * ow samples from dst_off; plane p takes aff.scale[p] and aff.bias[p].
template <typename T, int NP>
__device__ __forceinline__ void resample_body(const uint8_t *__restrict__ src, const ResizeImage *__restrict__ images, const uint32_t *__restrict__ tables,
                                              T *__restrict__ dst, uint32_t ow, uint32_t oh, uint32_t bands, const OutputAffine &aff) {
    __shared__ uint4 stage[2][NP][kResizePieceVecs];
    const uint32_t tid = threadIdx.x;
    const ResizeImage im = images[blockIdx.x / bands];
    const uint32_t o0 = (blockIdx.x % bands) * (uint32_t)kResizeBandRows;
    const int32_t *__restrict__ hstart = reinterpret_cast<const int32_t *>(tables + im.h_off);
    const float *__restrict__ hw = reinterpret_cast<const float *>(tables + im.h_off + ow);
    const int32_t *__restrict__ vstart = reinterpret_cast<const int32_t *>(tables + im.v_off);
    const float *__restrict__ vw = reinterpret_cast<const float *>(tables + im.v_off + oh);
    const int32_t kx = (int32_t)im.h_taps, ky = (int32_t)im.v_taps;
    const uint64_t plane_bytes = (uint64_t)im.w_in * im.h_in;

    // the band's output rows and the input rows their taps hold (a row beyond oh repeats the last one's sums and is not stored)
    int32_t vs[kResizeBandRows];
#pragma unroll
    for (int r = 0; r < kResizeBandRows; r++) vs[r] = vstart[min(o0 + (uint32_t)r, oh - 1u)];
    const uint32_t r_last = min(o0 + (uint32_t)kResizeBandRows, oh) - 1u;
    const int32_t y_begin = vs[0], y_end = vstart[r_last] + ky;

    uint32_t buf = 0;
    for (uint32_t c0 = 0; c0 < ow; c0 += 256u) {
        const uint32_t o = c0 + tid;
        const bool active = o < ow;
        const int32_t my_start = active ? hstart[o] : 0;
        const int32_t x_begin = hstart[c0], x_end = hstart[min(c0 + 255u, ow - 1u)] + kx;  // (the starts never decrease with o)
        float acc[kResizeBandRows][NP];
#pragma unroll
        for (int r = 0; r < kResizeBandRows; r++)
#pragma unroll
            for (int p = 0; p < NP; p++) acc[r][p] = 0.0f;

        // weights k0 .. k0 + 7 of this lane's column, +0.0 from `end` on (no load reaches behind the table's taps)
        auto load_weights = [&](float (&w)[kResizeTapGroup], int32_t k0, int32_t end) {
#pragma unroll
            for (int j = 0; j < kResizeTapGroup; j++) {
                w[j] = 0.0f;
                if (k0 + j < end) w[j] = hw[(uint32_t)(k0 + j) * ow + o];
            }
        };
        for (int32_t y = y_begin; y < y_end; y++) {
            float h[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) h[p] = 0.0f;
            for (int32_t px0 = x_begin; px0 < x_end; px0 += kResizePieceBytes) {
                const int32_t plen = min((int32_t)kResizePieceBytes, x_end - px0);
                const int32_t rel = my_start - px0;
                const int32_t kb = active ? max(0, -rel) : 0, ke = active ? min(kx, plen - rel) : 0;
                float wa[kResizeTapGroup];
                load_weights(wa, kb, ke);  // (in front of the row's own loads: both are in flight together)
                uint32_t shift[NP];
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    // bytes [g, g + plen) of the output buffer, fetched as the whole 16-byte pieces that hold them (the buffer's base is
                    // 256-byte aligned and 256 bytes of slack lie behind its last image)
                    const uint64_t g = im.src_off + (uint64_t)p * plane_bytes + (uint64_t)y * im.w_in + (uint64_t)px0;
                    shift[p] = (uint32_t)g & 15u;
                    const uint4 *__restrict__ from = reinterpret_cast<const uint4 *>(src + (g - shift[p]));
                    const uint32_t n16 = (shift[p] + (uint32_t)plen + 15u) >> 4;  // <= kResizePieceVecs - 1
                    for (uint32_t i = tid; i < n16; i += 256u) stage[buf][p][i] = from[i];
                }
                __syncthreads();
                // (the next piece goes to the other buffer: every lane has passed this barrier, so none still reads that one)
                const uint8_t *b[NP];
#pragma unroll
                for (int p = 0; p < NP; p++) b[p] = reinterpret_cast<const uint8_t *>(stage[buf][p]) + shift[p] + rel;
                // Eight taps at a time, in ascending k, while the next eight weights are in flight.  A tap at or behind ke has the weight +0.0
                // and reads a staged byte up to seven places behind the piece's (inside the buffer's slack): finite whatever it is, so the term is +0.
                for (int32_t k0 = kb; k0 < ke; k0 += kResizeTapGroup) {
                    float wn[kResizeTapGroup];
                    load_weights(wn, k0 + kResizeTapGroup, ke);
                    // the group's eight bytes of each plane in one LDS read (any alignment): a lane's taps are neighbours, while the lanes of a
                    // wave lie `scale` bytes apart and share banks -- byte reads made that conflict eight times as often
                    uint32_t q[NP][2];
#pragma unroll
                    for (int p = 0; p < NP; p++) __builtin_memcpy(q[p], b[p] + k0, 8);
#pragma unroll
                    for (int j = 0; j < kResizeTapGroup; j++) {
                        const int sh = 8 * (j & 3);
#pragma unroll
                        for (int p = 0; p < NP; p++) h[p] = __fadd_rn(h[p], __fmul_rn(wa[j], (float)((q[p][j >> 2] >> sh) & 0xFFu)));
                    }
#pragma unroll
                    for (int j = 0; j < kResizeTapGroup; j++) wa[j] = wn[j];
                }
                buf ^= 1u;
            }
#pragma unroll
            for (int r = 0; r < kResizeBandRows; r++) {
                const int32_t k = y - vs[r];
                if (k >= 0 && k < ky) {  // (uniform: a scalar branch)
                    const float wv = vw[(uint32_t)k * oh + min(o0 + (uint32_t)r, oh - 1u)];
#pragma unroll
                    for (int p = 0; p < NP; p++) acc[r][p] = __fadd_rn(acc[r][p], __fmul_rn(wv, h[p]));
                }
            }
        }
        if (active) {
            // (one pointer per plane, stepped row by row: twenty-four addresses of their own would not fit the scalar registers)
            const uint64_t plane_out = (uint64_t)oh * ow;
            T *q[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) q[p] = dst + im.dst_off + (uint64_t)p * plane_out + (uint64_t)o0 * ow + o;
#pragma unroll
            for (int r = 0; r < kResizeBandRows; r++) {
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    if (o0 + (uint32_t)r < oh) *q[p] = resize_sample<T>(acc[r][p], aff.scale[p], aff.bias[p]);
                    q[p] += ow;
                }
            }
        }
    }
}

}  // namespace jpgpu
