// jpeglibrary_amd/csrc/k4_resample.hip -- K4: the ragged RGB_PLANAR_U8 images K3 has written, resampled to one size in one launch:
// T[N][3][oh][ow], uint8, float16 or float32 (jpgpu_batch_set_resize).
//
// The result is a fixed function of the source bytes.  Separable antialiased bilinear resampling with the tap tables of resize_tables.h
// (built on the host in double, rounded once to float32): a horizontal pass over (float)byte, then a vertical pass over the horizontal
// pass's float32 results, each  acc = 0.0f; for k ascending: t = w[k] * x; acc = acc + t  with every multiply and every add rounded to
// float32 on its own (__fmul_rn / __fadd_rn, and -ffp-contract=off on the file).  v being the second pass's result, the sample is
// clamp(rint(v), 0, 255) as uint8 (ties to even), or (v * scale[c]) + bias[c] as float32, or that rounded to nearest even to binary16.
// Taps of weight +0.0 change no bit, because every term is >= +0: the tables pad every output to the axis's largest tap count with them.
//
// One 256-thread workgroup per (image, band of kResizeBandRows output rows); a lane owns one output column (chunks of 256 columns when
// ow > 256) of all three planes, so the weights are fetched once for three sums.  The band's input rows are walked in ascending y: the bytes
// of the row that the chunk's columns need are staged in LDS with 16-byte loads (in pieces of kResizePieceBytes per plane, double
// buffered: one barrier per piece), every lane forms the horizontal sums of its column from LDS, eight taps at a time with the
// next eight weights in flight, and adds wv * h into the accumulator of
// every output row of the band whose taps hold y -- the row index and the vertical weights are uniform, so those are scalar loads and
// the eight accumulators per plane are unrolled and predicated by scalar branches.  Rows arriving in ascending order give the vertical
// pass its ascending k; no intermediate image goes to memory, and an input row is read 1 + 2 / kResizeBandRows times at worst.
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

template <typename T>
__global__ __launch_bounds__(256) void resample_kernel(const uint8_t *__restrict__ src, const ResizeImage *__restrict__ images,
                                                       const uint32_t *__restrict__ tables, T *__restrict__ dst, uint32_t ow, uint32_t oh,
                                                       uint32_t bands, OutputAffine aff) {
    __shared__ uint4 stage[2][3][kResizePieceVecs];
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
        float acc[kResizeBandRows][3];
#pragma unroll
        for (int r = 0; r < kResizeBandRows; r++) acc[r][0] = acc[r][1] = acc[r][2] = 0.0f;

        // weights k0 .. k0 + 7 of this lane's column, +0.0 from `end` on (no load reaches behind the table's taps)
        auto load_weights = [&](float (&w)[kResizeTapGroup], int32_t k0, int32_t end) {
#pragma unroll
            for (int j = 0; j < kResizeTapGroup; j++) {
                w[j] = 0.0f;
                if (k0 + j < end) w[j] = hw[(uint32_t)(k0 + j) * ow + o];
            }
        };
        for (int32_t y = y_begin; y < y_end; y++) {
            float h[3] = {0.0f, 0.0f, 0.0f};
            for (int32_t px0 = x_begin; px0 < x_end; px0 += kResizePieceBytes) {
                const int32_t plen = min((int32_t)kResizePieceBytes, x_end - px0);
                const int32_t rel = my_start - px0;
                const int32_t kb = active ? max(0, -rel) : 0, ke = active ? min(kx, plen - rel) : 0;
                float wa[kResizeTapGroup];
                load_weights(wa, kb, ke);  // (in front of the row's own loads: both are in flight together)
                uint32_t shift[3];
#pragma unroll
                for (int p = 0; p < 3; p++) {
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
                const uint8_t *b0 = reinterpret_cast<const uint8_t *>(stage[buf][0]) + shift[0] + rel;
                const uint8_t *b1 = reinterpret_cast<const uint8_t *>(stage[buf][1]) + shift[1] + rel;
                const uint8_t *b2 = reinterpret_cast<const uint8_t *>(stage[buf][2]) + shift[2] + rel;
                // Eight taps at a time, in ascending k, while the next eight weights are in flight.  A tap at or behind ke has the weight +0.0
                // and reads a staged byte up to seven places behind the piece's (inside the buffer's slack): finite whatever it is, so the term is +0.
                for (int32_t k0 = kb; k0 < ke; k0 += kResizeTapGroup) {
                    float wn[kResizeTapGroup];
                    load_weights(wn, k0 + kResizeTapGroup, ke);
                    // the group's eight bytes of each plane in one LDS read (any alignment): a lane's taps are neighbours, while the lanes of a
                    // wave lie `scale` bytes apart and share banks -- byte reads made that conflict eight times as often
                    uint32_t q0[2], q1[2], q2[2];
                    __builtin_memcpy(q0, b0 + k0, 8);
                    __builtin_memcpy(q1, b1 + k0, 8);
                    __builtin_memcpy(q2, b2 + k0, 8);
#pragma unroll
                    for (int j = 0; j < kResizeTapGroup; j++) {
                        const int sh = 8 * (j & 3);
                        h[0] = __fadd_rn(h[0], __fmul_rn(wa[j], (float)((q0[j >> 2] >> sh) & 0xFFu)));
                        h[1] = __fadd_rn(h[1], __fmul_rn(wa[j], (float)((q1[j >> 2] >> sh) & 0xFFu)));
                        h[2] = __fadd_rn(h[2], __fmul_rn(wa[j], (float)((q2[j >> 2] >> sh) & 0xFFu)));
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
                    acc[r][0] = __fadd_rn(acc[r][0], __fmul_rn(wv, h[0]));
                    acc[r][1] = __fadd_rn(acc[r][1], __fmul_rn(wv, h[1]));
                    acc[r][2] = __fadd_rn(acc[r][2], __fmul_rn(wv, h[2]));
                }
            }
        }
        if (active) {
            // (one pointer per plane, stepped row by row: twenty-four addresses of their own would not fit the scalar registers)
            const uint64_t plane_out = (uint64_t)oh * ow;
            T *q0 = dst + im.dst_off + (uint64_t)o0 * ow + o, *q1 = q0 + plane_out, *q2 = q1 + plane_out;
#pragma unroll
            for (int r = 0; r < kResizeBandRows; r++) {
                if (o0 + (uint32_t)r < oh) {
                    *q0 = resize_sample<T>(acc[r][0], aff.scale[0], aff.bias[0]);
                    *q1 = resize_sample<T>(acc[r][1], aff.scale[1], aff.bias[1]);
                    *q2 = resize_sample<T>(acc[r][2], aff.scale[2], aff.bias[2]);
                }
                q0 += ow;
                q1 += ow;
                q2 += ow;
            }
        }
    }
}

hipError_t launch_resample(hipStream_t stream, const uint8_t *src, const ResizeImage *images, int n_images, const uint32_t *tables, void *dst,
                           int out_width, int out_height, int sample_format, const OutputAffine &aff) {
    if (n_images <= 0) return hipSuccess;
    const uint32_t ow = (uint32_t)out_width, oh = (uint32_t)out_height;
    const uint32_t bands = (oh + (uint32_t)kResizeBandRows - 1u) / (uint32_t)kResizeBandRows;
    const uint64_t groups = (uint64_t)n_images * bands;
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)groups), block(256);
    if (sample_format == kFmtRgbPlanarU8)
        hipLaunchKernelGGL(resample_kernel<uint8_t>, grid, block, 0, stream, src, images, tables, reinterpret_cast<uint8_t *>(dst), ow, oh, bands, aff);
    else if (sample_format == kFmtRgbPlanarF16)
        hipLaunchKernelGGL(resample_kernel<_Float16>, grid, block, 0, stream, src, images, tables, reinterpret_cast<_Float16 *>(dst), ow, oh, bands, aff);
    else if (sample_format == kFmtRgbPlanarF32)
        hipLaunchKernelGGL(resample_kernel<float>, grid, block, 0, stream, src, images, tables, reinterpret_cast<float *>(dst), ow, oh, bands, aff);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace jpgpu
