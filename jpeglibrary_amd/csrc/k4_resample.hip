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

#include "k4_resample_body.h"

namespace jpgpu {

// (the kernel's body: k4_resample_body.h, shared with the one-plane form of k4y_resample_luma.hip)
template <typename T>
__global__ __launch_bounds__(256) void resample_kernel(const uint8_t *__restrict__ src, const ResizeImage *__restrict__ images,
                                                       const uint32_t *__restrict__ tables, T *__restrict__ dst, uint32_t ow, uint32_t oh,
                                                       uint32_t bands, OutputAffine aff) {
    resample_body<T, 3>(src, images, tables, dst, ow, oh, bands, aff);
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
