// jpeglibrary_amd/csrc/k4y_resample_luma.hip -- K4 on one plane: the ragged grey planes K3Y has written under JPGPU_CHANNELS_LUMA, resampled
// to one size in one launch: T[N][1][oh][ow], uint8, float16 or float32 (jpgpu_batch_set_resize over a LUMA upload).  The tap tables and the
// function per plane are K4's (k4_resample.hip, k4_resample_body.h); the constants are scale[0] and bias[0].
// (A file of its own so that every other kernel object stays what it was.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k4_resample_body.h"

namespace jpgpu {

template <typename T>
__global__ __launch_bounds__(256) void resample_luma_kernel(const uint8_t *__restrict__ src, const ResizeImage *__restrict__ images,
                                                            const uint32_t *__restrict__ tables, T *__restrict__ dst, uint32_t ow, uint32_t oh,
                                                            uint32_t bands, OutputAffine aff) {
    resample_body<T, 1>(src, images, tables, dst, ow, oh, bands, aff);
}

hipError_t launch_resample_luma(hipStream_t stream, const uint8_t *src, const ResizeImage *images, int n_images, const uint32_t *tables, void *dst,
                                int out_width, int out_height, int sample_format, const OutputAffine &aff) {
    if (n_images <= 0) return hipSuccess;
    const uint32_t ow = (uint32_t)out_width, oh = (uint32_t)out_height;
    const uint32_t bands = (oh + (uint32_t)kResizeBandRows - 1u) / (uint32_t)kResizeBandRows;
    const uint64_t groups = (uint64_t)n_images * bands;
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)groups), block(256);
    if (sample_format == kFmtRgbPlanarU8)
        hipLaunchKernelGGL(resample_luma_kernel<uint8_t>, grid, block, 0, stream, src, images, tables, reinterpret_cast<uint8_t *>(dst), ow, oh, bands, aff);
    else if (sample_format == kFmtRgbPlanarF16)
        hipLaunchKernelGGL(resample_luma_kernel<_Float16>, grid, block, 0, stream, src, images, tables, reinterpret_cast<_Float16 *>(dst), ow, oh, bands, aff);
    else if (sample_format == kFmtRgbPlanarF32)
        hipLaunchKernelGGL(resample_luma_kernel<float>, grid, block, 0, stream, src, images, tables, reinterpret_cast<float *>(dst), ow, oh, bands, aff);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace jpgpu
