// jpeglibrary_amd/csrc/k3c_color.hip -- K3C: the colour step of the files JPGPU_COLOR_FILE treats by what they declare (include/jpgpu.h, "Colour").
// Images of kind RGB, CMYK and YCCK take K3's generic class, which leaves their INTERLEAVED_U8 samples in the scratch image; this kernel turns
// those samples into the five RGB forms.  One launch per batch: blockIdx.y = image (its descriptor in HBM, like extend_u16_kernel), blockIdx.x
// strides over the image's groups of four pixels, one group per lane -- a 4-component group is one 16-byte load, a 3-component group three
// dwords.  GRAY and YCBCR images never come here: they keep K3's fused classes and ycc_to_rgb_kernel.
// (A file of its own so that every other kernel object stays byte for byte what it was.  YCCK is defined through the bytes RGB_U8 would hold;
// the byte gathers, the clamp and the affine step are K3's, k3_pixel.h; the kinds' arithmetic
// and the plane stores are shared with K3O, k3c_pixel.h.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "k3c_pixel.h"

namespace jpgpu {

namespace {

template <int FMT>
__global__ __launch_bounds__(256) void color_convert_kernel(const uint8_t *__restrict__ scratch, uint8_t *__restrict__ out,
                                                            const ColorImage *__restrict__ images, YccRgbFactors kf, OutputAffine aff) {
    const ColorImage g = images[blockIdx.y];
    const uint8_t *src = scratch + g.src_off;
    uint8_t *dst = out + g.dst_off;
    const uint32_t kind = g.kind;
    const bool four = kind != kColorRgb;  // bytes per pixel in the scratch image: 4 (CMYK, YCCK) or 3
    constexpr uint32_t kSampleBytes = (uint32_t)fmt_rgb_plane_sample_bytes(FMT);
    const uint64_t groups = g.pixels >> 2;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q <= groups; q += (uint64_t)gridDim.x * 256) {
        if (q == groups) {
            // the tail: byte by byte, by the one lane that gets here
            for (uint64_t i = q * 4; i < g.pixels; i++) {
                const uint8_t *s = src + i * (four ? 4u : 3u);
                const uint32_t px = color_pixel(kind, (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | (four ? (uint32_t)s[3] << 24 : 0u), kf);
                if constexpr (fmt_is_rgb_planes(FMT)) {
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        store_plane1<FMT>(dst + (uint64_t)c * g.pixels * kSampleBytes, i, (px >> (8 * c)) & 0xFFu, aff.scale[c], aff.bias[c]);
                } else {
                    uint8_t *d = dst + i * (FMT == kFmtRgbaU8 ? 4u : 3u);
                    d[0] = (uint8_t)px;
                    d[1] = (uint8_t)(px >> 8);
                    d[2] = (uint8_t)(px >> 16);
                    if constexpr (FMT == kFmtRgbaU8) d[3] = 255;
                }
            }
            break;
        }
        uint32_t s[4];
        if (four) {  // (the scratch slot starts on a multiple of 256: every group is 16-byte aligned)
            const uint4 v = *reinterpret_cast<const uint4 *>(src + q * 16);
            s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
        } else {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(src + q * 12);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            s[0] = w0;  // (color_pixel masks the fourth byte away)
            s[1] = pick4(w0, w1, JPGPU_SEL(3, 4, 5, 12));
            s[2] = pick4(w1, w2, JPGPU_SEL(2, 3, 4, 12));
            s[3] = w2 >> 8;
        }
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; j++) px[j] = color_pixel(kind, s[j], kf);
        if constexpr (fmt_is_rgb_planes(FMT)) {
            const uint32_t lo_rg = pick4(px[0], px[1], JPGPU_SEL(0, 4, 1, 5)), hi_rg = pick4(px[2], px[3], JPGPU_SEL(0, 4, 1, 5));
            const uint32_t r = pick4(lo_rg, hi_rg, JPGPU_SEL(0, 1, 4, 5)), gr = pick4(lo_rg, hi_rg, JPGPU_SEL(2, 3, 6, 7));
            const uint32_t b = pick4(pick4(px[0], px[1], JPGPU_SEL(2, 6, 12, 12)), pick4(px[2], px[3], JPGPU_SEL(2, 6, 12, 12)), JPGPU_SEL(0, 1, 4, 5));
            const uint64_t plane = g.pixels * kSampleBytes, at = q * 4 * kSampleBytes;
            store_plane4<FMT>(dst + at, r, aff.scale[0], aff.bias[0]);
            store_plane4<FMT>(dst + plane + at, gr, aff.scale[1], aff.bias[1]);
            store_plane4<FMT>(dst + 2 * plane + at, b, aff.scale[2], aff.bias[2]);
        } else if constexpr (FMT == kFmtRgbaU8) {
            *reinterpret_cast<uint4 *>(dst + q * 16) = uint4{px[0] | 0xFF000000u, px[1] | 0xFF000000u, px[2] | 0xFF000000u, px[3] | 0xFF000000u};
        } else {  // four pixels -> three dwords
            uint32_t *d = reinterpret_cast<uint32_t *>(dst + q * 12);
            d[0] = pick4(px[0], px[1], JPGPU_SEL(0, 1, 2, 4));
            d[1] = pick4(px[1], px[2], JPGPU_SEL(1, 2, 4, 5));
            d[2] = pick4(px[2], px[3], JPGPU_SEL(2, 4, 5, 6));
        }
    }
}

}  // namespace

hipError_t launch_color_convert(hipStream_t stream, const uint8_t *scratch, uint8_t *out, const ColorImage *images, int n_images, uint64_t max_pixels,
                                int format, const YccRgbFactors &kf, const OutputAffine &aff) {
    if (n_images <= 0) return hipSuccess;
    if (!fmt_is_rgb(format)) return hipErrorInvalidValue;
    const uint32_t bx = (uint32_t)std::min<uint64_t>((max_pixels / 4 + 1 + 255) / 256, 4096);
    for (int base = 0; base < n_images; base += 65535) {  // grid.y limit
        const dim3 grid(bx, (uint32_t)std::min(n_images - base, 65535));
        switch (format) {
        case kFmtRgbU8: hipLaunchKernelGGL(color_convert_kernel<kFmtRgbU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbaU8: hipLaunchKernelGGL(color_convert_kernel<kFmtRgbaU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbPlanarU8: hipLaunchKernelGGL(color_convert_kernel<kFmtRgbPlanarU8>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        case kFmtRgbPlanarF16: hipLaunchKernelGGL(color_convert_kernel<kFmtRgbPlanarF16>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        default: hipLaunchKernelGGL(color_convert_kernel<kFmtRgbPlanarF32>, grid, dim3(256), 0, stream, scratch, out, images + base, kf, aff); break;
        }
    }
    return hipGetLastError();
}

}  // namespace jpgpu
