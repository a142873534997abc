// jpeglibrary_amd/csrc/k3u_taps.h -- the arithmetic of libjpeg's "fancy" (triangle) chroma upsampling as K3U (k3u_upsample.hip) applies it and
// as the planner (device_batch_layout.cpp) provides for it: which images are filtered, the taps and biases of an output pixel, and the
// rectangle of the stored frame K3 has to leave in the scratch image so that every tap is there.  Host + device: tests/test_upsample_cpu.py
// builds a stand-alone program over this header and compares its printout with tests/upsample_model.py.  (include/jpgpu.h, "Chroma
// upsampling", has the function in full.)
#pragma once
#include <stdint.h>

#ifndef JPGPU_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPGPU_HD __host__ __device__
#else
#define JPGPU_HD
#endif
#endif

namespace jpgpu {

// native chroma samples along an axis of `size` pixels subsampled by `step`: the REAL extent the taps clamp to (never the MCU padding)
JPGPU_HD inline uint32_t k3u_chroma_extent(uint32_t size, uint32_t step) { return (size + step - 1) / step; }

// The ratios that are filtered: h2v1, h2v2, h1v2 -- and, where hs == 2, only a chroma plane more than two samples wide (libjpeg takes its
// replicating routine for narrower ones).
JPGPU_HD inline bool k3u_ratio_filtered(uint32_t hs, uint32_t vs, uint32_t width) {
    const bool ratio = (hs == 2 && vs == 1) || (hs == 2 && vs == 2) || (hs == 1 && vs == 2);
    return ratio && (hs != 2 || k3u_chroma_extent(width, 2) > 2);
}

// Pixel coordinate p of an axis subsampled by two: the near native sample, the far one (clamped to [0, extent - 1]) and whether p is even.
struct K3uTap {
    uint32_t near, far;
    bool even;
};
JPGPU_HD inline K3uTap k3u_tap(uint32_t p, uint32_t extent) {
    K3uTap t;
    t.even = (p & 1u) == 0;
    t.near = p >> 1;
    t.far = t.even ? (t.near == 0 ? 0u : t.near - 1u) : (t.near + 1u < extent ? t.near + 1u : extent - 1u);
    return t;
}

// The biases and the shift.  Vertically filtered rows carry s = 3 * near + far unrounded; a pixel is
//   h2v1: (3 * C[near] + C[far] + k3u_bias_h2v1(x)) >> 2     h1v2: (s + k3u_bias_v(y)) >> 2     h2v2: (3 * s[near] + s[far] + k3u_bias_h2v2(x)) >> 4
JPGPU_HD inline uint32_t k3u_bias_h2v1(uint32_t x) { return (x & 1u) ? 2u : 1u; }
JPGPU_HD inline uint32_t k3u_bias_v(uint32_t y) { return (y & 1u) ? 2u : 1u; }
JPGPU_HD inline uint32_t k3u_bias_h2v2(uint32_t x) { return (x & 1u) ? 7u : 8u; }
// ... in one expression for the kernel, which holds Cb in the low and Cr in the high half of a dword (every sum stays below 2^16: 16 * 255 + 8)
JPGPU_HD inline uint32_t k3u_bias(uint32_t hs, uint32_t vs, uint32_t x, uint32_t y) {
    return hs == 2 ? (vs == 2 ? k3u_bias_h2v2(x) : k3u_bias_h2v1(x)) : k3u_bias_v(y);
}
JPGPU_HD inline uint32_t k3u_shift(uint32_t hs, uint32_t vs) { return hs == 2 && vs == 2 ? 4u : 2u; }

// One axis of the fetch rectangle: the pixels [p0, p1) of an axis of `size` pixels subsampled by `step`, widened to whole native samples
// plus one sample per side, clipped to the frame: [lo, hi).  step == 1: the pixels themselves.
struct K3uSpan {
    uint32_t lo, hi;
};
JPGPU_HD inline K3uSpan k3u_fetch_span(uint32_t p0, uint32_t p1, uint32_t size, uint32_t step) {
    K3uSpan s;
    if (step == 1) {
        s.lo = p0;
        s.hi = p1;
        return s;
    }
    const uint32_t first = p0 / step, behind = (p1 - 1) / step + 2;
    s.lo = first == 0 ? 0u : (first - 1) * step;
    s.hi = behind * step < size ? behind * step : size;
    return s;
}

// Native sample k of an axis lies at pixel k * step of the frame; the scratch image holds it only if that pixel is inside the span.  It
// always is for the taps of the pixels [p0, p1) the span was made for: tests/test_upsample_cpu.py enumerates it.
JPGPU_HD inline bool k3u_sample_in_span(uint32_t k, uint32_t step, const K3uSpan &s) { return k * step >= s.lo && k * step < s.hi; }

}  // namespace jpgpu
