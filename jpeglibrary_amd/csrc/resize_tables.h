// jpeglibrary_amd/csrc/resize_tables.h -- the tap tables of the resize stage (K4, k4_resample.hip), built on the host in double.
//
// Separable antialiased bilinear resampling (a triangle filter, widened by the scale when shrinking).  For an axis of input length I
// and output length O, all in IEEE double:
//     scale = I / O;  sup = max(scale, 1.0)
//     for o in 0 .. O-1:
//         c  = (o + 0.5) * scale
//         lo = max(0, (int)(c - sup + 0.5));  hi = min(I, (int)(c + sup + 0.5))         ((int): truncation toward zero)
//         w64[k] = max(0.0, 1.0 - fabs((k + lo - c + 0.5) / sup))   for k in 0 .. hi-lo-1
//         w[k]   = (float)(w64[k] / sum(w64))                        (the sum in ascending k)
// Host code only: no HIP type appears here, so a stand-alone program can include it.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace jpgpu {

// The table as the definition states it: output o takes the taps [lo[o], lo[o] + count[o]) with the weights w[first[o] ...].
struct ResizeAxis {
    int in_len = 0, out_len = 0;
    int max_taps = 0;
    std::vector<int32_t> lo, count;
    std::vector<uint32_t> first;
    std::vector<float> w;
};

inline ResizeAxis resize_axis(int in_len, int out_len) {
    ResizeAxis t;
    t.in_len = in_len;
    t.out_len = out_len;
    if (in_len <= 0 || out_len <= 0) return t;
    const double scale = (double)in_len / (double)out_len;
    const double sup = std::max(scale, 1.0);
    t.lo.resize((size_t)out_len);
    t.count.resize((size_t)out_len);
    t.first.resize((size_t)out_len);
    std::vector<double> w64;
    for (int o = 0; o < out_len; o++) {
        const double c = ((double)o + 0.5) * scale;
        const int lo = std::max(0, (int)(c - sup + 0.5));
        const int hi = std::min(in_len, (int)(c + sup + 0.5));
        const int n = hi - lo;
        w64.assign((size_t)n, 0.0);
        double sum = 0.0;
        for (int k = 0; k < n; k++) {
            w64[(size_t)k] = std::max(0.0, 1.0 - fabs(((double)(k + lo) - c + 0.5) / sup));
            sum += w64[(size_t)k];
        }
        t.lo[(size_t)o] = lo;
        t.count[(size_t)o] = n;
        t.first[(size_t)o] = (uint32_t)t.w.size();
        for (int k = 0; k < n; k++) t.w.push_back((float)(w64[(size_t)k] / sum));
        t.max_taps = std::max(t.max_taps, n);
    }
    return t;
}

// The form K4 reads: every output takes exactly K = max_taps taps from start[o] = min(lo[o], I - K) on, so that no tap leaves the axis;
// the taps the definition does not name carry the weight +0.0, which changes no bit of a sum whose terms are all >= +0.  The weights lie
// tap-major, w[k * O + o], so that the lanes of a wave, one output each, read neighbouring words.
// Appended to `words` (floats as their bit patterns): O starts, then K * O weights.  -> the offset of the starts.
inline uint32_t resize_axis_pack(const ResizeAxis &t, std::vector<uint32_t> &words) {
    const uint32_t base = (uint32_t)words.size();
    const int O = t.out_len, K = t.max_taps;
    words.resize((size_t)base + (size_t)O + (size_t)K * (size_t)O, 0u);
    for (int o = 0; o < O; o++) {
        const int start = std::min<int>(t.lo[(size_t)o], t.in_len - K);
        words[(size_t)base + (size_t)o] = (uint32_t)start;
        for (int k = 0; k < t.count[(size_t)o]; k++) {
            const float w = t.w[(size_t)t.first[(size_t)o] + (size_t)k];
            uint32_t bits;
            static_assert(sizeof bits == sizeof w, "float32");
            __builtin_memcpy(&bits, &w, sizeof bits);
            words[(size_t)base + (size_t)O + (size_t)(t.lo[(size_t)o] - start + k) * (size_t)O + (size_t)o] = bits;
        }
    }
    return base;
}

}  // namespace jpgpu
