// jpeglibrary_amd/csrc/ingest_host.h -- what the ingest (device_batch_ingest.cpp) does without a device: a file as a list of
// segments, and the cut of the input buffer into the pieces the crew copies into the staging ring.  Nothing here includes HIP:
// tools/ingest_host_check.cpp runs both under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/jpgpu.h"

namespace jpgpu {

// What a file declares about its colour space, in the markers between SOI and the first SOS (HostDecoder records it on every Identify walk),
// and libjpeg's rule over it (jdapimin.c, default_decompress_parms) -- the one decision JPGPU_COLOR_FILE makes (include/jpgpu.h, "Colour").
struct ColorMarkers {
    bool saw_jfif = false;     // an APP0 of at least 14 payload bytes that begins "JFIF\0"
    int adobe_transform = -1;  // payload[11] of the last APP14 of at least 12 payload bytes that begins "Adobe"; -1: none
};
inline void note_color_marker(ColorMarkers &m, int marker, const uint8_t *payload, size_t len) {
    if (marker == 0xE0 && len >= 14 && memcmp(payload, "JFIF\0", 5) == 0) m.saw_jfif = true;
    if (marker == 0xEE && len >= 12 && memcmp(payload, "Adobe", 5) == 0) m.adobe_transform = payload[11];
}
// -> a jpgpu_color_kind, or -1 for what the RGB formats refuse as before: 2 or more than 4 components, a precision other than 8.
// ids: the frame's component identifiers (num_components of them).
inline int color_kind_of(int precision, int num_components, const uint8_t *ids, const ColorMarkers &m) {
    if (precision != 8) return -1;
    const bool adobe = m.adobe_transform >= 0;
    switch (num_components) {
    case 1: return JPGPU_COLOR_KIND_GRAY;
    case 3:
        if (m.saw_jfif) return JPGPU_COLOR_KIND_YCBCR;
        if (adobe) return m.adobe_transform == 0 ? JPGPU_COLOR_KIND_RGB : JPGPU_COLOR_KIND_YCBCR;
        return ids && ids[0] == 0x52 && ids[1] == 0x47 && ids[2] == 0x42 ? JPGPU_COLOR_KIND_RGB : JPGPU_COLOR_KIND_YCBCR;
    case 4: return adobe && m.adobe_transform != 0 ? JPGPU_COLOR_KIND_YCCK : JPGPU_COLOR_KIND_CMYK;  // (JFIF says nothing about four components)
    default: return -1;
    }
}

// One input file as the caller handed it over: a list of segments (one for jpgpu_batch_upload), and the contiguous bytes the
// host parser reads -- the file itself, or what was gathered of a multi-segment file (its head for the header-only plan, all
// of it for the full marker walks).
struct FileSegs {
    const jpgpu_segment *seg = nullptr;
    int n = 0;
    size_t len = 0;
    const uint8_t *base = nullptr;
    size_t base_len = 0;
    std::vector<uint8_t> gathered;
    // jpgpu_batch_upload_device: the file lies in the caller's device memory (no segments) and, once staged, at `slot` of the
    // input buffer; `base` is its head as the device delivered it, or the whole file fetched back from its slot; the host sees
    // nothing else of it but the two bytes at its ingest verdict (verdict_at: offset in the file)
    const uint8_t *dev = nullptr;
    bool device = false;
    uint64_t slot = 0;  // where the file lies in the input buffer, whatever its source (DeviceBatch::place_files)
    size_t verdict_at = 0;
    uint32_t verdict = 0;
    static constexpr size_t kHeadBytes = 64u << 10;
    bool whole() const { return base_len == len; }
    void gather(size_t want) {
        want = std::min(want, len);
        gathered.resize(want);
        size_t pos = 0;
        for (int k = 0; k < n && pos < want; k++) {
            const size_t m = std::min(seg[k].len, want - pos);
            if (m) memcpy(gathered.data() + pos, seg[k].data, m);
            pos += m;
        }
        base = gathered.data();
        base_len = want;
    }
    uint8_t at(size_t off) const {
        if (device) return off == verdict_at ? (uint8_t)verdict : off == verdict_at + 1 ? (uint8_t)(verdict >> 8) : 0;
        for (int k = 0; k < n; k++) {
            if (off < seg[k].len) return seg[k].data[off];
            off -= seg[k].len;
        }
        return 0;
    }
};

// A piece of the input buffer as the crew fills it into the staging ring.
struct StagePiece {
    const uint8_t *src;  // nullptr: zero fill (slack in front of the first file, behind the last, between files)
    uint64_t dst;
    uint32_t n;
};
constexpr uint32_t kStagePieceMax = 2u << 20;

// [dst, dst + n) of the input buffer, cut into pieces that never cross a slot of the ring and never exceed kStagePieceMax
inline void cut_stage_pieces(std::vector<StagePiece> &pieces, const uint8_t *src, uint64_t dst, uint64_t n, uint64_t slot_bytes) {
    while (n) {
        const uint64_t room = slot_bytes - dst % slot_bytes;
        const uint32_t m = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n, room), kStagePieceMax);
        pieces.push_back({src, dst, m});
        if (src) src += m;
        dst += m;
        n -= m;
    }
}

}  // namespace jpgpu
