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

// What a file declares about the way its pixels are to be turned for display: the Orientation tag (0x0112) in IFD0 of the FIRST APP1 "Exif\0\0"
// segment in front of the first SOS (HostDecoder records it on every Identify walk, next to the colour markers) -- the one decision
// JPGPU_ORIENT_FILE makes (include/jpgpu.h, "Orientation").  A block that is short, malformed or without the tag gives 1: it never fails an image.
struct ExifMarker {
    bool seen = false;        // the first such APP1 has been read; later ones are not
    uint8_t orientation = 1;  // 1..8
    size_t value_at = 0;      // a value that counts: its two bytes behind "Exif\0\0" ...
    bool little = false;      // ... and their byte order (the optimizer's lossless transform rewrites them)
};
// t: the n bytes behind "Exif\0\0" (the TIFF header onwards).  Every read is checked against n.  value_at / little (may be null): where the
// two bytes of a value that counts stand in t, and their byte order (the optimizer's lossless transform rewrites them).
inline int exif_orientation_of(const uint8_t *t, size_t n, size_t *value_at = nullptr, bool *little_endian = nullptr) {
    if (n < 8) return 1;
    const bool little = t[0] == 'I' && t[1] == 'I';
    if (!little && !(t[0] == 'M' && t[1] == 'M')) return 1;
    const auto u16 = [&](size_t at) { return little ? (uint32_t)t[at] | ((uint32_t)t[at + 1] << 8) : ((uint32_t)t[at] << 8) | (uint32_t)t[at + 1]; };
    const auto u32 = [&](size_t at) { return little ? u16(at) | (u16(at + 2) << 16) : (u16(at) << 16) | u16(at + 2); };
    if (u16(2) != 42) return 1;
    const size_t ifd = u32(4);
    if (ifd > n || n - ifd < 2) return 1;
    const uint32_t entries = u16(ifd);
    for (uint32_t k = 0; k < entries; k++) {
        const size_t e = ifd + 2 + (size_t)k * 12;
        if (e > n || n - e < 12) return 1;  // (an entry that leaves the segment)
        if (u16(e) != 0x0112) continue;
        if (u16(e + 2) != 3 || u32(e + 4) != 1) return 1;  // SHORT, count 1
        const uint32_t v = u16(e + 8);
        if (v < 1 || v > 8) return 1;
        if (value_at) *value_at = e + 8;
        if (little_endian) *little_endian = little;
        return (int)v;
    }
    return 1;
}
inline void note_exif_marker(ExifMarker &m, int marker, const uint8_t *payload, size_t len) {
    if (m.seen || marker != 0xE1 || len < 6 || memcmp(payload, "Exif\0\0", 6) != 0) return;
    m.seen = true;
    m.orientation = (uint8_t)exif_orientation_of(payload + 6, len - 6, &m.value_at, &m.little);
}
// Orientation o (1..8) over a stored frame of `width` x `height`: the size of the oriented frame, and the rectangle of the stored frame that
// holds the pixels of a rectangle given in the oriented one (include/jpgpu.h: the table's (y, x) over the rectangle's corners).
constexpr bool orientation_transposes(int o) { return o >= 5; }
constexpr bool orientation_flips_x(int o) { return o == 2 || o == 3 || o == 7 || o == 8; }  // the stored column runs against the output's
constexpr bool orientation_flips_y(int o) { return o == 3 || o == 4 || o == 6 || o == 7; }  // the stored row runs against the output's
inline jpgpu_rect orientation_stored_rect(int o, jpgpu_rect r, uint32_t width, uint32_t height) {
    jpgpu_rect s = orientation_transposes(o) ? jpgpu_rect{r.y, r.x, r.height, r.width} : r;
    if (orientation_flips_x(o)) s.x = width - s.x - s.width;
    if (orientation_flips_y(o)) s.y = height - s.y - s.height;
    return s;
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
