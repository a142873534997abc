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
