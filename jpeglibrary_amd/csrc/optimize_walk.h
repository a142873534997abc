// jpeglibrary_amd/csrc/optimize_walk.h -- the host side of JpegOptimizer: Scan()'s and Optimize(strip)'s marker walks (ref:
// JpegOptimizer.cs:66-153, :540-648) over one file -> the pieces of its output, or its refusal.  No device, no HIP: OptimizeBatch::upload
// and the stand-alone sanitizer harness (tools/fuzz/optimizer_walk_asan.cpp, linked with host_parser.cpp for the marker reader and the
// header parsers) share it.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/jpgpu.h"
#include "common.h"
#include "host.h"

namespace jpgpu {

// JpegWriter.WriteMarker (ref: JpegWriter.cs:289-303) and WriteLength (:309-321: the length counts its own two bytes), for the
// encoder's byte vectors and the optimizer's strings alike
template <typename Bytes>
void put_marker(Bytes &o, int m) {
    o.push_back((typename Bytes::value_type)0xFF);
    o.push_back((typename Bytes::value_type)m);
}
template <typename Bytes>
void put_length(Bytes &o, uint16_t length) {
    const uint16_t v = (uint16_t)(length + 2);
    o.push_back((typename Bytes::value_type)(v >> 8));
    o.push_back((typename Bytes::value_type)v);
}

struct Verdict {
    int status = JPGPU_OK, detail = 0;
    std::string error;
};
using Refuse = Verdict;  // ... as the walks throw it
[[noreturn]] inline void refuse(int status, const std::string &msg, int detail = 0) { throw Refuse{status, detail, msg}; }
inline std::string at_offset(int off, const char *msg) { return "Failed to decode JPEG data at offset " + std::to_string(off) + ". " + msg; }

// Optimize()'s output is a fixed sequence of pieces: bytes known on the host, the new DHT segment, the scan's data
struct Piece {
    enum Kind { kBytes, kHuffmanTables, kEntropy } kind;
    std::string bytes;
};

// what the walks leave of one file: its verdict, and
struct WalkPlan : Verdict {
    // failures of the marker walks BEHIND the scan: the reference meets them only once the scan itself went through
    // (Scan() throws from ProcessScanBaseline first), so they are reported after the device-side status
    Verdict late;
    // ... and what the walks end in instead when the scan leaves exactly one whole byte unread: the reference's reader
    // then resumes one byte INTO the terminating marker (DeviceBatch::plan_swallowed_terminator has the mechanism)
    Verdict swallow;
    int dri_at_scan = 0;
    size_t rsts_in_scan = 0;  // RSTn markers between the scan header and the scan's terminating marker
    std::vector<Piece> pieces;
    void refused(const Refuse &e) {
        static_cast<Verdict &>(*this) = e;
        pieces.clear();
    }
};

// find_scan_end of the scan the walks of one file keep coming back to (four walks, one search); it lives as long as the file's bytes do
struct ScanEndCache {
    const uint8_t *key = nullptr;
    size_t len = 0, val = 0;
    std::string rsts;
    size_t scan_end(const uint8_t *entropy, size_t n) {
        if (entropy != key || n != len) {
            key = entropy;
            len = n;
            rsts.clear();
            val = find_scan_end(entropy, n, &rsts);
        }
        return val;
    }
};

// a segment's length, then its bytes (skipped when `buf` is null: `content` is then what the reference says of a short one)
inline uint16_t read_segment(MarkerReader &r, const uint8_t **buf, const char *content = "Unexpected end of input data when reading segment content.") {
    uint16_t length;
    if (!r.try_read_length(&length))
        refuse(JPGPU_ERR_INVALID_DATA, at_offset(r.consumed_byte_count(), "Unexpected end of input data when reading segment length."));
    if (!(buf ? r.try_read_bytes(length, buf) : r.try_advance(length))) refuse(JPGPU_ERR_INVALID_DATA, at_offset(r.consumed_byte_count(), content));
    return length;
}
[[noreturn]] inline void refuse_frame_type(const MarkerReader &r, int marker, int detail) {
    refuse(JPGPU_ERR_INVALID_DATA,
           at_offset(r.consumed_byte_count(), ("This type of JPEG stream is not supported (StartOfFrame" + std::to_string(marker - 0xC0) + ").").c_str()), detail);
}
inline void parse_frame_header(const MarkerReader &r, const uint8_t *buf, uint16_t length, FrameHeader *fh) {
    int consumed = 0;
    if (!FrameHeader::try_parse(buf, length, false, fh, &consumed))
        refuse(JPGPU_ERR_INVALID_DATA, at_offset(r.consumed_byte_count() - length + consumed, "Failed to parse frame header."));
}

// what Scan() hands Optimize(): tables, frame, restart interval as of the scan
struct ScanWalk {
    std::vector<QuantTable> quant;  // _quantizationTables: replace by identifier, else append (:319-338)
    FrameHeader frame;
    uint16_t dri_at_scan = 0;
    bool after_scan = false;  // from here on a failure of the walks is only met once the scan itself went through
};

// ---- Scan(): exactly one scan
inline void walk_scan(WalkPlan &p, ScanWalk &w, ScanEndCache &ends, const uint8_t *data, size_t len, bool swallow_terminator) {
    bool have_frame = false;
    int n_scans = 0;
    uint16_t dri = 0;
    if (len == 0) refuse(JPGPU_ERR_INVALID_OPERATION, "Input buffer is not specified.");
    MarkerReader r(data, len);
    bool eoi = false;
    while (!eoi && !r.is_empty()) {
        int marker;
        if (!r.try_read_marker(&marker)) refuse(JPGPU_ERR_INVALID_DATA, at_offset(r.consumed_byte_count(), "No marker found."));
        uint16_t length;
        const uint8_t *buf;
        switch (marker) {
        case 0xD8: break;
        case 0xC0:
        case 0xC1: {
            length = read_segment(r, &buf);
            FrameHeader fh;
            parse_frame_header(r, buf, length, &fh);
            if (have_frame) refuse(JPGPU_ERR_INVALID_DATA, at_offset(r.consumed_byte_count(), "Multiple frame is not supported."));
            have_frame = true;
            w.frame = fh;
            break;
        }
        // StartOfFrame2 is not among Scan()'s cases (:95-146): a progressive frame header is skipped like an APPn segment and
        // the first SOS then finds no frame header (the null reference below)
        case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
            refuse_frame_type(r, marker, kDetailUnsupportedFrame);
        case 0xC4: {
            // The decoding tables themselves are the decoder-side parser's business, but a table that does not parse ends Scan()
            // HERE (JpegOptimizer.cs ProcessDefineHuffmanTable), in front of whatever a later marker would have thrown -- e.g. the
            // missing frame header at SOS when a bit flip made the SOF marker a DHT
            // (tests/golden/stress/optimizer_dht_in_place_of_sof_*.jpg)
            length = read_segment(r, &buf);
            int off = r.consumed_byte_count() - length;
            for (size_t rem = length; rem != 0;) {
                HuffTable t;
                int consumed = 0;
                if (!HuffTable::try_parse(buf, rem, &t, &consumed)) refuse(JPGPU_ERR_INVALID_DATA, at_offset(off, "Failed to parse Huffman table."));
                buf += consumed;
                rem -= (size_t)consumed;
                off += consumed;
            }
            break;
        }
        case 0xDB: {
            length = read_segment(r, &buf);
            const int base = r.consumed_byte_count() - length;
            int off = 0;
            while (off < (int)length) {
                QuantTable t;
                int consumed = 0;
                if (!QuantTable::try_parse(buf + off, (size_t)length - off, &t, &consumed))
                    refuse(JPGPU_ERR_INVALID_DATA, at_offset(base + off, "Failed to parse quantization table."));
                off += consumed;
                bool replaced = false;
                for (QuantTable &q : w.quant)
                    if (q.identifier == t.identifier) {
                        q = t;
                        replaced = true;
                    }
                if (!replaced) w.quant.push_back(t);
            }
            break;
        }
        case 0xDD:
            length = read_segment(r, &buf);
            if (length < 2)
                refuse(JPGPU_ERR_INVALID_DATA, at_offset(r.consumed_byte_count(), "Unexpected end of input data when reading segment content."));
            dri = (uint16_t)(buf[0] << 8 | buf[1]);
            break;
        case 0xDA: {
            read_segment(r, &buf);
            if (!have_frame) refuse(JPGPU_ERR_INVALID_OPERATION, "Object reference not set to an instance of an object.");
            if (++n_scans > 1)
                refuse(JPGPU_ERR_NOT_SUPPORTED, "Files with more than one scan are not supported by the optimizer path.", kDetailUnsupportedFrame);
            w.dri_at_scan = dri;
            p.dri_at_scan = dri;
            w.after_scan = true;
            const size_t end = ends.scan_end(r.remaining_bytes(), (size_t)r.remaining_byte_count());
            r.try_advance((int)end + (swallow_terminator && end < (size_t)r.remaining_byte_count() ? 1 : 0));
            break;
        }
        case 0xD0: case 0xD1: case 0xD2: case 0xD3: case 0xD4: case 0xD5: case 0xD6: case 0xD7: break;
        case 0xD9: eoi = true; break;
        default: read_segment(r, nullptr, "Unexpected end of input data reached."); break;
        }
    }
    if (n_scans == 0) refuse(JPGPU_ERR_INVALID_DATA, at_offset(r.consumed_byte_count(), "No image data is read."));
    if (w.dri_at_scan != dri)
        refuse(JPGPU_ERR_NOT_SUPPORTED, "A restart interval that changes after the scan is not supported by the optimizer path.", kDetailUnsupportedFrame);
}

// ---- Optimize(strip): the pieces of the output into p.pieces.  turned: the file is F' (the source with its SOF / DQT / Exif patches),
// whose scan holds exactly the restart markers it needs
inline void walk_optimize(WalkPlan &p, const ScanWalk &w, ScanEndCache &ends, const uint8_t *data, size_t len, bool strip, bool swallow_terminator,
                          bool turned) {
    MarkerReader r(data, len);
    std::string cur;
    auto flush = [&]() {
        if (!cur.empty()) p.pieces.push_back({Piece::kBytes, cur});
        cur.clear();
    };
    auto copy_segment = [&](int marker) {  // the marker, then CopyMarkerData (:661-675)
        put_marker(cur, marker);
        const uint8_t *buf;
        const uint16_t length = read_segment(r, &buf);
        put_length(cur, length);
        cur.append((const char *)buf, length);
    };
    bool eoi = false, dht_written = false, dqt_written = false;
    while (!eoi && !r.is_empty()) {
        int marker;
        if (!r.try_read_marker(&marker)) refuse(JPGPU_ERR_INVALID_DATA, at_offset(r.consumed_byte_count(), "No marker found."));
        switch (marker) {
        case 0xD8: put_marker(cur, marker); break;
        case 0xE0:
        case 0xC0:
        case 0xC1: copy_segment(marker); break;
        case 0xC2: {  // ProcessFrameHeader, then "not supported" (:580-582).  Reached on baseline files too: the walk does not
                      // skip the DQT / DHT payloads, and a quantisation table may hold the bytes FF C2 (low qualities)
            const uint8_t *buf;
            const uint16_t length = read_segment(r, &buf);
            FrameHeader fh;
            parse_frame_header(r, buf, length, &fh);
            refuse(JPGPU_ERR_INVALID_DATA, "Progressive JPEG is not supported currently.");
        }
        case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
            refuse_frame_type(r, marker, 0);
        case 0xC4:  // the segment's own bytes are not skipped: the marker search runs through them (:596-602)
            if (!dht_written) {
                flush();
                p.pieces.push_back({Piece::kHuffmanTables, std::string()});
                dht_written = true;
            }
            break;
        case 0xDB:
            if (!dqt_written) {
                put_marker(cur, 0xDB);
                uint16_t total = 0;
                for (const QuantTable &q : w.quant) total = (uint16_t)(total + (uint8_t)(q.precision == 0 ? 65 : 129));
                put_length(cur, total);
                for (const QuantTable &q : w.quant) {
                    cur.push_back((char)(q.precision << 4 | (q.identifier & 0xF)));
                    for (int k = 0; k < 64; k++) {
                        if (q.precision != 0) cur.push_back((char)(q.elements[k] >> 8));
                        cur.push_back((char)q.elements[k]);
                    }
                }
                dqt_written = true;
            }
            break;
        case 0xDA: {
            copy_segment(marker);
            flush();
            p.pieces.push_back({Piece::kEntropy, std::string()});
            const size_t end = ends.scan_end(r.remaining_bytes(), (size_t)r.remaining_byte_count());
            // More RSTn markers than the frame's intervals need: the scan stops behind its last MCU and the walk meets
            // the others as markers of their own, copied one by one (:603-612).  The first of them depends on where
            // the bit reader stood (transcode_kernel decides it), the rest are certain.
            int max_h = 1, max_v = 1;
            for (const FrameComponent &c : w.frame.components) {
                max_h = std::max(max_h, (int)c.h);
                max_v = std::max(max_v, (int)c.v);
            }
            const uint64_t mcus = (uint64_t)((w.frame.samples_per_line + 8 * max_h - 1) / (8 * max_h)) * ((w.frame.lines + 8 * max_v - 1) / (8 * max_v));
            const uint64_t intervals = w.dri_at_scan ? (mcus + w.dri_at_scan - 1) / w.dri_at_scan : 1;
            p.rsts_in_scan = ends.rsts.size();
            // (a turned image: `data` is F' with the SOURCE's scan still behind its header; the scan of F' itself is written
            // from the turned blocks and holds exactly the markers its intervals need)
            for (size_t k = (size_t)intervals; !turned && k < ends.rsts.size(); k++) put_marker(cur, (uint8_t)ends.rsts[k]);
            r.try_advance((int)end + (swallow_terminator && end < (size_t)r.remaining_byte_count() ? 1 : 0));
            break;
        }
        case 0xD0: case 0xD1: case 0xD2: case 0xD3: case 0xD4: case 0xD5: case 0xD6: case 0xD7: put_marker(cur, marker); break;
        case 0xD9:
            put_marker(cur, 0xD9);
            eoi = true;
            break;
        default:
            if (strip) read_segment(r, nullptr);
            else copy_segment(marker);
            break;
        }
    }
    flush();
}

// Both walks over one file.  A failure behind the scan is late -- kept in p.late, the pieces dropped -- unless it is NOT_SUPPORTED;
// every other failure is thrown.
inline void walk_file(WalkPlan &p, ScanEndCache &ends, const uint8_t *data, size_t len, bool strip, bool swallow_terminator = false, bool turned = false) {
    ScanWalk w;
    try {
        walk_scan(p, w, ends, data, len, swallow_terminator);
        walk_optimize(p, w, ends, data, len, strip, swallow_terminator, turned);
    } catch (const Refuse &e) {
        if (!w.after_scan || e.status == JPGPU_ERR_NOT_SUPPORTED) throw;
        p.late = e;
        p.pieces.clear();
    }
}

// The same walks with the reader resuming inside the scan's terminating marker: only the verdict is kept, in p.swallow (a walk
// that still goes through would write a different file: refused)
inline void walk_swallowed_terminator(WalkPlan &p, ScanEndCache &ends, const uint8_t *data, size_t len, bool strip) {
    WalkPlan alt;
    p.swallow = {JPGPU_ERR_NOT_SUPPORTED, kDetailUnsupportedFrame,
                 "A scan that leaves one byte unread in front of its terminating marker is not supported by the optimizer path."};
    try {
        walk_file(alt, ends, data, len, strip, true);
        if (alt.late.status != JPGPU_OK) p.swallow = alt.late;
    } catch (const Refuse &e) {
        if (e.status != JPGPU_ERR_NOT_SUPPORTED) p.swallow = e;
    }
}

}  // namespace jpgpu
