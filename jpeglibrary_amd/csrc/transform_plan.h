// jpeglibrary_amd/csrc/transform_plan.h -- the host side of the optimizer's lossless transform (include/jpgpu.h section (5), "Lossless
// transform"): a file's headers, the orientation rule and the edge policy -> what the image is turned by, or its refusal.  No device, no HIP:
// jpgpu_transform_plan, jpgpu_transform_plan_window, OptimizeBatch::upload and the stand-alone sanitizer harnesses
// (tools/fuzz/transform_plan_asan.cpp and, for the window, tools/fuzz/crop_plan_asan.cpp, linked with host_parser.cpp for the marker reader
// and the header parsers) share it.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/jpgpu.h"
#include "host.h"
#include "ingest_host.h"

namespace jpgpu {

// A lossless transform resolved on the host (include/jpgpu.h section (5), "Lossless transform"): what jpgpu_transform_plan reports, and what
// OptimizeBatch::upload turns an image by.  status != JPGPU_OK: the refusal of this image, with its message.
struct TransformPlan {
    int status = JPGPU_OK;
    std::string message;
    int orientation = 1;     // the one applied
    bool from_file = false;  // ... which the policy took from the file's Exif block (not the caller's value)
    size_t exif_value_at = 0;  // from_file: the two bytes of the tag's value in the file ...
    bool exif_little = false;  // ... and their byte order
    bool trimmed = false;
    int ncomp = 0;
    uint8_t h[4] = {}, v[4] = {};  // the source's factors, frame order
    uint32_t max_h = 1, max_v = 1;
    uint32_t src_width = 0, src_height = 0;          // the file's
    uint32_t kept_width = 0, kept_height = 0;        // ... behind the trim
    uint32_t src_mcus_per_line = 0, src_mcus_per_column = 0, kept_mcus_per_line = 0, kept_mcus_per_column = 0;
    uint32_t out_width = 0, out_height = 0;          // kept, swapped for 5..8
    size_t sof_at = 0;  // the frame header's payload (precision byte) in the file
    struct Segment {
        size_t at, length;
    };
    std::vector<Segment> dqt;  // the payloads of the DQT segments in front of the scan
    // the window ("Window" of the same section): in pixels of the frame of F' (turned_width x turned_height, the turned frame behind the trim).
    // With one, out_width x out_height is the window's size, and win_* is what it keeps of the MCU grid of F'.
    bool has_window = false;
    int origin = JPGPU_ORIGIN_REFUSE;
    jpgpu_rect window = {0, 0, 0, 0}, applied = {0, 0, 0, 0};  // as asked for; as applied (behind JPGPU_ORIGIN_EXPAND)
    uint32_t turned_width = 0, turned_height = 0;
    uint32_t win_mcu_x = 0, win_mcu_y = 0, win_mcus_per_line = 0, win_mcus_per_column = 0;
    bool transposes() const { return orientation >= 5; }
    // the image takes the coefficient road (entropy decode, KX, the encoder's entropy stages): it is turned, or cut, or both
    bool coefficient_road() const { return orientation != 1 || has_window; }
};
// orientation: 0 = by `policy` (a jpgpu_orientation_policy), 1..8 as given.  window: NULL or all zero = none (nothing below changes for it);
// origin: a jpgpu_origin_policy.  Returns JPGPU_OK (plan->status may refuse the image), or the library's header error for a file without a
// usable frame header.
// The headers of a file up to its first SOS: Identify()'s marker loop restated over the same reader (HostDecoder::identify_until_scan,
// host_parser.cpp: MarkerReader finds the markers -- bytes in front of one are stepped over, no leading SOI is asked for -- and reads the
// lengths with the reference's rule), so the Exif block found here is the one jpgpu_identify_orientation finds, and a file that walk
// accepts is accepted here.  Beside what Identify() keeps it notes WHERE things stand: the frame header, the DQT segments, the Exif value.
inline int plan_transform(const uint8_t *file, size_t len, int orientation, int policy, int edge, TransformPlan *tp, const jpgpu_rect *window = nullptr,
                          int origin = JPGPU_ORIGIN_REFUSE) {
    *tp = TransformPlan();
    if (window && (window->x | window->y | window->width | window->height) != 0) {
        tp->has_window = true;
        tp->window = *window;
        tp->origin = origin;
    }
    const auto header_error = [&](const char *msg) {
        tp->status = JPGPU_ERR_INVALID_DATA;
        tp->message = msg;
        return JPGPU_ERR_INVALID_DATA;
    };
    const auto refuse_image = [&](const std::string &msg) {
        tp->status = JPGPU_ERR_NOT_SUPPORTED;
        tp->message = msg;
        return JPGPU_OK;
    };
    if (!file || len == 0) return header_error("Input buffer is not specified.");
    bool have_frame = false, have_scan = false, eoi = false;
    int other_sof = 0;
    ExifMarker exif;
    uint8_t ids[4] = {}, scan_n = 0, scan_sel[4] = {};
    MarkerReader r(file, len);
    while (!have_scan && !eoi && !r.is_empty()) {
        int m;
        if (!r.try_read_marker(&m)) return header_error("No marker found.");
        if (m == kSOI || is_restart_marker(m)) continue;
        if (m == kEOI) {
            eoi = true;
            continue;
        }
        uint16_t length;
        const uint8_t *body;
        if (!r.try_read_length(&length)) return header_error("Unexpected end of input data when reading segment length.");
        const bool any_sof = m >= 0xC0 && m <= 0xCF && m != kDHT && m != 0xC8 && m != kDAC;
        if (!any_sof && m != kSOS && m != kDRI && m != kDQT) {  // (Identify's ProcessOtherMarker: APPn, COM, DHT, ...)
            if ((int)length <= r.remaining_byte_count()) {
                const uint8_t *payload = r.remaining_bytes();
                const bool first_exif = !exif.seen;
                note_exif_marker(exif, m, payload, length);
                if (first_exif && exif.seen) tp->exif_value_at = (size_t)(payload - file) + 6 + exif.value_at;
            }
            if (!r.try_advance(length)) return header_error("Unexpected end of input data reached.");
            continue;
        }
        if (!r.try_read_bytes(length, &body)) return header_error("Unexpected end of input data when reading segment content.");
        if (any_sof) {
            FrameHeader fh;
            int consumed = 0;
            if (!FrameHeader::try_parse(body, length, false, &fh, &consumed)) return header_error("Failed to parse frame header.");
            if (have_frame) return header_error("Multiple frame is not supported.");
            have_frame = true;
            if (m != kSOF0 && m != kSOF1) other_sof = m;
            tp->sof_at = (size_t)(body - file);
            tp->src_height = fh.lines;
            tp->src_width = fh.samples_per_line;
            tp->ncomp = fh.num_components;
            for (int c = 0; c < tp->ncomp && c < 4; c++) {
                ids[c] = fh.components[(size_t)c].identifier;
                tp->h[c] = fh.components[(size_t)c].h;
                tp->v[c] = fh.components[(size_t)c].v;
            }
        } else if (m == kSOS) {
            ScanHeader sh;
            int consumed = 0;
            if (!ScanHeader::try_parse(body, length, false, &sh, &consumed)) return header_error("Failed to parse scan header.");
            have_scan = true;
            scan_n = sh.num_components;
            for (int c = 0; c < scan_n && c < 4; c++) scan_sel[c] = sh.components[(size_t)c].selector;
        } else if (m == kDRI) {
            if (length < 2) return header_error("Unexpected end of input data when reading segment content.");
        } else {  // DQT: where its tables stand (patch_turned_file transposes them)
            tp->dqt.push_back({(size_t)(body - file), (size_t)length});
        }
    }
    if (!have_frame) return header_error("Frame header was not found.");
    if (!have_scan) return header_error("No image data is read.");
    tp->exif_little = exif.little;
    const int exif_orientation = exif.orientation;
    tp->orientation = orientation != 0 ? orientation : (policy == JPGPU_ORIENT_FILE ? exif_orientation : 1);
    tp->from_file = orientation == 0 && tp->orientation != 1;
    tp->kept_width = tp->out_width = tp->src_width;
    tp->kept_height = tp->out_height = tp->src_height;
    tp->turned_width = tp->src_width;
    tp->turned_height = tp->src_height;
    if (!tp->coefficient_road()) return JPGPU_OK;  // (today's road: nothing below is asked of the file)
    const int o = tp->orientation;
    if (other_sof != 0)
        return refuse_image(other_sof == kSOF2 ? "Progressive JPEG is not supported by the optimizer path." : "This type of JPEG stream is not supported by the optimizer path.");
    if (tp->ncomp < 1 || tp->ncomp > 4) return refuse_image("A frame of more than four components cannot be turned.");
    if (tp->src_width == 0 || tp->src_height == 0) return refuse_image("A frame without a size in its header cannot be turned.");
    uint32_t bpm = 0;
    for (int c = 0; c < tp->ncomp; c++) {
        if (tp->h[c] < 1 || tp->h[c] > 4 || tp->v[c] < 1 || tp->v[c] > 4) return refuse_image("Sampling factors outside 1..4 cannot be turned.");
        tp->max_h = std::max<uint32_t>(tp->max_h, tp->h[c]);
        tp->max_v = std::max<uint32_t>(tp->max_v, tp->v[c]);
        bpm += (uint32_t)tp->h[c] * tp->v[c];
    }
    if (bpm > 10) return refuse_image("More than ten blocks per MCU cannot be turned.");
    if (tp->ncomp == 1 && bpm != 1) return refuse_image("A one-component frame whose sampling factors are not 1 x 1 cannot be turned.");
    bool whole_frame = scan_n == tp->ncomp;
    for (int c = 0; whole_frame && c < tp->ncomp; c++) whole_frame = scan_sel[c] == ids[c];
    if (!whole_frame) return refuse_image("A scan that does not hold every component of the frame once, in frame order, cannot be turned.");
    const uint32_t mcu_w = 8 * tp->max_h, mcu_h = 8 * tp->max_v;
    tp->src_mcus_per_line = (tp->src_width + mcu_w - 1) / mcu_w;
    tp->src_mcus_per_column = (tp->src_height + mcu_h - 1) / mcu_h;
    const struct {
        bool mirrored;
        uint32_t *kept;
        uint32_t mcu;
        const char *name, *axis;
    } axes[2] = {{orientation_flips_x(o), &tp->kept_width, mcu_w, "width", "x"}, {orientation_flips_y(o), &tp->kept_height, mcu_h, "height", "y"}};
    for (const auto &a : axes) {
        if (!a.mirrored || *a.kept % a.mcu == 0) continue;
        const std::string what = std::string("The ") + a.name + " (" + std::to_string(*a.kept) + ") is ";
        if (edge != JPGPU_EDGE_TRIM)
            return refuse_image(what + "not a whole number of MCUs (" + std::to_string(a.mcu) + " pixels) and orientation " + std::to_string(o) + " mirrors the " +
                                a.axis + " axis.");
        if (*a.kept < a.mcu) return refuse_image(what + "shorter than one MCU (" + std::to_string(a.mcu) + " pixels): nothing is left of the mirrored " + a.axis + " axis.");
        *a.kept -= *a.kept % a.mcu;
        tp->trimmed = true;
    }
    tp->kept_mcus_per_line = (tp->kept_width + mcu_w - 1) / mcu_w;
    tp->kept_mcus_per_column = (tp->kept_height + mcu_h - 1) / mcu_h;
    tp->out_width = tp->transposes() ? tp->kept_height : tp->kept_width;
    tp->out_height = tp->transposes() ? tp->kept_width : tp->kept_height;
    tp->turned_width = tp->out_width;
    tp->turned_height = tp->out_height;
    if (!tp->has_window) return JPGPU_OK;
    // ---- the window, in the frame of F': the orientation and the edge policy are resolved by now, on the whole frame
    const jpgpu_rect w = tp->window;
    const std::string rect = "The window {" + std::to_string(w.x) + ", " + std::to_string(w.y) + ", " + std::to_string(w.width) + ", " + std::to_string(w.height) + "} ";
    const auto bad_window = [&](const std::string &msg) {
        tp->status = JPGPU_ERR_ARGUMENT;
        tp->message = msg;
        return JPGPU_OK;
    };
    if (w.width == 0 || w.height == 0) return bad_window(rect + "has a zero side.");
    if ((uint64_t)w.x + w.width > tp->turned_width || (uint64_t)w.y + w.height > tp->turned_height)
        return bad_window(rect + "lies outside the " + std::to_string(tp->turned_width) + " x " + std::to_string(tp->turned_height) + " frame.");
    const uint32_t mw = tp->transposes() ? mcu_h : mcu_w, mh = tp->transposes() ? mcu_w : mcu_h;  // the MCU of F'
    jpgpu_rect a = w;
    if (a.x % mw != 0 || a.y % mh != 0) {
        if (origin != JPGPU_ORIGIN_EXPAND) {
            const bool in_x = a.x % mw != 0;
            return refuse_image(std::string("The window's ") + (in_x ? "x" : "y") + " (" + std::to_string(in_x ? a.x : a.y) + ") is not a multiple of the MCU " +
                                (in_x ? "width" : "height") + " (" + std::to_string(in_x ? mw : mh) + " pixels).");
        }
        a.width += a.x % mw;
        a.x -= a.x % mw;
        a.height += a.y % mh;
        a.y -= a.y % mh;
    }
    tp->applied = a;
    tp->win_mcu_x = a.x / mw;
    tp->win_mcu_y = a.y / mh;
    tp->win_mcus_per_line = (a.width + mw - 1) / mw;
    tp->win_mcus_per_column = (a.height + mh - 1) / mh;
    tp->out_width = a.width;
    tp->out_height = a.height;
    return JPGPU_OK;
}

inline void transform_info_of(const TransformPlan &tp, jpgpu_transform_info *info) {
    memset(info, 0, sizeof *info);
    info->orientation = tp.orientation;
    info->trimmed = tp.trimmed ? 1 : 0;
    info->width = tp.out_width;
    info->height = tp.out_height;
    info->num_components = (uint32_t)std::min(tp.ncomp, 4);
    for (int c = 0; c < tp.ncomp && c < 4; c++) {
        info->h[c] = tp.transposes() ? tp.v[c] : tp.h[c];
        info->v[c] = tp.transposes() ? tp.h[c] : tp.v[c];
    }
}

// F' (with a window: F'') in place: `b` holds a copy of the file `tp` was planned from (status JPGPU_OK, on the coefficient road).  The SOF's
// size -- the window's where there is one -- and, for 5..8, its factor nibbles; for 5..8 every table of every DQT segment in front of the scan transposed; the Exif value where the file decided.
// Every place written is one plan_transform read through the marker reader's own bounds checks: the frame header's 6 + 3 n bytes, the DQT
// payloads it recorded, the two bytes of the Exif value.
inline void patch_turned_file(uint8_t *b, size_t len, const TransformPlan &tp) {
    (void)len;
    uint8_t *sof = b + tp.sof_at;
    sof[1] = (uint8_t)(tp.out_height >> 8);
    sof[2] = (uint8_t)tp.out_height;
    sof[3] = (uint8_t)(tp.out_width >> 8);
    sof[4] = (uint8_t)tp.out_width;
    if (tp.transposes()) {
        for (int c = 0; c < tp.ncomp; c++) sof[7 + 3 * c] = (uint8_t)(tp.v[c] << 4 | tp.h[c]);
        // every table of every DQT segment in front of the scan: entry zz(v, u) <- entry zz(u, v)
        uint8_t zz[64], nat[64];
        for (int k = 0; k < 64; k++) zz[k] = 0;
        {
            int k = 0;
            for (int s = 0; s < 15; s++)  // the zig-zag walk: anti-diagonal s, upwards for even s
                for (int t = 0; t <= s; t++) {
                    const int v = (s & 1) ? t : s - t, u = s - v;
                    if (v < 8 && u < 8) nat[k++] = (uint8_t)(v * 8 + u);
                }
            for (k = 0; k < 64; k++) zz[nat[k]] = (uint8_t)k;
        }
        for (const TransformPlan::Segment &seg : tp.dqt) {
            size_t at = seg.at;
            const size_t end = seg.at + seg.length;
            while (at < end) {
                const size_t bytes = (b[at] >> 4) != 0 ? 2 : 1;
                if (at + 1 + 64 * bytes > end) break;
                uint8_t *e = b + at + 1;
                for (int k = 0; k < 64; k++) {
                    const int other = zz[(nat[k] & 7) * 8 + (nat[k] >> 3)];
                    if (other <= k) continue;
                    for (size_t j = 0; j < bytes; j++) std::swap(e[(size_t)k * bytes + j], e[(size_t)other * bytes + j]);
                }
                at += 1 + 64 * bytes;
            }
        }
    }
    if (tp.from_file) {
        b[tp.exif_value_at] = tp.exif_little ? 1 : 0;
        b[tp.exif_value_at + 1] = tp.exif_little ? 0 : 1;
    }
}

}  // namespace jpgpu
