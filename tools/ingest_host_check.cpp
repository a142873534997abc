// tools/ingest_host_check.cpp -- the parts of the ingest that need no device (jpeglibrary_amd/csrc/ingest_host.h), run on the CPU under the
// host sanitizers: FileSegs::gather and FileSegs::at against a byte-serial model over awkward segment lists, and cut_stage_pieces
// (a piece never crosses a slot of the staging ring, never exceeds kStagePieceMax, the pieces tile the range in order), and the colour rule
// (note_color_marker reads exactly the payload it is given; color_kind_of row by row).
//
//     make -C tools ingest_host_check && tools/ingest_host_check
//
// Prints "ok" and exits 0; the first property that does not hold is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "../jpeglibrary_amd/csrc/ingest_host.h"

using namespace jpgpu;

#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            exit(1);                                               \
        }                                                          \
    } while (0)

static void check_file(const std::vector<std::vector<uint8_t>> &parts) {
    std::vector<jpgpu_segment> segs;
    std::vector<uint8_t> flat;
    for (const std::vector<uint8_t> &p : parts) {
        segs.push_back({p.empty() ? nullptr : p.data(), p.size()});  // (an empty segment has no pointer anybody may read)
        flat.insert(flat.end(), p.begin(), p.end());
    }
    FileSegs f;
    f.seg = segs.data();
    f.n = (int)segs.size();
    f.len = flat.size();
    for (size_t off = 0; off < flat.size(); off++) CHECK(f.at(off) == flat[off]);
    CHECK(f.at(flat.size()) == 0 && f.at(flat.size() + 1) == 0 && f.at(flat.size() + (1u << 20)) == 0);  // behind the file: zero, no read
    for (size_t want : {(size_t)0, (size_t)1, flat.size() / 2, flat.size() - (flat.empty() ? 0 : 1), flat.size(), flat.size() + 1, FileSegs::kHeadBytes, (size_t)-1}) {
        f.gather(want);
        const size_t got = std::min(want, flat.size());
        CHECK(f.base_len == got && f.whole() == (got == flat.size()));
        CHECK(got == 0 || memcmp(f.base, flat.data(), got) == 0);
    }
}

static void check_cut(const uint8_t *src, uint64_t dst, uint64_t n, uint64_t slot) {
    std::vector<StagePiece> pieces;
    cut_stage_pieces(pieces, src, dst, n, slot);
    uint64_t at = dst;
    for (const StagePiece &p : pieces) {
        CHECK(p.n > 0 && p.n <= kStagePieceMax);
        CHECK(p.dst == at && p.dst / slot == (p.dst + p.n - 1) / slot);
        CHECK(src ? p.src == src + (at - dst) : p.src == nullptr);
        at += p.n;
    }
    CHECK(at == dst + n && (n != 0 || pieces.empty()));
}

int main() {
    std::mt19937 rng(7);
    auto bytes = [&](size_t n) {
        std::vector<uint8_t> v(n);
        for (uint8_t &b : v) b = (uint8_t)rng();
        return v;
    };
    check_file({});
    check_file({{}});
    check_file({bytes(1)});
    check_file({{}, bytes(1), {}, {}, bytes(2), {}});
    check_file({bytes(16384), bytes(16384), bytes(16384), bytes(16384), bytes(5)});   // the head ends exactly at a segment's end
    check_file({bytes(FileSegs::kHeadBytes - 1), bytes(3), bytes(70000)});             // ... inside a segment
    for (int k = 0; k < 50; k++) {
        std::vector<std::vector<uint8_t>> parts;
        for (int s = (int)(rng() % 9); s > 0; s--) parts.push_back(bytes(rng() % 4 == 0 ? 0 : rng() % 3000));
        check_file(parts);
    }
    // a device file answers with its two verdict bytes and nothing else
    FileSegs d;
    d.device = true;
    d.len = 100;
    d.verdict_at = 40;
    d.verdict = 0xD9FFu;
    CHECK(d.at(40) == 0xFF && d.at(41) == 0xD9 && d.at(39) == 0 && d.at(42) == 0 && d.at(0) == 0);

    const std::vector<uint8_t> src(22u << 20);  // (only addresses inside it are formed)
    for (uint64_t slot : {(uint64_t)1 << 20, (uint64_t)3 << 20, (uint64_t)32 << 20, (uint64_t)4097}) {
        for (uint64_t dst : {(uint64_t)0, (uint64_t)256, slot - 1, slot, slot + 1, 5 * slot - 7, ((uint64_t)1 << 32) + 3})
            for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)255, slot - 1, slot, slot + 1, (uint64_t)kStagePieceMax, (uint64_t)kStagePieceMax + 1, 7 * slot + 13}) {
                if (n <= src.size()) check_cut(src.data(), dst, n, slot);
                check_cut(nullptr, dst, n, slot);
            }
    }
    // the colour rule: payloads allocated at their exact length, so a read behind one is caught
    auto marker = [](ColorMarkers &m, int code, const char *tag, size_t len, int at11) {
        std::vector<uint8_t> p(len);
        for (size_t i = 0; i < len && i < 5; i++) p[i] = (uint8_t)tag[i];
        if (len > 11) p[11] = (uint8_t)at11;
        note_color_marker(m, code, p.data(), len);
    };
    ColorMarkers m;
    marker(m, 0xEE, "Adobe", 11, 0);  // too short: no transform byte
    marker(m, 0xE0, "JFIF", 13, 0);
    marker(m, 0xEE, "Adobf", 12, 0);
    marker(m, 0xE1, "Adobe", 12, 0);
    note_color_marker(m, 0xEE, nullptr, 0);
    CHECK(!m.saw_jfif && m.adobe_transform == -1);
    const uint8_t rgb[4] = {0x52, 0x47, 0x42, 0}, ycc[4] = {1, 2, 3, 4};
    CHECK(color_kind_of(8, 1, ycc, m) == JPGPU_COLOR_KIND_GRAY && color_kind_of(8, 3, ycc, m) == JPGPU_COLOR_KIND_YCBCR);
    CHECK(color_kind_of(8, 3, rgb, m) == JPGPU_COLOR_KIND_RGB && color_kind_of(8, 3, nullptr, m) == JPGPU_COLOR_KIND_YCBCR);
    CHECK(color_kind_of(8, 4, ycc, m) == JPGPU_COLOR_KIND_CMYK);
    CHECK(color_kind_of(8, 2, ycc, m) == -1 && color_kind_of(8, 5, ycc, m) == -1 && color_kind_of(12, 3, ycc, m) == -1 && color_kind_of(12, 4, ycc, m) == -1);
    marker(m, 0xEE, "Adobe", 12, 2);
    CHECK(m.adobe_transform == 2 && color_kind_of(8, 4, ycc, m) == JPGPU_COLOR_KIND_YCCK && color_kind_of(8, 3, rgb, m) == JPGPU_COLOR_KIND_YCBCR);
    marker(m, 0xEE, "Adobe", 14, 0);  // the last one wins
    CHECK(m.adobe_transform == 0 && color_kind_of(8, 4, ycc, m) == JPGPU_COLOR_KIND_CMYK && color_kind_of(8, 3, ycc, m) == JPGPU_COLOR_KIND_RGB);
    marker(m, 0xE0, "JFIF", 14, 0);
    CHECK(m.saw_jfif && color_kind_of(8, 3, rgb, m) == JPGPU_COLOR_KIND_YCBCR && color_kind_of(8, 4, ycc, m) == JPGPU_COLOR_KIND_CMYK);
    printf("ok\n");
    return 0;
}
