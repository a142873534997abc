// tools/fuzz/crop_plan_asan.cpp -- the window of the optimizer's lossless transform (csrc/transform_plan.h: plan_transform with a window, and
// the SOF patch of F'') under AddressSanitizer / UBSan on the CPU: a hand-made 4:2:0 baseline header, planned and patched with windows under
// every orientation and both origin policies, then seeded edits of the header AND of the window (coordinates near the frame's size, near 2^32,
// zero sides).  Every file is handed over in a heap allocation of exactly its size, so a read or a write past it is reported; every plan that
// comes back good is checked against the invariants KX relies on (the window's MCUs lie inside the grid of F').
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -I jpeglibrary_amd/csrc tools/fuzz/crop_plan_asan.cpp jpeglibrary_amd/csrc/host_parser.cpp -o /tmp/crop_asan && /tmp/crop_asan [edits]
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "transform_plan.h"

using namespace jpgpu;

namespace {

typedef std::vector<uint8_t> Bytes;

void segment(Bytes &f, int marker, const Bytes &body) {
    f.push_back(0xFF);
    f.push_back((uint8_t)marker);
    f.push_back((uint8_t)((body.size() + 2) >> 8));
    f.push_back((uint8_t)(body.size() + 2));
    f.insert(f.end(), body.begin(), body.end());
}

// SOI, DQT (one 8-bit table), SOF0 4:2:0, DHT (empty), DRI, SOS, two bytes, EOI
Bytes file(uint32_t width, uint32_t height) {
    Bytes f = {0xFF, 0xD8};
    Bytes dqt = {0x00};
    for (int k = 0; k < 64; k++) dqt.push_back((uint8_t)(k + 1));
    segment(f, 0xDB, dqt);
    segment(f, 0xC0, Bytes{8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8), (uint8_t)width, 3, 1, 0x22, 0, 2, 0x11, 0, 3, 0x11, 0});
    segment(f, 0xC4, Bytes{0x00, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
    segment(f, 0xDD, Bytes{0, 3});
    segment(f, 0xDA, Bytes{3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    f.insert(f.end(), {0x12, 0x34, 0xFF, 0xD9});
    return f;
}

int failures = 0;
void expect(bool ok, const char *what) {
    if (ok) return;
    fprintf(stderr, "%s\n", what);
    failures++;
}

// what a good windowed plan promises whoever fills KX's descriptor from it
void check_invariants(const TransformPlan &tp) {
    if (tp.status != JPGPU_OK || !tp.has_window) return;
    const uint32_t mw = 8 * (tp.transposes() ? tp.max_v : tp.max_h), mh = 8 * (tp.transposes() ? tp.max_h : tp.max_v);
    const uint32_t grid_w = tp.transposes() ? tp.kept_mcus_per_column : tp.kept_mcus_per_line, grid_h = tp.transposes() ? tp.kept_mcus_per_line : tp.kept_mcus_per_column;
    expect(tp.win_mcus_per_line >= 1 && tp.win_mcus_per_column >= 1, "a window keeps at least one MCU");
    expect((uint64_t)tp.win_mcu_x + tp.win_mcus_per_line <= grid_w && (uint64_t)tp.win_mcu_y + tp.win_mcus_per_column <= grid_h, "the window's MCUs lie inside the grid");
    expect(tp.applied.x % mw == 0 && tp.applied.y % mh == 0, "the applied origin is aligned");
    expect(tp.applied.x <= tp.window.x && tp.applied.y <= tp.window.y && tp.applied.x + tp.applied.width == tp.window.x + tp.window.width &&
               tp.applied.y + tp.applied.height == tp.window.y + tp.window.height,
           "the applied window ends where the asked one ends and holds it");
    expect(tp.out_width == tp.applied.width && tp.out_height == tp.applied.height, "the output's size is the applied window's");
    expect((uint64_t)tp.applied.x + tp.applied.width <= tp.turned_width && (uint64_t)tp.applied.y + tp.applied.height <= tp.turned_height, "inside the frame");
}

// plan and, where the image takes the coefficient road, patch: both on exact-size heap copies
int run(const Bytes &f, int orientation, int edge, const jpgpu_rect *window, int origin, TransformPlan *tp) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[f.size() ? f.size() : 1]);
    if (!f.empty()) memcpy(copy.get(), f.data(), f.size());
    const int rc = plan_transform(copy.get(), f.size(), orientation, JPGPU_ORIENT_STORED, edge, tp, window, origin);
    jpgpu_transform_info info;
    transform_info_of(*tp, &info);
    if (rc != JPGPU_OK) return rc;
    check_invariants(*tp);
    if (tp->status == JPGPU_OK && tp->coefficient_road()) {
        patch_turned_file(copy.get(), f.size(), *tp);
        TransformPlan again;  // F'' has a header of its own
        if (plan_transform(copy.get(), f.size(), 1, JPGPU_ORIENT_STORED, edge, &again) != JPGPU_OK || again.src_width != tp->out_width ||
            again.src_height != tp->out_height) {
            fprintf(stderr, "the patched header does not say %u x %u\n", tp->out_width, tp->out_height);
            failures++;
        }
    }
    return rc;
}

uint64_t rng_state = 0xD1B54A32D192ED03ull;
uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 32) % (n ? n : 1));
}
// a coordinate that is small, near `size`, or near 2^32
uint32_t coordinate(uint32_t size) {
    switch (rnd(6)) {
    case 0: return 0;
    case 1: return size - rnd(4) + rnd(4);
    case 2: return 0xFFFFFFFFu - rnd(40);
    case 3: return 16 * rnd(6);
    default: return rnd(size + 8);
    }
}

}  // namespace

int main(int argc, char **argv) {
    const int edits = argc > 1 ? atoi(argv[1]) : 4000;
    TransformPlan tp;
    const Bytes f = file(48, 32);  // 3 x 2 MCUs of 16 x 16
    for (int o = 1; o <= 8; o++) {
        const uint32_t W = o >= 5 ? 32u : 48u, H = o >= 5 ? 48u : 32u;
        const jpgpu_rect one = {16, 16, 16, 16}, off = {20, 8, 10, 20}, out = {16, 16, W, 8}, flat = {0, 0, 8, 0}, far = {0xFFFFFFF0u, 0, 0x20u, 8}, all = {0, 0, W, H};
        expect(run(f, o, JPGPU_EDGE_REFUSE, &one, JPGPU_ORIGIN_REFUSE, &tp) == JPGPU_OK && tp.status == JPGPU_OK && tp.win_mcu_x == 1 && tp.win_mcu_y == 1 &&
                   tp.win_mcus_per_line == 1 && tp.win_mcus_per_column == 1 && tp.out_width == 16 && tp.out_height == 16,
               "one aligned MCU");
        expect(run(f, o, JPGPU_EDGE_REFUSE, &off, JPGPU_ORIGIN_REFUSE, &tp) == JPGPU_OK && tp.status == JPGPU_ERR_NOT_SUPPORTED, "unaligned: refused");
        expect(run(f, o, JPGPU_EDGE_REFUSE, &off, JPGPU_ORIGIN_EXPAND, &tp) == JPGPU_OK && tp.status == JPGPU_OK && tp.applied.x == 16 && tp.applied.y == 0 &&
                   tp.applied.width == 14 && tp.applied.height == 28 && tp.win_mcus_per_line == 1 && tp.win_mcus_per_column == 2,
               "unaligned: expanded");
        expect(run(f, o, JPGPU_EDGE_REFUSE, &out, JPGPU_ORIGIN_EXPAND, &tp) == JPGPU_OK && tp.status == JPGPU_ERR_ARGUMENT, "outside the frame");
        expect(run(f, o, JPGPU_EDGE_REFUSE, &flat, JPGPU_ORIGIN_EXPAND, &tp) == JPGPU_OK && tp.status == JPGPU_ERR_ARGUMENT, "one zero side");
        expect(run(f, o, JPGPU_EDGE_REFUSE, &far, JPGPU_ORIGIN_EXPAND, &tp) == JPGPU_OK && tp.status == JPGPU_ERR_ARGUMENT, "x + w wraps past 2^32");
        expect(run(f, o, JPGPU_EDGE_REFUSE, &all, JPGPU_ORIGIN_REFUSE, &tp) == JPGPU_OK && tp.status == JPGPU_OK && tp.has_window && tp.coefficient_road() &&
                   tp.out_width == W && tp.out_height == H,
               "the whole frame written out");
        const jpgpu_rect none = {0, 0, 0, 0};
        TransformPlan plain;
        (void)run(f, o, JPGPU_EDGE_REFUSE, nullptr, JPGPU_ORIGIN_REFUSE, &plain);
        expect(run(f, o, JPGPU_EDGE_REFUSE, &none, JPGPU_ORIGIN_EXPAND, &tp) == JPGPU_OK && !tp.has_window && tp.out_width == plain.out_width &&
                   tp.out_height == plain.out_height && tp.coefficient_road() == (o != 1),
               "an all-zero window is no window");
    }
    // the mirrored edge is resolved before the window: a 40-wide frame under orientation 2 is refused, or trimmed to 32 with the window inside THAT
    const jpgpu_rect left = {0, 0, 16, 16}, right = {32, 0, 8, 16};
    expect(run(file(40, 27), 2, JPGPU_EDGE_REFUSE, &left, JPGPU_ORIGIN_REFUSE, &tp) == JPGPU_OK && tp.status == JPGPU_ERR_NOT_SUPPORTED, "the edge refuses before the window");
    expect(run(file(40, 27), 2, JPGPU_EDGE_TRIM, &left, JPGPU_ORIGIN_REFUSE, &tp) == JPGPU_OK && tp.status == JPGPU_OK && tp.trimmed, "trim, then window");
    expect(run(file(40, 27), 2, JPGPU_EDGE_TRIM, &right, JPGPU_ORIGIN_REFUSE, &tp) == JPGPU_OK && tp.status == JPGPU_ERR_ARGUMENT, "outside the trimmed frame");
    expect(run(file(40, 27), 1, JPGPU_EDGE_REFUSE, &right, JPGPU_ORIGIN_REFUSE, &tp) == JPGPU_OK && tp.status == JPGPU_OK, "inside the untrimmed one");
    for (size_t n = 0; n <= f.size(); n++) (void)run(Bytes(f.begin(), f.begin() + n), 6, JPGPU_EDGE_TRIM, &left, JPGPU_ORIGIN_EXPAND, &tp);  // every truncation
    size_t cut = 0;
    for (int k = 0; k < edits; k++) {
        const uint32_t width = 8 + rnd(120), height = 8 + rnd(120);
        Bytes b = file(width, height);
        for (uint32_t e = 0, n = rnd(4); e < n && !b.empty(); e++) {  // (no edit at all in a quarter of the rounds: the window alone varies)
            const uint32_t pos = rnd((uint32_t)b.size());
            switch (rnd(5)) {
            case 0: b[pos] ^= (uint8_t)(1u << rnd(8)); break;
            case 1: b[pos] = (uint8_t)rnd(256); break;
            case 2: b.erase(b.begin() + pos, b.begin() + std::min<size_t>(b.size(), pos + 1 + rnd(6))); break;
            case 3: b.insert(b.begin() + pos, (size_t)(1 + rnd(6)), (uint8_t)rnd(256)); break;
            default: b.resize(pos); break;
            }
        }
        const int o = (int)rnd(9);
        jpgpu_rect w = {coordinate(width), coordinate(height), coordinate(width), coordinate(height)};
        if (rnd(2)) {  // half of the windows lie inside the frame the header was written with, as the orientation turns it
            const uint32_t W = o >= 5 ? height : width, H = o >= 5 ? width : height;
            w.x = rnd(W);
            w.y = rnd(H);
            if (rnd(2)) {  // ... and half of those start on the MCU grid
                w.x -= w.x % 16;
                w.y -= w.y % 16;
            }
            w.width = 1 + rnd(W - w.x);
            w.height = 1 + rnd(H - w.y);
        }
        if (run(b, o, (int)rnd(2), &w, (int)rnd(2), &tp) == JPGPU_OK && tp.status == JPGPU_OK && tp.has_window) cut++;
    }
    printf("crop plan ok: %d edits, %zu of them still cut, %d failures\n", edits, cut, failures);
    return failures ? 1 : 0;
}
