// tools/fuzz/transform_plan_asan.cpp -- the host side of the optimizer's lossless transform (csrc/transform_plan.h: plan_transform,
// patch_turned_file) under AddressSanitizer / UBSan on the CPU: a hand-made baseline header with an Exif block and two DQT tables, planned and
// patched under every orientation, policy and edge policy, then random edits and truncations of it.  Every file is handed over in a heap
// allocation of exactly its size, so a read or a write past it is reported.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -I jpeglibrary_amd/csrc tools/fuzz/transform_plan_asan.cpp jpeglibrary_amd/csrc/host_parser.cpp -o /tmp/plan_asan && /tmp/plan_asan [edits]
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

// SOI, APP1 Exif (orientation o, big-endian), DQT (an 8-bit and a 16-bit table in one segment), SOF0 4:2:0, DHT (empty), SOS, two bytes, EOI
Bytes file(uint32_t width, uint32_t height, int o) {
    Bytes f = {0xFF, 0xD8};
    Bytes exif = {'E', 'x', 'i', 'f', 0, 0, 'M', 'M', 0, 42, 0, 0, 0, 8, 0, 1, 0x01, 0x12, 0, 3, 0, 0, 0, 1, 0, (uint8_t)o, 0, 0, 0, 0, 0, 0};
    segment(f, 0xE1, exif);
    Bytes dqt = {0x00};
    for (int k = 0; k < 64; k++) dqt.push_back((uint8_t)(k + 1));
    dqt.push_back(0x11);
    for (int k = 0; k < 64; k++) {
        dqt.push_back(1);
        dqt.push_back((uint8_t)k);
    }
    segment(f, 0xDB, dqt);
    segment(f, 0xC0, Bytes{8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8), (uint8_t)width, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    segment(f, 0xC4, Bytes{0x00, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
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

// plan and, where the image is turned, patch: both on exact-size heap copies
int run(const Bytes &f, int orientation, int policy, int edge, TransformPlan *tp) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[f.size() ? f.size() : 1]);
    if (!f.empty()) memcpy(copy.get(), f.data(), f.size());
    const int rc = plan_transform(copy.get(), f.size(), orientation, policy, edge, tp);
    jpgpu_transform_info info;
    transform_info_of(*tp, &info);
    if (rc == JPGPU_OK && tp->status == JPGPU_OK && tp->orientation != 1) {
        patch_turned_file(copy.get(), f.size(), *tp);
        TransformPlan again;  // F' has a header of its own: it plans under orientation 1
        if (plan_transform(copy.get(), f.size(), 1, JPGPU_ORIENT_STORED, edge, &again) != JPGPU_OK || again.src_width != tp->out_width ||
            again.src_height != tp->out_height) {
            fprintf(stderr, "the patched header does not say %u x %u\n", tp->out_width, tp->out_height);
            failures++;
        }
        if (tp->from_file) {
            TransformPlan by_file;
            (void)plan_transform(copy.get(), f.size(), 0, JPGPU_ORIENT_FILE, edge, &by_file);
            expect(by_file.orientation == 1, "the rewritten Exif tag says 1");
        }
    }
    return rc;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 32) % (n ? n : 1));
}

}  // namespace

int main(int argc, char **argv) {
    const int edits = argc > 1 ? atoi(argv[1]) : 4000;
    TransformPlan tp;
    for (int o = 1; o <= 8; o++) {
        expect(run(file(48, 32, 6), o, JPGPU_ORIENT_STORED, JPGPU_EDGE_REFUSE, &tp) == JPGPU_OK && tp.status == JPGPU_OK && tp.orientation == o, "aligned, as given");
        expect(tp.out_width == (o >= 5 ? 32u : 48u) && tp.out_height == (o >= 5 ? 48u : 32u) && !tp.trimmed && !tp.from_file, "aligned: the size");
        expect(run(file(48, 32, o), 0, JPGPU_ORIENT_FILE, JPGPU_EDGE_REFUSE, &tp) == JPGPU_OK && tp.orientation == o && tp.from_file == (o != 1), "by the file");
        expect(run(file(48, 32, o), 0, JPGPU_ORIENT_STORED, JPGPU_EDGE_REFUSE, &tp) == JPGPU_OK && tp.orientation == 1, "stored");
        const bool mx = o == 2 || o == 3 || o == 7 || o == 8, my = o == 3 || o == 4 || o == 6 || o == 7;
        (void)run(file(40, 27, 1), o, JPGPU_ORIENT_STORED, JPGPU_EDGE_REFUSE, &tp);
        expect((tp.status == JPGPU_OK) == !(mx || my), "partial axes: refused where one is mirrored");
        (void)run(file(40, 27, 1), o, JPGPU_ORIENT_STORED, JPGPU_EDGE_TRIM, &tp);
        expect(tp.status == JPGPU_OK && tp.trimmed == (mx || my) && tp.kept_width == (mx ? 32u : 40u) && tp.kept_height == (my ? 16u : 27u), "partial axes: trimmed");
        (void)run(file(12, 32, 1), o, JPGPU_ORIENT_STORED, JPGPU_EDGE_TRIM, &tp);
        expect((tp.status == JPGPU_OK) == !mx, "narrower than one MCU");
    }
    const Bytes valid = file(48, 32, 6);
    for (size_t n = 0; n <= valid.size(); n++) (void)run(Bytes(valid.begin(), valid.begin() + n), 0, JPGPU_ORIENT_FILE, JPGPU_EDGE_TRIM, &tp);  // every truncation
    size_t turned = 0;
    for (int k = 0; k < edits; k++) {
        Bytes b = file(8 + rnd(80), 8 + rnd(80), 1 + (int)rnd(8));
        for (uint32_t e = 0, n = 1 + rnd(4); e < n && !b.empty(); e++) {
            const uint32_t pos = rnd((uint32_t)b.size());
            switch (rnd(5)) {
            case 0: b[pos] ^= (uint8_t)(1u << rnd(8)); break;
            case 1: b[pos] = (uint8_t)rnd(256); break;
            case 2: b.erase(b.begin() + pos, b.begin() + std::min<size_t>(b.size(), pos + 1 + rnd(6))); break;
            case 3: b.insert(b.begin() + pos, (size_t)(1 + rnd(6)), (uint8_t)rnd(256)); break;
            default: b.resize(pos); break;
            }
        }
        std::unique_ptr<uint8_t[]> copy(new uint8_t[b.size() ? b.size() : 1]);
        if (!b.empty()) memcpy(copy.get(), b.data(), b.size());
        const int rc = plan_transform(copy.get(), b.size(), (int)rnd(9), (int)rnd(2), (int)rnd(2), &tp);
        if (rc == JPGPU_OK && tp.status == JPGPU_OK && tp.orientation != 1) {
            patch_turned_file(copy.get(), b.size(), tp);
            turned++;
        }
    }
    printf("plan ok: %d edits, %zu of them still turned, %d failures\n", edits, turned, failures);
    return failures ? 1 : 0;
}
