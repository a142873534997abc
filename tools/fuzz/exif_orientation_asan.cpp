// tools/fuzz/exif_orientation_asan.cpp -- the Exif orientation rule (csrc/ingest_host.h: exif_orientation_of, note_exif_marker) and the window
// mapping (orientation_stored_rect) under AddressSanitizer / UBSan on the CPU: hand-made blocks with their expected values, then random edits
// and truncations of a valid block.  Every block is handed over in a heap allocation of exactly its size, so a read past it is reported.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -I jpeglibrary_amd/csrc tools/fuzz/exif_orientation_asan.cpp -o /tmp/exif_asan && /tmp/exif_asan [edits]
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "ingest_host.h"

using namespace jpgpu;

namespace {

typedef std::vector<uint8_t> Bytes;

void put16(Bytes &b, bool little, uint32_t v) {
    b.push_back((uint8_t)(little ? v : v >> 8));
    b.push_back((uint8_t)(little ? v >> 8 : v));
}
void put32(Bytes &b, bool little, uint32_t v) {
    put16(b, little, little ? v & 0xFFFF : v >> 16);
    put16(b, little, little ? v >> 16 : v & 0xFFFF);
}
struct Entry {
    uint32_t tag, type, count, value;
};
// the bytes behind "Exif\0\0": header, IFD0 at `ifd`, its entries (a SHORT value sits in the first two value bytes), the next-IFD offset
Bytes tiff(bool little, const std::vector<Entry> &entries, uint32_t magic = 42, uint32_t ifd = 8, int written_count = -1) {
    Bytes b = {(uint8_t)(little ? 'I' : 'M'), (uint8_t)(little ? 'I' : 'M')};
    put16(b, little, magic);
    put32(b, little, ifd);
    while (b.size() < ifd && b.size() < 64) b.push_back(0);
    put16(b, little, written_count < 0 ? (uint32_t)entries.size() : (uint32_t)written_count);
    for (const Entry &e : entries) {
        put16(b, little, e.tag);
        put16(b, little, e.type);
        put32(b, little, e.count);
        if (e.type == 3) {
            put16(b, little, e.value);
            put16(b, little, 0);
        } else {
            put32(b, little, e.value);
        }
    }
    put32(b, little, 0);
    return b;
}
// the rule on an exact-size heap copy
int rule(const Bytes &t) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[t.size() ? t.size() : 1]);
    if (!t.empty()) memcpy(copy.get(), t.data(), t.size());
    return exif_orientation_of(copy.get(), t.size());
}
int through_marker(const Bytes &t, ExifMarker &m, int marker = 0xE1, const char *id = "Exif\0\0") {
    Bytes p(id, id + 6);
    p.insert(p.end(), t.begin(), t.end());
    std::unique_ptr<uint8_t[]> copy(new uint8_t[p.size()]);
    memcpy(copy.get(), p.data(), p.size());
    note_exif_marker(m, marker, copy.get(), p.size());
    return m.orientation;
}

int failures = 0;
void expect(int got, int want, const char *what) {
    if (got == want) return;
    fprintf(stderr, "%s: orientation %d, expected %d\n", what, got, want);
    failures++;
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
    const Entry make = {0x010F, 2, 4, 0x61626300}, soft = {0x0131, 2, 4, 0x78797A00};
    for (int little = 0; little < 2; little++) {
        for (uint32_t o = 0; o <= 9; o++) expect(rule(tiff(little, {make, {0x0112, 3, 1, o}, soft})), o >= 1 && o <= 8 ? (int)o : 1, "value 0..9");
        expect(rule(tiff(little, {{0x0112, 3, 1, 6}})), 6, "the only entry");
        expect(rule(tiff(little, {make, soft, {0x0112, 3, 1, 8}})), 8, "the third entry");
        expect(rule(tiff(little, {make, soft})), 1, "no tag");
        expect(rule(tiff(little, {{0x0112, 4, 1, 6}})), 1, "type LONG");
        expect(rule(tiff(little, {{0x0112, 3, 2, 6}})), 1, "count 2");
        expect(rule(tiff(little, {{0x0112, 3, 1, 6}}, 43)), 1, "magic 43");
        expect(rule(tiff(little, {{0x0112, 3, 1, 6}}, 42, 4000)), 1, "IFD offset past the end");
        expect(rule(tiff(little, {{0x0112, 3, 1, 6}}, 42, 0xFFFFFFF8u)), 1, "IFD offset near 2^32");
        expect(rule(tiff(little, {make}, 42, 8, 200)), 1, "entry count past the segment");
        expect(rule(tiff(little, {{0x0112, 3, 1, 5}, {0x0112, 3, 1, 7}})), 5, "the first of two tags");
        expect(rule(tiff(little, {{0x0112, 3, 1, 6}}, 42, 20)), 6, "IFD0 further on");
        Bytes whole = tiff(little, {make, {0x0112, 3, 1, 6}, soft});
        for (size_t n = 0; n <= whole.size(); n++) {  // every truncation: 6 once the entry is whole, 1 before
            const int got = rule(Bytes(whole.begin(), whole.begin() + n));
            const size_t needed = 8 + 2 + 12 * 2;
            expect(got, n >= needed ? 6 : 1, "truncated");
        }
    }
    expect(rule(Bytes()), 1, "a 6-byte payload");
    expect(rule(Bytes{'X', 'X', 0, 42, 0, 0, 0, 8}), 1, "no byte order");
    {
        ExifMarker m;
        expect(through_marker(tiff(false, {{0x0112, 3, 1, 3}}), m, 0xE1, "http:/"), 1, "an APP1 that is not Exif");
        expect(through_marker(tiff(false, {{0x0112, 3, 1, 3}}), m, 0xE2), 1, "an APP2");
        expect(through_marker(tiff(false, {{0x0112, 3, 1, 3}}), m), 3, "the first Exif APP1");
        expect(through_marker(tiff(false, {{0x0112, 3, 1, 6}}), m), 3, "a second Exif APP1 is not read");
        ExifMarker broken;
        expect(through_marker(tiff(false, {{0x0112, 3, 1, 6}}, 43), broken), 1, "a broken first block");
        expect(through_marker(tiff(false, {{0x0112, 3, 1, 6}}), broken), 1, "... still counts as the first");
        ExifMarker tiny;
        const uint8_t five[5] = {'E', 'x', 'i', 'f', 0};
        std::unique_ptr<uint8_t[]> copy(new uint8_t[5]);
        memcpy(copy.get(), five, 5);
        note_exif_marker(tiny, 0xE1, copy.get(), 5);
        expect(tiny.seen ? 0 : 1, 1, "a 5-byte payload is no Exif segment");
    }
    // random edits of a valid block: any value 1..8 may come out, nothing may be read outside
    const Bytes valid = tiff(true, {make, {0x0112, 3, 1, 6}, soft});
    size_t changed = 0;
    for (int k = 0; k < edits; k++) {
        Bytes b = k & 1 ? valid : tiff(false, {make, soft, {0x0112, 3, 1, 7}});
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
        const int o = rule(b);
        if (o < 1 || o > 8) {
            fprintf(stderr, "edit %d: orientation %d\n", k, o);
            failures++;
        }
        changed += o != (k & 1 ? 6 : 7);
        ExifMarker m;
        (void)through_marker(b, m);
    }
    // the window mapping: a rectangle inside the oriented frame maps to one of the same area inside the stored frame
    for (int k = 0; k < edits; k++) {
        const uint32_t w = 1 + rnd(300), h = 1 + rnd(300);
        const int o = 1 + (int)rnd(8);
        const uint32_t ow = orientation_transposes(o) ? h : w, oh = orientation_transposes(o) ? w : h;
        jpgpu_rect r;
        r.x = rnd(ow);
        r.y = rnd(oh);
        r.width = 1 + rnd(ow - r.x);
        r.height = 1 + rnd(oh - r.y);
        const jpgpu_rect s = orientation_stored_rect(o, r, w, h);
        if ((uint64_t)s.x + s.width > w || (uint64_t)s.y + s.height > h || (uint64_t)s.width * s.height != (uint64_t)r.width * r.height) {
            fprintf(stderr, "orientation %d: {%u, %u, %u, %u} of %u x %u maps outside\n", o, r.x, r.y, r.width, r.height, w, h);
            failures++;
        }
    }
    printf("exif ok: %d edits, %zu of them changed the value, %d failures\n", edits, changed, failures);
    return failures ? 1 : 0;
}
