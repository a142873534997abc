// tools/fuzz/optimizer_walk_asan.cpp -- the optimizer's host walks (csrc/optimize_walk.h: Scan()'s and Optimize(strip)'s marker walks, the
// late-failure rule, the swallowed-terminator verdict) under AddressSanitizer / UBSan on the CPU.  Every file named on the command line is
// handed over in a heap allocation of exactly its size, so a read past it is reported, and walked as OptimizeBatch::upload walks it, for
// both values of `strip`.  One line of JSON per file: per strip the status, detail and message, the late and the swallowed verdicts, and the
// pieces of the output -- host bytes in hex, "DHT" and "ENTROPY" where the device's pieces go.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -I jpeglibrary_amd/csrc tools/fuzz/optimizer_walk_asan.cpp jpeglibrary_amd/csrc/host_parser.cpp -o /tmp/walk_asan && /tmp/walk_asan FILE...
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "optimize_walk.h"

using namespace jpgpu;

namespace {

void print_text(const std::string &s) {
    putchar('"');
    for (const char c : s) {
        if (c == '"' || c == '\\') putchar('\\');
        if ((unsigned char)c < 0x20) printf("\\u%04x", c);
        else putchar(c);
    }
    putchar('"');
}

void walk(const uint8_t *data, size_t len, bool strip) {
    WalkPlan p;
    ScanEndCache ends;
    try {
        walk_file(p, ends, data, len, strip);
    } catch (const Refuse &e) {
        p.refused(e);
    }
    if (p.status == JPGPU_OK) walk_swallowed_terminator(p, ends, data, len, strip);
    printf("{\"strip\": %d, \"status\": %d, \"detail\": %d, \"error\": ", (int)strip, p.status, p.detail);
    print_text(p.error);
    printf(", \"late_status\": %d, \"late_detail\": %d, \"late_error\": ", p.late.status, p.late.detail);
    print_text(p.late.error);
    printf(", \"swallow_status\": %d, \"swallow_detail\": %d, \"swallow_error\": ", p.swallow.status, p.swallow.detail);
    print_text(p.swallow.error);
    printf(", \"dri\": %d, \"rsts\": %zu, \"pieces\": [", p.dri_at_scan, p.rsts_in_scan);
    for (size_t k = 0; k < p.pieces.size(); k++) {
        const Piece &pc = p.pieces[k];
        printf("%s\"", k ? ", " : "");
        if (pc.kind == Piece::kHuffmanTables) printf("DHT");
        else if (pc.kind == Piece::kEntropy) printf("ENTROPY");
        else
            for (const char c : pc.bytes) printf("%02x", (unsigned)(uint8_t)c);
        putchar('"');
    }
    printf("]}");
}

}  // namespace

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> d;
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
        fclose(f);
        std::unique_ptr<uint8_t[]> exact(new uint8_t[d.size()]);  // (an empty file: a block of no bytes, every read of it is reported)
        if (!d.empty()) memcpy(exact.get(), d.data(), d.size());
        printf("{\"file\": ");
        print_text(argv[a]);
        printf(", \"runs\": [");
        walk(exact.get(), d.size(), false);
        printf(", ");
        walk(exact.get(), d.size(), true);
        printf("]}\n");
    }
    return 0;
}
