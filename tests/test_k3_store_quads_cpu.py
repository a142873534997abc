"""K3 stores the interleaved rows of 4:2:0 / 4:2:2 frames as whole 64-byte blocks per lane quad (jpeglibrary_amd/csrc/k3_store_quads.h).
The header is host + device code: a stand-alone program built with g++ enumerates what the kernel rests on.

  pieces     the twelve (store, lane) entries write every piece 0..11 of the quad's 192 bytes exactly once
  blocks     the four lanes of store s write the four pieces of block s: one aligned 64-byte block of the 192 bytes
  sources    the (lane, register) an entry names holds that piece: piece = 3 * lane + register
  kept       two lanes of every store write a register of their own, the one named like the store (o0 / o1 / o2): two selected moves
  addresses  the packed lane offsets are dst_px - 48 * lane + 16 * piece
  quads      the eligibility rule implies: tasks t .. t + 3 of a tile (t a multiple of 4) are one pixel row of the tile, four MCUs side by
             side in one MCU line of the image, so their 48-byte runs are 192 contiguous bytes -- for every mpl <= 512, n_mcu <= 64 and gx0
             (with the tile's 16 pixel rows of a 4:2:0 MCU, the most of the two layouts), by the index arithmetic of k3_index_math.h
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include "k3_index_math.h"
#include "k3_store_quads.h"
using namespace jpgpu;
static int bad = 0;
static void fail(const char *what, uint32_t a, uint32_t b, uint32_t c) { if (bad++ < 10) std::printf("FAIL %s %u %u %u\n", what, a, b, c); }
int main() {
    uint64_t checked = 0;
    static_assert(kK3QuadStores == 3 && kK3QuadLanes == 4 && kK3QuadPieceBytes == 16, "three 16-byte registers per lane, four lanes");
    int written[12] = {0};
    for (uint32_t s = 0; s < kK3QuadStores; s++) {
        uint32_t in_block = 0, own = 0;
        for (uint32_t lane = 0; lane < kK3QuadLanes; lane++, checked++) {
            const K3QuadMove m = k3_quad_move(s, lane);
            if (m.piece >= 12 || m.src_lane >= 4 || m.src_reg >= 3) { fail("range", s, lane, m.piece); continue; }
            written[m.piece]++;
            if (m.piece / 4 != s) fail("block of the store", s, lane, m.piece);
            in_block |= 1u << (m.piece % 4);
            if (m.piece != 3u * m.src_lane + m.src_reg) fail("source holds the piece", s, lane, m.piece);
            if (m.src_lane == lane) {
                own++;
                if (m.src_reg != s) fail("a kept register is the store's own name", s, lane, m.src_reg);
            }
            // the lane's address: bytes from the start of its own 48, inside the quad's 192, the piece's place
            const int32_t off = (int32_t)k3_quad_lane_offset(k3_quad_offsets_packed(s), lane);
            if (off != 16 * (int32_t)m.piece - 48 * (int32_t)lane) fail("offset", s, lane, (uint32_t)off);
            const int32_t in_quad = 48 * (int32_t)lane + off;
            if (in_quad < 0 || in_quad + 16 > 192 || in_quad / 64 != (int32_t)s || in_quad % 16 != 0) fail("address", s, lane, (uint32_t)in_quad);
            if (k3_quad_lane_offset(k3_quad_offsets_packed(s), lane + 4 * s + 64) != (uint32_t)off) fail("lane of the quad, not of the wave", s, lane, 0);
        }
        if (in_block != 0xFu) fail("the store covers its 64-byte block", s, in_block, 0);
        if (own != 2) fail("two lanes keep their own register", s, own, 0);
    }
    for (uint32_t c = 0; c < 12; c++)
        if (written[c] != 1) fail("every piece once", c, (uint32_t)written[c], 0);

    // eligibility => same pixel row, side by side, no line wrap inside a quad
    for (uint32_t mpl = 1; mpl <= 512; mpl++) {
        const uint32_t line_recip = k3_line_recip(mpl);
        for (uint32_t n_mcu = 1; n_mcu <= 64; n_mcu++) {
            const uint32_t row_recip = k3_row_recip(n_mcu);
            for (uint32_t gx0 = 0; gx0 < mpl; gx0++) {
                if (!k3_quad_eligible(n_mcu, mpl, gx0)) {
                    if (n_mcu % 4 == 0 && mpl % 4 == 0 && gx0 % 4 == 0) fail("eligible by the rule, refused", mpl, n_mcu, gx0);
                    continue;
                }
                if (n_mcu % 4 || mpl % 4 || gx0 % 4) fail("rule", mpl, n_mcu, gx0);
                const uint32_t n_tasks = 16 * n_mcu;
                if (n_tasks % 4) fail("whole quads of tasks", mpl, n_mcu, gx0);
                for (uint32_t t = 0; t < n_tasks; t += 4, checked++) {
                    uint32_t row0 = 0, wraps0 = 0, gx_first = 0;
                    for (uint32_t j = 0; j < 4; j++) {
                        const uint32_t row = k3_task_row(t + j, row_recip), m = t + j - row * n_mcu;
                        const uint32_t x = gx0 + m, wraps = k3_line_wraps(x, mpl, line_recip), gx = x - wraps * mpl;
                        if (j == 0) row0 = row, wraps0 = wraps, gx_first = gx;
                        if (row != row0 || wraps != wraps0) fail("one pixel row, one MCU line", mpl, n_mcu, t + j);
                        if (gx != gx_first + j || gx >= mpl) fail("side by side", mpl, n_mcu, t + j);
                    }
                    if (gx_first % 4) fail("the quad's 192 bytes start at a multiple of 192 in a line that is one", mpl, n_mcu, t);
                }
            }
        }
    }
    std::printf("checked %llu bad %d\n", (unsigned long long)checked, bad);
    return bad != 0;
}
"""


def test_the_quad_table_covers_whole_blocks_and_eligible_quads_are_contiguous(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / c++) on PATH: the enumeration cannot run"
    src = tmp_path / "k3_store_quads.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "k3_store_quads"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad 0" in r.stdout, r.stdout
    assert int(r.stdout.split()[1]) > 1_000_000, r.stdout  # (the loops did run)
