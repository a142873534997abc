"""K3's tile loop divides by multiplying (jpeglibrary_amd/csrc/k3_index_math.h).  The helpers are host + device code: a stand-alone
program built with g++ enumerates every claim the kernel rests on against / and %:

  rows       t / n_mcu for every n_mcu = 1..85 and every t < 16 * n_mcu (16 pixel rows of a 4:2:0 MCU: the most of the three fast layouts)
  lines      the wraps of x over a line of mpl MCUs, for every mpl below the threshold and every x < mpl + 256 (the tile's MCUs + its first
             one's column; the issue's x < mpl + 85 is inside), and on either side of the threshold the compare
  operands   every multiply has both operands below 2^24 and a product below 2^32 (what v_mul_u32_u24 computes)
  walk       the (gx0, gy0) carried from tile to tile by addition and one wrap, from every first MCU of a 7 x 5 and a 300 x 3 MCU grid,
             for tiles of 40, 42, 64 and 85 MCUs
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "k3_index_math.h"
using namespace jpgpu;
static int bad = 0;
static void fail(const char *what, uint32_t a, uint32_t b) { if (bad++ < 10) std::printf("FAIL %s %u %u\n", what, a, b); }
static bool fits24(uint32_t a, uint32_t b) { return a < (1u << 24) && b < (1u << 24) && (uint64_t)a * b < (1ull << 32); }
int main() {
    uint64_t checked = 0;
    for (uint32_t n = 1; n <= kK3MaxTileMcus; n++) {
        const uint32_t r = k3_row_recip(n);
        for (uint32_t t = 0; t < 16 * n; t++, checked++) {
            if (!fits24(t, r)) fail("row operands", n, t);
            const uint32_t row = k3_task_row(t, r);
            if (row != t / n) fail("row", n, t);
            if (!fits24(row, n) || t - k3_mul24(row, n) != t % n) fail("mcu of the task", n, t);
        }
    }
    static_assert(kK3MaxTileMcus == 85 && kK3MaxTileLanes == 256, "the ranges this program enumerates");
    for (uint32_t mpl = 1; mpl < kK3LineRecipBelow + 600; mpl++) {  // (below the threshold the reciprocal, from it on the compare)
        const uint32_t r = k3_line_recip(mpl);
        for (uint32_t x = 0; x < mpl + kK3MaxTileLanes; x++, checked++) {
            if (!fits24(x, r)) fail("line operands", mpl, x);
            const uint32_t w = k3_line_wraps(x, mpl, r);
            if (w != x / mpl) fail("wraps", mpl, x);
            if (!fits24(w, mpl) || x - k3_mul24(w, mpl) != x % mpl) fail("column", mpl, x);
        }
    }
    for (uint32_t mpl : {4095u, 4096u, 8191u, 8192u})  // (the widest frames: 65 535 samples are 8 192 MCUs of 8)
        for (uint32_t x = 0; x < mpl + kK3MaxTileLanes; x++, checked++)
            if (k3_line_wraps(x, mpl, k3_line_recip(mpl)) != x / mpl) fail("wraps, wide", mpl, x);
    const uint32_t grids[2][2] = {{7, 5}, {300, 3}};
    for (auto &g : grids)
        for (uint32_t tile : {40u, 42u, 64u, 85u})
            for (uint32_t first = 0; first < g[0] * g[1]; first++) {
                K3TilePos p = k3_tile_pos(first, g[0]);
                const K3TilePos step = k3_tile_pos(tile, g[0]);
                if (p.gx0 != first % g[0] || p.gy0 != first / g[0]) fail("first", first, g[0]);
                for (uint32_t at = first; at < g[0] * g[1]; at += tile, checked++) {
                    if (p.gx0 != at % g[0] || p.gy0 != at / g[0]) fail("walk", first, at);
                    k3_tile_advance(p, step, g[0]);
                }
            }
    std::printf("checked %llu bad %d\n", (unsigned long long)checked, bad);
    return bad != 0;
}
"""


def test_the_reciprocals_and_the_tile_walk_agree_with_division(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / c++) on PATH: the enumeration cannot run"
    src = tmp_path / "k3_index_math.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "k3_index_math"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad 0" in r.stdout, r.stdout
    assert int(r.stdout.split()[1]) > 500_000, r.stdout  # (the loops did run)
