"""The rule of K3's kernel variants (kernels.h: k3_variant), checked without a GPU.  A stand-alone host program prints the rule's answer for
every output format 0..9, layout class 0..5 and form (dense, split, window); the printout is compared with the matrix written out below,
every "no kernel" included, and the set of kernels the matrix reaches with the 82 variants K3 is known to compile.  The launcher instantiates
a kernel exactly where the rule reaches it (k3_idct.hip: launch_k3_variant_if), and test_float_sink_isa_cpu.py compares the names in the
listing with the same enumeration: planner, launcher and compiled set cannot drift apart unnoticed."""
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")
FORMS = ("dense", "split", "window")

PROGRAM = r"""
#include <stdio.h>
#include "kernels.h"
int main() {
    using namespace jpgpu;
    static_assert(kK3Dense == 0 && kK3Split == 1 && kK3Window == 2 && kNumK3Forms == 3, "the forms, in the order the test names them");
    static_assert(kNumOutputFormats == 10 && kNumIdctLayoutClasses == 6 && kNumIdctLayouts == 5 && kIdctClassStoreHoldsSamples == 5, "the matrix");
    for (int form = 0; form < kNumK3Forms; form++)
        for (int f = 0; f < kNumOutputFormats; f++)
            for (int c = 0; c < kNumIdctLayoutClasses; c++) {
                const K3Variant v = k3_variant(f, c, form);
                if (!v.exists) printf("%d %d %d -\n", form, f, c);
                else if (v.pre) printf("%d %d %d pre%d%s\n", form, f, c, v.fmt, v.to_scratch ? "*" : "");
                else printf("%d %d %d %d,%d%s\n", form, f, c, v.fmt, v.lay, v.to_scratch ? "*" : "");
                if (v.exists && !k3_variant_compiled(form, v.pre, v.fmt, v.lay)) return 1;  // (what the rule names is what the launcher instantiates)
                if (v.pre && v.lay != kLayGeneric) return 2;
            }
    // outside the matrix: no kernel
    if (k3_variant(-1, 0, 0).exists || k3_variant(10, 0, 0).exists || k3_variant(0, -1, 0).exists || k3_variant(0, 6, 0).exists || k3_variant(0, 0, 3).exists) return 3;
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def k3_variant_rows():
    """{(form name, format, class): the rule's answer} -- "-" no kernel, "F,L" kernel <F, L> of the form, "preF" its flush kernel <F>, a
    trailing "*": written to the RGB formats' scratch image"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / c++) on PATH: the rule cannot be printed"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "variants.cpp"), os.path.join(tmp, "variants")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-o", exe, src])
        out = subprocess.check_output([exe], text=True)
    rows = {}
    for ln in out.splitlines():
        form, fmt, cls, what = ln.split()
        rows[(FORMS[int(form)], int(fmt), int(cls))] = what
    return rows


def k3_compiled_variants():
    """the kernels the rule reaches: {(kernel name, template arguments)}"""
    names = {("dense", False): "idct_output_kernel", ("split", False): "idct_split_kernel", ("window", False): "idct_window_kernel",
             ("dense", True): "flush_output_kernel", ("window", True): "flush_window_kernel"}
    reached = set()
    for (form, _, _), what in k3_variant_rows().items():
        if what == "-":
            continue
        what = what.rstrip("*")
        pre = what.startswith("pre")
        reached.add((names[(form, pre)], (int(what[3:]),) if pre else tuple(int(v) for v in what.split(","))))
    return reached


NONE6 = ["-"] * 6


def _fast(fmt):
    return ["%d,%d" % (fmt, c) for c in (1, 2, 3, 4)]


# The matrix: per form and format, the answer for classes 0 (generic), 1 (4:4:4), 2 (4:2:2), 3 (4:2:0), 4 (gray), 5 (the store holds samples).
# Formats: 0 INTERLEAVED_U8, 1 PLANAR_U8, 2 PLANAR_I16, 3 RGB_U8, 4 RGBA_U8, 5 EXTENDED_U16 (launched as PLANAR_I16, whose planes
# extend_u16_kernel widens), 6 INTERLEAVED_U8_SCALED, 7 RGB_PLANAR_U8, 8 RGB_PLANAR_F16, 9 RGB_PLANAR_F32.
MATRIX = {
    "dense": {
        0: ["0,0"] + _fast(0) + ["pre0"],
        1: ["1,0"] * 5 + ["pre1"],
        2: ["2,0"] * 5 + ["pre2"],
        3: ["0,0*"] + _fast(3) + ["pre0*"],
        4: ["0,0*"] + _fast(4) + ["pre0*"],
        5: ["2,0"] * 5 + ["pre2"],
        6: ["6,0"] + _fast(6) + ["pre6"],
        7: ["0,0*"] + _fast(7) + ["pre0*"],
        8: ["0,0*"] + _fast(8) + ["pre0*"],
        9: ["0,0*"] + _fast(9) + ["pre0*"],
    },
    "split": {
        0: ["-"] + _fast(0) + ["-"],
        1: ["1,0"] * 5 + ["-"],
        2: ["2,0"] * 5 + ["-"],
        3: ["-", "3,1", "-", "-", "3,4", "-"],
        4: ["-", "4,1", "4,2", "-", "4,4", "-"],
        5: ["2,0"] * 5 + ["-"],
        6: ["-", "6,1", "6,2", "6,3", "-", "-"],
        7: ["-"] + _fast(7) + ["-"],
        8: ["-"] + _fast(8) + ["-"],
        9: ["-"] + _fast(9) + ["-"],
    },
    "window": {
        0: ["0,0", "-", "-", "-", "-", "pre0"],
        1: NONE6,
        2: NONE6,
        3: ["0,0*"] + _fast(3) + ["pre0*"],
        4: ["0,0*", "-", "-", "-", "-", "pre0*"],
        5: NONE6,
        6: ["6,0", "-", "-", "-", "-", "pre6"],
        7: ["0,0*"] + _fast(7) + ["pre0*"],
        8: ["0,0*"] + _fast(8) + ["pre0*"],
        9: ["0,0*"] + _fast(9) + ["pre0*"],
    },
}

# The 82 variants K3 compiles, listed apart from the matrix so that a lost or an extra instantiation shows.
COMPILED = (
    {("idct_output_kernel", (f, c)) for f in (0, 6) for c in range(5)} | {("idct_output_kernel", (f, 0)) for f in (1, 2)}
    | {("idct_output_kernel", (f, c)) for f in (3, 4, 7, 8, 9) for c in (1, 2, 3, 4)}
    | {("idct_split_kernel", (0, c)) for c in (1, 2, 3, 4)} | {("idct_split_kernel", a) for a in ((1, 0), (2, 0), (3, 1), (3, 4), (4, 1), (4, 2), (4, 4))}
    | {("idct_split_kernel", (6, c)) for c in (1, 2, 3)} | {("idct_split_kernel", (f, c)) for f in (7, 8, 9) for c in (1, 2, 3, 4)}
    | {("idct_window_kernel", (0, 0)), ("idct_window_kernel", (6, 0))} | {("idct_window_kernel", (f, c)) for f in (3, 7, 8, 9) for c in (1, 2, 3, 4)}
    | {("flush_output_kernel", (f,)) for f in (0, 1, 2, 6)} | {("flush_window_kernel", (f,)) for f in (0, 6)}
)


def test_the_rule_is_the_matrix():
    rows = k3_variant_rows()
    assert len(rows) == 3 * 10 * 6
    want = {(form, fmt, cls): MATRIX[form][fmt][cls] for form in FORMS for fmt in range(10) for cls in range(6)}
    assert rows == want, {k: (rows.get(k), want[k]) for k in want if rows.get(k) != want[k]}


def test_the_matrix_reaches_exactly_the_82_compiled_variants():
    assert len(COMPILED) == 82
    by_kernel = {name: sum(1 for k, _ in COMPILED if k == name) for name, _ in COMPILED}
    assert by_kernel == {"idct_output_kernel": 32, "idct_split_kernel": 26, "idct_window_kernel": 18, "flush_output_kernel": 4, "flush_window_kernel": 2}
    reached = k3_compiled_variants()
    assert reached == COMPILED, (sorted(reached - COMPILED), sorted(COMPILED - reached))
