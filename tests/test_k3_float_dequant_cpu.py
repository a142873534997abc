"""K3 dequantises in float with tables prescaled by 1/8 and packs its bytes with a saturating pack, checked without a GPU:

(a) a numpy float32 model of the two orders of operations -- the reference's (float)(q * c), two butterfly passes, * 0.125 against
    (float)c * ((float)q * 0.125), the same passes, no closing multiplication -- gives the same bits, the sign of zero included;
(b) the pair order the host writes DevQuantTable::qf in (k3_quant_order.h, a stand-alone program built with g++) against kNat;
(c) the listing of the two headline kernels: what the change took out stays out."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")

# JpegZigZag.cs:27-38: natural position of zig-zag index k
NAT = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50,
       43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def test_the_kernel_s_zig_zag_table_is_the_one_this_file_checks_against():
    text = open(os.path.join(CSRC, "k3_idct.hip")).read()
    m = re.search(r"kNat\[64\]\s*=\s*\{([^}]*)\}", text)
    assert [int(v) for v in m.group(1).split(",")] == NAT


# ------------------------------------------------------------------------------------------------ (a) the float32 model

F = np.float32


def _idct8(y):
    """idct8 of k3_idct.hip on float32 arrays: y[0..7], every operation one IEEE rounding, order and parentheses as there"""
    y0, y1, y2, y3, y4, y5, y6, y7 = y
    mz0, mz2, mz1, mz3 = y1 + y7, y3 + y7, y3 + y5, y1 + y5
    mz4 = (mz0 + mz1) * F(1.175875602)
    mz2 = (mz2 * F(-1.961570560)) + mz4
    mz3 = (mz3 * F(-0.390180644)) + mz4
    mz0 = mz0 * F(-0.899976223)
    mz1 = mz1 * F(-2.562915447)
    mb3 = ((y7 * F(0.298631336)) + mz0) + mz2
    mb2 = ((y5 * F(2.053119869)) + mz1) + mz3
    mb1 = ((y3 * F(3.072711026)) + mz1) + mz2
    mb0 = ((y1 * F(1.501321110)) + mz0) + mz3
    mz4 = (y2 + y6) * F(0.541196100)
    mz0, mz1 = y0 + y4, y0 - y4
    mz2 = mz4 + (y6 * F(-1.847759065))
    mz3 = mz4 + (y2 * F(0.765366865))
    a0, a3, a1, a2 = mz0 + mz3, mz0 - mz3, mz1 + mz2, mz1 - mz2
    return [a0 + mb0, a1 + mb1, a2 + mb2, a3 + mb3, a3 - mb3, a2 - mb2, a1 - mb1, a0 - mb0]


def _two_passes(f):
    """f: float32[n, 8, 8] in natural order -> the transform's results in front of the rounding: rows first, then columns"""
    a = np.stack(_idct8([f[:, :, c] for c in range(8)]), axis=2)
    return np.stack(_idct8([a[:, r, :] for r in range(8)]), axis=1)


def _both_forms(z, q):
    """z: int16[n, 64], q: uint16[64], both zig-zag -> (the reference's order, the kernel's), float32[n, 8, 8] each"""
    nat = np.array(NAT)
    prod = z.astype(np.int32) * q.astype(np.int32)[None, :]  # ushort * short -> int
    f_ref = np.zeros((len(z), 64), F)
    f_ref[:, nat] = prod.astype(F)
    ref = _two_passes(f_ref.reshape(-1, 8, 8)) * F(0.125)
    qf = q.astype(F) * F(0.125)
    f_new = np.zeros((len(z), 64), F)
    f_new[:, nat] = z.astype(F) * qf[None, :]
    return ref, _two_passes(f_new.reshape(-1, 8, 8))


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


N_BLOCKS = 200_000


@pytest.mark.parametrize("regime", ["sparse_8bit", "dense_8bit", "sparse_16bit", "dense_16bit"])
def test_prescaled_float_dequantisation_gives_the_reference_s_bits(regime):
    rng = np.random.default_rng({"sparse_8bit": 1, "dense_8bit": 2, "sparse_16bit": 3, "dense_16bit": 4}[regime])
    wide = regime.endswith("16bit")
    q = rng.integers(1, 65536 if wide else 256, 64).astype(np.uint16)
    if wide:
        q[rng.integers(0, 64, 8)] = 65535
    z = rng.integers(-32768, 32768, (N_BLOCKS, 64)).astype(np.int16)
    if regime.startswith("sparse"):
        z[rng.random(z.shape) < 0.9] = 0
        z[:, 0] = rng.integers(-1024, 1024, N_BLOCKS)
    else:
        z[: N_BLOCKS // 2] >>= 8  # half of them moderate, half the full int16 range
    z[rng.random(z.shape) < 0.01] = -32768
    ref, new = _both_forms(z, q)
    assert np.isfinite(ref).all()
    assert _same_bits(ref, new), int((ref.view(np.uint32) != new.view(np.uint32)).sum())


def test_the_corner_product_at_every_position():
    """q = 65535, c = -32768 (and 32767) alone at each of the 64 positions, and all 64 at once"""
    q = np.full(64, 65535, np.uint16)
    z = np.zeros((2 * 64 + 2, 64), np.int16)
    for k in range(64):
        z[k, k], z[64 + k, k] = -32768, 32767
    z[128], z[129] = -32768, 32767
    ref, new = _both_forms(z, q)
    assert _same_bits(ref, new)
    assert (ref[:, 0, 0] != 0).all()


def test_a_zero_quantiser_only_changes_the_sign_of_a_zero():
    """q = 0 is not a table an encoder writes, but the parser takes it: (float)(0 * c) is +0 where (float)c * 0.0f is -0 for c < 0.
    Every sample is still the same integer: the zeros differ in sign alone, and the conversion behind the rounding drops it."""
    rng = np.random.default_rng(5)
    q = rng.integers(0, 4, 64).astype(np.uint16)
    z = rng.integers(-300, 300, (20_000, 64)).astype(np.int16)
    ref, new = _both_forms(z, q)
    assert np.array_equal(np.rint(ref).astype(np.int32), np.rint(new).astype(np.int32))
    assert np.array_equal(ref, new)  # (equal as numbers: -0 == +0)


# ------------------------------------------------------------------------------------------------ (b) the pair order

PROGRAM = r"""
#include <stdio.h>
#include "k3_quant_order.h"
int main() {
    uint16_t q[64];
    float qf[64];
    for (int t = 0; t < 2; t++) {
        for (int k = 0; k < 64; k++) q[k] = (uint16_t)(t == 0 ? k + 1 : 65535 - 1000 * k);
        jpgpu::k3_quant_pair_floats(q, qf);
        for (int e = 0; e < 64; e++) printf("%a\n", qf[e]);
    }
    return 0;
}
"""


def test_the_host_writes_the_float_table_in_pair_order(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / c++) on PATH: the order cannot be checked"
    src, exe = tmp_path / "order.cpp", tmp_path / "order"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    got = [float.fromhex(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert len(got) == 128
    zig_of_nat = {n: k for k, n in enumerate(NAT)}
    for t, q in enumerate(([k + 1 for k in range(64)], [65535 - 1000 * k for k in range(64)])):
        for r2 in range(4):
            for c in range(8):
                for h in range(2):
                    nat = (2 * r2 + h) * 8 + c
                    assert got[t * 64 + 2 * (r2 * 8 + c) + h] == q[zig_of_nat[nat]] / 8.0, (t, r2, c, h)


def test_the_device_table_holds_both_forms_and_the_kernel_copies_the_floats():
    common = open(os.path.join(CSRC, "common.h")).read()
    m = re.search(r"struct alignas\(16\) DevQuantTable \{(.*?)\};", common, re.S)
    assert re.search(r"uint16_t q\[64\];\s*float qf\[64\];", m.group(1))
    layout = open(os.path.join(CSRC, "device_batch_layout.cpp")).read()
    assert "k3_quant_pair_floats(d.q, d.qf)" in layout


# ------------------------------------------------------------------------------------------------ (c) the listing

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "k3_idct.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, "k3_idct.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


def _body(text, mangled_prefix):
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = [ln.strip() for ln in lines[start:end] if ln.strip() and not ln.strip().startswith(";")]
    return [ln for ln in body if not ln.split(";")[0].strip().endswith(":") and not ln.startswith(".")]


def _resources(text):
    names = re.findall(r"\.name:\s+(\S+)", text)
    out = {n: {} for n in names}
    for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size"):
        values = re.findall(r"\.%s:\s+(\d+)" % key, text)
        assert len(values) == len(names), key
        for n, v in zip(names, values):
            out[n][key] = int(v)
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kernel", ["_ZN5jpgpu17idct_split_kernelILi0ELi3EEE", "_ZN5jpgpu18idct_output_kernelILi0ELi3EEE"], ids=["split", "dense"])
def test_the_headline_kernels_dequantise_in_float_and_pack_saturating(isa, kernel):
    body = _body(isa, kernel)
    ops = [ln.split()[0] for ln in body]
    starts = lambda prefix: sum(1 for o in ops if o.startswith(prefix))
    assert starts("v_mul_i32_i24") == 0          # no integer product per coefficient
    assert starts("v_cvt_f32_i32") == 64         # one conversion per coefficient (sign-extending word select)
    assert starts("v_sat_pk_u8_i16") == 32       # clamp + pack of a sample pair in one
    assert starts("v_pk_max_i16") == 0 and starts("v_pk_min_i16") == 0
    valu = sum(1 for o in ops if o.startswith("v_"))
    assert valu <= 1990, valu
    moves = sum(1 for o in ops if re.sub(r"_(e32|e64|sdwa|dpp)$", "", o) == "v_mov_b32")
    assert moves <= 300, moves
    (name,) = [n for n in _resources(isa) if n.startswith(kernel)]
    r = _resources(isa)[name]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["vgpr_count"] <= 168, r


@pytest.mark.timeout(600)
def test_no_kernel_of_the_file_spills_or_uses_scratch(isa):
    res = _resources(isa)
    assert len(res) >= 80
    for n, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
