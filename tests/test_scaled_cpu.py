"""The scaled decode without a GPU (include/jpgpu.h, "Scaled decode").

1. tests/scaled_model.py IS libjpeg's scaled decode: on grey, 4:4:4, 4:2:2 and 4:2:0 files of eight sizes, Q50 / Q90, baseline and
   progressive, at 1/2, 1/4 and 1/8 the model -- jidctred.c's transforms over the oracle's coefficients, jdmaster.c's size per component,
   upsample_model's triangle filter on the residual ratio, libjpeg's colour constants -- equals Pillow's draft() decode in every sample, as
   "L", as "YCbCr" and as convert("RGB"); so does a 4:4:0 file.  The same files stay inside the range where libjpeg's C code, its SIMD code
   and 32-bit wrapping arithmetic are one function (asserts_in_range).
2. jdmaster's table for the layouts the GPU tests use.
3. jpeglibrary_amd/csrc/k3r_reduced.h states the same transforms: a stand-alone host program over the header transforms those files' blocks
   and 10 000 random ones up to +-32767 against 16-bit tables at s = 4, 2 and 1, and equals the wrapped model sample for sample; built once
   more with the undefined-behaviour and address sanitizers it runs clean.
4. The C ABI and the Python helpers, as far as they go without a device.
Without Pillow the Pillow cases skip and the rest runs."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import islow_model as im
import scaled_model as sm
import upsample_model as um
from test_libjpeg_cpu import _have_pillow, _random_blocks, needs_pillow, pillow_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")
SIZES = [(8, 8), (9, 9), (16, 16), (17, 31), (33, 40), (64, 48), (100, 75), (131, 67)]  # (w, h)
SUBSAMPLING = {0: "444", 1: "422", 2: "420"}  # Pillow's subsampling=
QUALITIES = (50, 90)


# ------------------------------------------------------------------------------------------------ 1: the model is libjpeg's scaled decode

@needs_pillow
@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
@pytest.mark.parametrize("subsampling", list(SUBSAMPLING), ids=list(SUBSAMPLING.values()))
def test_the_model_equals_pillows_draft_decode_and_stays_in_range(subsampling, progressive):
    n = 0
    for (w, h) in SIZES:
        for q in QUALITIES:
            f = pillow_file(w, h, subsampling, q, progressive)
            assert im.frame(f)[2] == progressive
            for denom in sm.DENOMS:
                what = (w, h, q, denom)
                ycc = sm.ycc(f, denom, "fancy", check=True)
                assert ycc.shape == sm.out_size(w, h, denom)[::-1] + (3,), what
                want = sm.pillow_draft(f, denom, "YCbCr")
                assert np.array_equal(ycc, want), (what, int((ycc != want).sum()))
                rgb, want = sm.decode(f, denom, "fancy"), sm.pillow_draft(f, denom, "RGB")
                assert np.array_equal(rgb, want), (what, int((rgb != want).sum()))
                assert np.array_equal(rgb, im.ycc_rgb(ycc))
                n += 1
    assert n == 48  # (eight sizes, two qualities, three scales; x 3 samplings x 2 kinds of file, and the grey files below)


@needs_pillow
@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
def test_the_model_equals_pillow_on_grey_files(progressive):
    for (w, h) in SIZES:
        for q in QUALITIES:
            f = pillow_file(w, h, 0, q, progressive, gray=True)
            for denom in sm.DENOMS:
                s = sm.samples(f, denom, check=True)
                assert s.shape == sm.out_size(w, h, denom)[::-1] + (1,)
                assert np.array_equal(s[..., 0], sm.pillow_draft(f, denom, "L")), (w, h, q, denom)
                assert np.array_equal(sm.decode(f, denom), sm.pillow_draft(f, denom, "RGB")), (w, h, q, denom)


@needs_pillow
def test_a_440_file():
    """a 4:2:2 file of one MCU per line with its frame header patched: (Y, Y, Cb, Cr) per MCU either way"""
    for q in QUALITIES:
        f = um.patch_sof(pillow_file(16, 24, 1, q), width=8, height=48, luma=0x12)
        assert um.ratio(f) == (1, 2)
        for denom in sm.DENOMS:
            assert sm.residual_ratio(f, denom) == (1, 2) and sm.filters(f, denom) == (denom < 8)
            ycc, want = sm.ycc(f, denom, "fancy", check=True), sm.pillow_draft(f, denom, "YCbCr")
            assert np.array_equal(ycc, want), (q, denom, int((ycc != want).sum()))
            assert np.array_equal(sm.decode(f, denom, "fancy"), sm.pillow_draft(f, denom, "RGB")), (q, denom)


@needs_pillow
def test_the_scale_1_transform_and_a_replicated_picture_are_other_pictures():
    """what the transforms are for: neither every m-th sample of the full decode nor the unfiltered 4:2:2 picture is Pillow's draft()"""
    f = pillow_file(131, 67, 1, 90)
    full = im.samples(f)
    for denom in (2, 4):
        assert not np.array_equal(full[::denom, ::denom], sm.samples(f, denom))
        assert not np.array_equal(sm.ycc(f, denom, "replicate"), sm.pillow_draft(f, denom, "YCbCr"))
    assert np.array_equal(sm.ycc(f, 8, "replicate"), sm.pillow_draft(f, 8, "YCbCr"))  # (libjpeg switches the filter off)


# ------------------------------------------------------------------------------------------------ 2: jdmaster's rule

def test_jdmasters_table():
    # layout -> {denom: [(s, rh, rv) of luma, of chroma]}
    table = {
        ((1, 1), (1, 1)): {2: [(4, 1, 1), (4, 1, 1)], 4: [(2, 1, 1), (2, 1, 1)], 8: [(1, 1, 1), (1, 1, 1)]},
        ((2, 1), (1, 1)): {2: [(4, 1, 1), (4, 2, 1)], 4: [(2, 1, 1), (2, 2, 1)], 8: [(1, 1, 1), (1, 2, 1)]},
        ((2, 2), (1, 1)): {2: [(4, 1, 1), (8, 1, 1)], 4: [(2, 1, 1), (4, 1, 1)], 8: [(1, 1, 1), (2, 1, 1)]},
        ((1, 2), (1, 1)): {2: [(4, 1, 1), (4, 1, 2)], 4: [(2, 1, 1), (2, 1, 2)], 8: [(1, 1, 1), (1, 1, 2)]},
        ((4, 1), (1, 1)): {2: [(4, 1, 1), (4, 4, 1)], 4: [(2, 1, 1), (2, 4, 1)], 8: [(1, 1, 1), (1, 4, 1)]},
    }
    for (luma, chroma), by_denom in table.items():
        for denom, want in by_denom.items():
            got = sm.component_sizes(8 // denom, [luma, chroma, chroma])
            assert got == [want[0], want[1], want[1]], (luma, denom, got)
            for (s, rh, rv), (h, v) in zip(got, (luma, chroma, chroma)):  # every component covers the reduced MCU exactly
                assert (h * s * rh, v * s * rv) == (luma[0] * 8 // denom, luma[1] * 8 // denom)
    for denom in sm.DENOMS:
        assert sm.component_sizes(8 // denom, [(1, 1)]) == [(8 // denom, 1, 1)]  # grey
    assert sm.out_size(131, 67, 2) == (66, 34) and sm.out_size(131, 67, 4) == (33, 17) and sm.out_size(131, 67, 8) == (17, 9)
    assert sm.out_size(1, 1, 8) == (1, 1) and sm.out_size(8, 8, 8) == (1, 1) and sm.out_size(9, 9, 8) == (2, 2)


# ------------------------------------------------------------------------------------------------ 3: the header's transforms

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "k3r_reduced.h"
using namespace jpgpu;
// argv: in out s.  in: n records of 64 int16 coefficients (zig-zag) + 64 uint16 quantisers (zig-zag); out: s * s samples per record, row by
// row.  The records are read from the heap at their exact size so that the address sanitizer sees every byte the header touches.
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const uint32_t s = (uint32_t)std::atoi(argv[3]);
    if (s != 1 && s != 2 && s != 4 && s != 8) return 2;
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    unsigned long n = 0;
    for (;;) {
        std::vector<int16_t> coef(64);
        std::vector<uint16_t> q(64);
        if (std::fread(coef.data(), 2, 64, in) != 64 || std::fread(q.data(), 2, 64, in) != 64) break;
        uint32_t px[16] = {0};
        reduced_block(s, reinterpret_cast<const uint8_t *>(coef.data()), 0, q.data(), px);
        std::vector<uint8_t> bytes(s * s);
        for (uint32_t r = 0; r < s; r++)
            for (uint32_t c = 0; c < s; c++) bytes[r * s + c] = (uint8_t)(px[2 * r + (c >> 2)] >> (8 * (c & 3)));
        if (std::fwrite(bytes.data(), 1, s * s, out) != s * s) return 4;
        n++;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 5;
    // the per-component rule, for the table test: "m h v hmax vmax -> s rh rv"
    for (uint32_t m = 1; m <= 4; m *= 2)
        for (uint32_t hmax = 1; hmax <= 4; hmax *= 2)
            for (uint32_t vmax = 1; vmax <= 4; vmax *= 2)
                for (uint32_t h = 1; h <= hmax; h *= 2)
                    for (uint32_t v = 1; v <= vmax; v *= 2) {
                        const uint32_t bs = reduced_block_size(m, h, v, hmax, vmax);
                        std::printf("%u %u %u %u %u %u %u %u\n", m, h, v, hmax, vmax, bs, reduced_replication(m, bs, h, hmax), reduced_replication(m, bs, v, vmax));
                    }
    std::printf("%lu\n", n);
    return 0;
}
"""


@pytest.fixture(scope="module")
def reduced_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / c++) on PATH: the header cannot be run"
    d = tmp_path_factory.mktemp("k3r_reduced")
    src = d / "k3r_reduced.cpp"
    src.write_text(PROGRAM)
    exes = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover"])):
        exes[name] = str(d / ("k3r_reduced_" + name))
        subprocess.check_call([cxx, *flags, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exes[name], str(src)])
    exes["dir"] = d
    return exes


def _file_blocks():
    """the coefficient blocks of the model's files with their tables (synthetic files without Pillow)"""
    from oracle import pyoracle
    from tools import jpegsynth

    cases = [(w, h, s, q) for (w, h) in SIZES for s in SUBSAMPLING for q in QUALITIES]
    if _have_pillow():
        files = [pillow_file(w, h, s, q) for (w, h, s, q) in cases]
    else:
        files = [bytes(jpegsynth.encode(w, h, SUBSAMPLING[s], q, 0, seed=w)) for (w, h, s, q) in cases]
    coefs, quant = [], []
    for f in files:
        blocks, comp = pyoracle.decode_coefficients(f)
        q, comps = im.tables(f), im.frame(f)[3]
        coefs.append(blocks)
        quant.append(np.stack([q[comps[c][3]] for c in comp]))
    return np.concatenate(coefs), np.concatenate(quant)


def _run(exe, d, coefs, quant, s, tag):
    rec = np.zeros(len(coefs), np.dtype([("coef", "<i2", 64), ("q", "<u2", 64)]))
    rec["coef"], rec["q"] = coefs, quant
    src, dst = str(d / ("%s_%d.in" % (tag, s))), str(d / ("%s_%d.out" % (tag, s)))
    rec.tofile(src)
    r = subprocess.run([exe, src, dst, str(s)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == str(len(coefs))
    return np.fromfile(dst, np.uint8).reshape(-1, s, s), [tuple(int(v) for v in line.split()) for line in lines[:-1]]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_header_equals_the_wrapped_model_sample_for_sample(reduced_program, build):
    rc, rq = _random_blocks()
    rq = rq.copy()
    rq[:3000] = np.random.default_rng(7).integers(1, 65536, (3000, 64))  # (16-bit tables under encoder-like blocks as well)
    fc, fq = _file_blocks()
    assert len(fc) > 2000
    coefs, quant = np.concatenate([rc, fc]), np.concatenate([rq, fq])
    for s in (4, 2, 1, 8):
        got, rule = _run(reduced_program[build], reduced_program["dir"], coefs, quant, s, build)
        want = sm.reduced(coefs, quant, s)
        assert got.shape == want.shape
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        assert len(bad) == 0, (s, len(bad), int(bad[0]))
        sm.asserts_in_range(fc, fq, s)  # the files' blocks stay inside the range the equality with libjpeg is claimed for
    with pytest.raises(AssertionError):
        sm.asserts_in_range(rc[9000:], rq[9000:], 4)  # ... the extremes do not
    assert len(rule) > 50
    for m, h, v, hmax, vmax, bs, rh, rv in rule:  # the header's rule is the model's
        assert bs == sm.block_size(m, h, v, hmax, vmax) and (rh, rv) == (hmax * m // (h * bs), vmax * m // (v * bs)), (m, h, v, hmax, vmax)


def test_a_flat_block_is_its_dc_at_every_size():
    q = np.ones(64, np.uint16)
    for dc, want in ((1023, 255), (-1023, 0), (8 * 200, 255), (-8 * 200, 0), (0, 128), (8, 129), (4, 129), (3, 128), (-4, 128), (-5, 127)):
        c = np.zeros(64, np.int16)
        c[0] = dc
        for s in (1, 2, 4, 8):
            assert (sm.reduced(c, q, s) == want).all(), (dc, s)


# ------------------------------------------------------------------------------------------------ 4: the ABI without a device

def test_the_library_exports_the_three_entries_and_the_header_states_the_function():
    import jpeglibrary_amd as jl

    lib = jl._capi.lib
    for name in ("jpgpu_batch_set_scale_policy", "jpgpu_batch_set_scale_fit", "jpgpu_batch_image_scale"):
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
        assert any(s[0] == name for s in jl._capi.SYMBOLS), name
    header = open(os.path.join(ROOT, "include", "jpgpu.h")).read()
    assert "Scaled decode" in header
    for c in (15137, 6270, 1730, 11893, 17799, 8697, 4176, 4926, 7373, 20995, 5906, 6967, 10426, 29692):
        assert re.search(r"\b%d\b" % c, header), c  # the header states the function in full
    assert lib.jpgpu_batch_set_scale_policy(None, 2) == jl._capi.ERR_ARGUMENT  # no batch: refused without a device
    assert lib.jpgpu_batch_set_scale_fit(None, 8, 8) == jl._capi.ERR_ARGUMENT
    denom = ctypes.c_int(7)
    assert lib.jpgpu_batch_image_scale(None, 0, ctypes.byref(denom)) == jl._capi.ERR_ARGUMENT and denom.value == 7
    assert lib.jpgpu_version() == 101
    assert jl._capi.SCALE_DENOMINATORS == (1, 2, 4, 8)
    # the public structs are what they were
    C = ctypes
    assert (lib.jpgpu_sizeof_image_result(), lib.jpgpu_sizeof_plan_stats(), lib.jpgpu_sizeof_rect(), lib.jpgpu_sizeof_progressive_plan(),
            lib.jpgpu_sizeof_device_ingest_stats()) == (C.sizeof(jl._capi.ImageResult), C.sizeof(jl._capi.PlanStats), C.sizeof(jl._capi.Rect),
                                                        C.sizeof(jl._capi.ProgressivePlan), C.sizeof(jl._capi.DeviceIngestStats))
    assert C.sizeof(jl._capi.Rect) == 16


def _no_library_batch():
    import jpeglibrary_amd as jl

    b = object.__new__(jl.Batch)  # no context, no handle: a library call would be refused with another exception
    b._h = None
    return b


@pytest.mark.parametrize("bad", [3, 0, 16, -2, "2", None, 2.0, True, "fit"], ids=repr)
def test_the_python_helpers_refuse_a_bad_scale_before_any_library_call(bad):
    import jpeglibrary_amd as jl

    with pytest.raises(ValueError):
        _no_library_batch().set_scale_policy(bad)
    with pytest.raises(ValueError, match="scale"):
        jl.decode_to_tensors([b"x"], arithmetic="libjpeg", scale=bad)
    if bad != "fit":
        with pytest.raises(ValueError, match="scale"):
            jl.decode_resized([b"x"], (8, 8), arithmetic="libjpeg", scale=bad)


def test_a_scale_needs_libjpegs_arithmetic_and_fit_takes_no_windows():
    import jpeglibrary_amd as jl

    for scale in (2, 4, 8):
        with pytest.raises(ValueError, match="libjpeg"):
            jl.decode_to_tensors([b"x"], scale=scale)
        with pytest.raises(ValueError, match="libjpeg"):
            jl.decode_to_tensors([b"x"], arithmetic="reference", scale=scale)
        with pytest.raises(ValueError, match="libjpeg"):
            jl.decode_resized([b"x"], (8, 8), arithmetic="reference", scale=scale)
    with pytest.raises(ValueError, match="libjpeg"):
        jl.decode_resized([b"x"], (8, 8), scale="fit")
    with pytest.raises(ValueError, match="windows"):
        jl.decode_resized([b"x"], (8, 8), arithmetic="libjpeg", scale="fit", windows=[(0, 0, 4, 4)])
    for bad in ((0, 8), (8,), 8, "8x8", (8.0, 8), (-1, 4)):
        with pytest.raises(ValueError):
            _no_library_batch().set_scale_fit(bad)
