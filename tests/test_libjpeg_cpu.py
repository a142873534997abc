"""The arithmetic policy "libjpeg" without a GPU (include/jpgpu.h, "Arithmetic").

1. tests/islow_model.py IS libjpeg's default decode: on 72 textured files (eight sizes, 4:4:4 / 4:2:2 / 4:2:0, Q25 / 75 / 95) and on their
   progressive versions the model -- jpeg_idct_islow over the oracle's coefficients, upsample_model's triangle filter, libjpeg's four
   colour constants -- equals Pillow's convert("RGB") in every sample, and on grey files its "L".  The same files stay inside the range
   where libjpeg's C code, its SIMD code and 32-bit wrapping arithmetic are one function (asserts_in_range).
2. jpeglibrary_amd/csrc/k3j_islow.h states the same transform: a stand-alone host program over the header transforms those files' blocks and
   10 000 random ones, some of them extreme (+-32767 and -32768 coefficients against 8- and 16-bit tables), and equals the wrapped model
   sample for sample; built once more with the undefined-behaviour sanitizer it runs clean.
3. The C ABI and the Python helpers, as far as they go without a device.
Without Pillow the Pillow cases skip and the rest runs."""
import ctypes
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import islow_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")
SIZES = [(1, 1), (3, 5), (8, 8), (16, 16), (17, 13), (33, 17), (47, 31), (136, 96)]  # (w, h)
SUBSAMPLING = {0: "444", 1: "422", 2: "420"}  # Pillow's subsampling=
QUALITIES = (25, 75, 95)
_FILES = {}


def _have_pillow():
    try:
        import PIL  # noqa: F401
    except ImportError:
        return False
    return True


needs_pillow = pytest.mark.skipif(not _have_pillow(), reason="Pillow is not installed")


def _texture(w, h, channels, seed):
    """smooth gradients, an edge and noise: every AC band carries something"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for c in range(channels):
        a = 128 + 90 * np.sin((xx * (0.11 + 0.05 * c) + yy * (0.07 + 0.03 * c)) + c) + rng.normal(0, 24, (h, w))
        a[(xx + 2 * yy) % 23 < 3] += 70
        out.append(np.clip(a, 0, 255))
    return np.stack(out, axis=-1).astype(np.uint8)


def pillow_file(w, h, subsampling, quality, progressive=False, gray=False):
    from PIL import Image

    key = (w, h, subsampling, quality, progressive, gray)
    if key not in _FILES:
        buf = io.BytesIO()
        if gray:
            Image.fromarray(_texture(w, h, 1, w * 7 + h)[..., 0], "L").save(buf, format="JPEG", quality=quality, progressive=progressive)
        else:
            Image.fromarray(_texture(w, h, 3, w * 7 + h + quality), "RGB").save(buf, format="JPEG", quality=quality, subsampling=subsampling, progressive=progressive)
        _FILES[key] = buf.getvalue()
    return _FILES[key]


CASES = [(w, h, s, q) for (w, h) in SIZES for s in SUBSAMPLING for q in QUALITIES]


# ------------------------------------------------------------------------------------------------ 1: the model is libjpeg's decode

@needs_pillow
@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
@pytest.mark.parametrize("subsampling", list(SUBSAMPLING), ids=list(SUBSAMPLING.values()))
def test_the_model_equals_pillows_rgb_and_stays_in_range(subsampling, progressive):
    n = 0
    for (w, h) in SIZES:
        for q in QUALITIES:
            f = pillow_file(w, h, subsampling, q, progressive)
            assert im.frame(f)[2] == progressive
            want = im.pillow_rgb(f)
            got = im.decode(f, "fancy", transform=im.asserts_in_range)
            assert got.shape == want.shape == (h, w, 3)
            assert np.array_equal(got, want), (w, h, q, int((got != want).sum()))
            assert np.array_equal(im.decode(f, "fancy"), got)  # (the wrapped model is the same function there)
            n += 1
    assert n == 24  # (x 3 samplings = the 72 files)


@needs_pillow
@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
def test_the_model_equals_pillow_on_grey_files(progressive):
    for (w, h) in SIZES:
        for q in (30, 75, 95, 100):
            f = pillow_file(w, h, 0, q, progressive, gray=True)
            s = im.samples(f, im.asserts_in_range)
            assert s.shape == (h, w, 1)
            assert np.array_equal(s[..., 0], im.pillow_l(f)), (w, h, q)
            assert np.array_equal(im.decode(f), im.pillow_rgb(f)), (w, h, q)


@needs_pillow
def test_the_float_transform_and_the_references_constant_are_other_pictures():
    """what the policy is for: the oracle's decode of the same file differs from Pillow's, and so does 22553 in place of 22554"""
    from oracle import pyoracle

    f = pillow_file(136, 96, 0, 75, gray=True)
    ref, _ = pyoracle.decode_8bit(f)
    assert 0 < int((ref[..., 0] != im.pillow_l(f)).sum()) < ref.size // 10
    s = np.zeros((256, 256, 3), np.uint8)  # every (Cb, Cr)
    s[..., 0], s[..., 1], s[..., 2] = 128, np.arange(256)[None, :], np.arange(256)[:, None]
    a, b = im.ycc_rgb(s), pyoracle.ycbcr8_to_rgb(s)
    assert np.array_equal(a[..., 0], b[..., 0]) and np.array_equal(a[..., 2], b[..., 2])
    assert 0 < int((a[..., 1] != b[..., 1]).sum()) < 256  # (green, in a few places)


# ------------------------------------------------------------------------------------------------ 2: the header's transform

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "k3j_islow.h"
using namespace jpgpu;
// in: n records of 64 int16 coefficients (zig-zag) + 64 uint16 quantisers (zig-zag); out: 64 samples per record, row by row
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    struct Record {
        int16_t coef[64];
        uint16_t q[64];
    } rec;
    unsigned long n = 0;
    while (std::fread(&rec, sizeof rec, 1, in) == 1) {
        uint32_t px[16];
        islow_block(reinterpret_cast<const uint8_t *>(rec.coef), 0, rec.q, px);
        uint8_t bytes[64];
        for (int r = 0; r < 8; r++)
            for (int c = 0; c < 8; c++) bytes[r * 8 + c] = (uint8_t)(px[2 * r + (c >> 2)] >> (8 * (c & 3)));
        if (std::fwrite(bytes, 1, 64, out) != 64) return 4;
        n++;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 5;
    std::printf("%lu\n", n);
    return 0;
}
"""


@pytest.fixture(scope="module")
def islow_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / c++) on PATH: the header cannot be run"
    d = tmp_path_factory.mktemp("k3j_islow")
    src = d / "k3j_islow.cpp"
    src.write_text(PROGRAM)
    exes = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover"])):
        exes[name] = str(d / ("k3j_islow_" + name))
        subprocess.check_call([cxx, *flags, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exes[name], str(src)])
    exes["dir"] = d
    return exes


def _random_blocks():
    """10 000 blocks: encoder-like ones, sparse large ones, and the extremes"""
    rng = np.random.default_rng(2026)
    coefs = np.zeros((10000, 64), np.int16)
    quant = np.zeros((10000, 64), np.uint16)
    decay = 1.0 / (1.0 + np.arange(64))
    coefs[:6000] = np.round(rng.normal(0, 300, (6000, 64)) * decay).astype(np.int16)
    quant[:6000] = rng.integers(1, 256, (6000, 64))
    coefs[6000:9000] = rng.integers(-32768, 32768, (3000, 64)) * (rng.random((3000, 64)) < 0.15)
    quant[6000:8000] = rng.integers(1, 256, (2000, 64))
    quant[8000:9000] = rng.integers(1, 65536, (1000, 64))
    ext = rng.choice(np.array([32767, -32767, -32768, 0], np.int16), (1000, 64))
    coefs[9000:] = ext
    coefs[9000], coefs[9001], coefs[9002] = 32767, -32768, np.where(np.arange(64) & 1, -32768, 32767)
    quant[9000:9500] = rng.choice(np.array([1, 2, 255], np.uint16), (500, 64))
    quant[9500:] = rng.choice(np.array([1, 256, 32768, 65535], np.uint16), (500, 64))
    return coefs, quant


def _file_blocks():
    """the coefficient blocks of a few of the 72 files with their tables (all of them where Pillow is there; synthetic files otherwise)"""
    from oracle import pyoracle
    from tools import jpegsynth

    if _have_pillow():
        files = [pillow_file(w, h, s, q) for (w, h, s, q) in CASES]
    else:
        files = [bytes(jpegsynth.encode(w, h, SUBSAMPLING[s], q, 0, seed=w)) for (w, h, s, q) in CASES]
    coefs, quant = [], []
    for f in files:
        blocks, comp = pyoracle.decode_coefficients(f)
        q, comps = im.tables(f), im.frame(f)[3]
        coefs.append(blocks)
        quant.append(np.stack([q[comps[c][3]] for c in comp]))
    return np.concatenate(coefs), np.concatenate(quant)


def _run(exe, d, coefs, quant, tag):
    rec = np.zeros(len(coefs), np.dtype([("coef", "<i2", 64), ("q", "<u2", 64)]))
    rec["coef"], rec["q"] = coefs, quant
    src, dst = str(d / (tag + ".in")), str(d / (tag + ".out"))
    rec.tofile(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == str(len(coefs))
    return np.fromfile(dst, np.uint8).reshape(-1, 8, 8)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_header_equals_the_wrapped_model_sample_for_sample(islow_program, build):
    rc, rq = _random_blocks()
    fc, fq = _file_blocks()
    assert len(fc) > 2000
    coefs, quant = np.concatenate([rc, fc]), np.concatenate([rq, fq])
    got = _run(islow_program[build], islow_program["dir"], coefs, quant, build)
    want = im.islow(coefs, quant)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), int(bad[0]))
    # the extremes do leave the range the equality with libjpeg is claimed for, the files' blocks do not
    with pytest.raises(AssertionError):
        im.asserts_in_range(rc[9000:], rq[9000:])
    im.asserts_in_range(fc, fq)


def test_the_clamp_saturates_where_libjpegs_table_wraps():
    q = np.ones(64, np.uint16)
    for dc, want in ((1023, 255), (-1023, 0), (8 * 200, 255), (-8 * 200, 0), (0, 128), (8, 129)):
        c = np.zeros(64, np.int16)
        c[0] = dc
        assert (im.islow(c, q) == want).all(), dc


# ------------------------------------------------------------------------------------------------ 3: the ABI without a device

def test_the_library_exports_the_policy_and_the_header_states_its_values():
    import jpeglibrary_amd as jl

    lib = jl._capi.lib
    for name in ("jpgpu_batch_set_arithmetic_policy", "jpgpu_batch_image_arithmetic"):
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
        assert any(s[0] == name for s in jl._capi.SYMBOLS), name
    header = open(os.path.join(ROOT, "include", "jpgpu.h")).read()
    values = dict(re.findall(r"\b(JPGPU_ARITHMETIC_[A-Z]+)\s*=\s*(\d+)", header))
    assert values == {"JPGPU_ARITHMETIC_REFERENCE": "0", "JPGPU_ARITHMETIC_LIBJPEG": "1"}
    assert jl._capi.ARITHMETIC_POLICIES == ("reference", "libjpeg")  # (a policy's value is its index)
    for c in (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172, 91881, 46802, 116130, 22554):
        assert re.search(r"\b%d\b" % c, header), c  # the header states the function in full
    assert lib.jpgpu_batch_set_arithmetic_policy(None, 1) == jl._capi.ERR_ARGUMENT  # no batch: refused without a device
    taken = ctypes.c_int(7)
    assert lib.jpgpu_batch_image_arithmetic(None, 0, ctypes.byref(taken)) == jl._capi.ERR_ARGUMENT and taken.value == 7
    assert lib.jpgpu_version() == 101
    assert len([n for n in dir(jl) if n.startswith("FMT_")]) >= 10


@pytest.mark.parametrize("bad", ["islow", 1, None, "LIBJPEG", b"libjpeg"], ids=repr)
def test_the_python_helpers_refuse_a_bad_policy_before_any_library_call(bad):
    import jpeglibrary_amd as jl

    assert [jl.batch._arithmetic_policy(p) for p in ("reference", "libjpeg")] == [0, 1]
    with pytest.raises(ValueError):
        jl.batch._arithmetic_policy(bad)
    b = object.__new__(jl.Batch)  # no context, no handle: a library call would be refused with another exception
    b._h = None
    with pytest.raises(ValueError):
        b.set_arithmetic_policy(bad)
    for helper, args in ((jl.decode_batch, ([b"x"],)), (jl.decode_to_tensors, ([b"x"],)), (jl.decode_resized, ([b"x"], (8, 8)))):
        with pytest.raises(ValueError, match="arithmetic"):
            helper(*args, arithmetic=bad)
