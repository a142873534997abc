"""The upsampling policy "fancy" without a GPU (include/jpgpu.h, "Chroma upsampling").

1. tests/upsample_model.py IS libjpeg's fancy upsampler: YCbCr pictures whose luma and chroma are constant per native 8 x 8 block go through
   Pillow in mode YCbCr at quality 100 (every DCT block is a DC term, every IDCT exact), come back through draft("YCbCr"), and equal the model
   applied to the known native planes -- 4:2:0 and 4:2:2 as Pillow writes them, 4:4:0 from a 4:2:2 file whose frame header is patched.
   Replication does not equal them wherever the chroma plane has more than one block.
2. The taps clamp to the REAL extent of the chroma plane, not to the MCU padding, and planes of one or two samples' width are replicated:
   frame headers patched to smaller sizes over chroma ramps.
3. jpeglibrary_amd/csrc/k3u_taps.h states the same arithmetic: a stand-alone host program over the header prints the fetch rectangle of
   every window and the taps of every pixel, the printout is compared with the model, every tap lies inside its fetch rectangle, and the
   program runs clean under the address and undefined-behaviour sanitizers.
4. The C ABI and the Python helpers, as far as they go without a device."""
import ctypes
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import upsample_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")
SIZES = [(16, 16), (17, 17), (45, 67), (64, 48), (33, 31), (100, 75), (5, 5), (6, 3)]  # (w, h)
SUBSAMPLING = {2: (2, 2), 1: (2, 1)}  # Pillow's subsampling= -> (hs, vs)


def _save(ycc, subsampling):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(ycc, "YCbCr").save(buf, format="JPEG", quality=100, subsampling=subsampling)
    return buf.getvalue()


def _read(f):
    """Pillow's decode without the colour conversion: (Y, Cb', Cr') as libjpeg upsamples them"""
    from PIL import Image

    im = Image.open(io.BytesIO(f))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    return np.asarray(im)


def _blocks(rng, h, w):
    """uint8[h, w], constant per 8 x 8 block"""
    return rng.integers(16, 240, ((h + 7) // 8, (w + 7) // 8)).astype(np.uint8)[np.arange(h) // 8][:, np.arange(w) // 8]


def _block_picture(w, h, hs, vs, seed):
    """-> the full-size YCbCr picture, its native chroma planes [Cb, Cr] and its luma"""
    rng = np.random.default_rng(seed)
    C = [_blocks(rng, um.chroma_extent(h, vs), um.chroma_extent(w, hs)) for _ in range(2)]
    L = _blocks(rng, h, w)
    return np.stack([L] + [um.replicate(c, hs, vs, w, h) for c in C], axis=-1), C, L


def _ramp_picture(w, h, hs, vs):
    """chroma ramps (not constant inside a block: what lies in the padding differs from the edge sample), luma constant per block"""
    jj, ii = np.mgrid[0:h // vs, 0:w // hs]
    C = [(60 + 4 * ii + 2 * jj).astype(np.uint8), (195 - 4 * ii - 2 * jj).astype(np.uint8)]
    yy, xx = np.mgrid[0:h, 0:w]
    L = (((xx // 8) * 37 + (yy // 8) * 91) % 200 + 20).astype(np.uint8)
    return np.stack([L] + [um.replicate(c, hs, vs, w, h) for c in C], axis=-1), C, L


# ------------------------------------------------------------------------------------------------ 1: the model is libjpeg's upsampler

@pytest.mark.parametrize("subsampling", [2, 1], ids=["420", "422"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_the_model_equals_pillow_on_block_constant_pictures(size, subsampling):
    (w, h), (hs, vs) = size, SUBSAMPLING[subsampling]
    full, C, L = _block_picture(w, h, hs, vs, w * 100 + h)
    f = _save(full, subsampling)
    assert um.ratio(f) == (hs, vs) and um.qualifies(f) == (um.chroma_extent(w, 2) > 2)
    got = _read(f)
    want = np.stack([L] + [um.upsample(c, hs, vs, w, h) for c in C], axis=-1)
    assert np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())
    assert np.array_equal(um.filtered(full, hs, vs), want)  # (the native samples read back from the replicated picture: the policy's definition)
    if (hs == 2 and um.chroma_extent(w, 2) > 8) or (vs == 2 and um.chroma_extent(h, 2) > 8):  # more than one chroma block along a filtered axis: replication is another picture
        assert np.abs(got.astype(int) - full).max() >= 28
    else:  # (one block of one value: both expansions give it back)
        assert np.array_equal(got, full)


@pytest.mark.parametrize("cut", [0, 1, 7, 9])
@pytest.mark.parametrize("n", [1, 3])
def test_the_model_equals_pillow_on_440(n, cut):
    """Pillow cannot write 4:4:0.  A 16-wide 4:2:2 file of 8n rows has MCUs of (Y, Y, Cb, Cr), one per line; with width 8, height 16n and luma
    factors 1 x 2 the same stream is a 4:4:0 file whose MCUs stack the two luma blocks, over the same 8 x 8n chroma plane."""
    full, C, L = _block_picture(16, 8 * n, 2, 1, 7 + n)  # chroma planes of 8 x 8n samples, one block per MCU
    h = 16 * n - cut
    f = um.patch_sof(_save(full, 1), width=8, height=h, luma=0x12)
    assert um.ratio(f) == (1, 2) and um.qualifies(f)
    got = _read(f)
    assert got.shape == (h, 8, 3)
    luma = np.concatenate([np.concatenate([L[8 * r:8 * r + 8, :8], L[8 * r:8 * r + 8, 8:]], axis=0) for r in range(n)], axis=0)[:h]
    ch = um.chroma_extent(h, 2)
    want = np.stack([luma] + [um.upsample(c[:ch], 1, 2, 8, h) for c in C], axis=-1)
    assert np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())
    if n > 1:
        assert not np.array_equal(got[..., 1], um.replicate(C[0][:ch], 1, 2, 8, h))


# ------------------------------------------------------------------------------------------------ 2: the edge rule

@pytest.fixture(scope="module")
def ramp_420():
    full, C, L = _ramp_picture(32, 32, 2, 2)
    f = _save(full, 2)
    want = np.stack([L] + [um.upsample(c, 2, 2, 32, 32) for c in C], axis=-1)
    assert np.array_equal(_read(f), want)  # (the ramps are IDCT-exact: the native planes are known)
    return f, C, L


@pytest.mark.parametrize("size", [(18, 32), (17, 32), (32, 18), (21, 19)], ids=lambda s: "%dx%d" % s)
def test_the_taps_clamp_to_the_real_extent_not_to_the_mcu_padding(ramp_420, size):
    f, C, L = ramp_420
    w, h = size  # (each keeps the two MCUs per line of the 32 x 32 file)
    got = _read(um.patch_sof(f, width=w, height=h))
    cw, ch = um.chroma_extent(w, 2), um.chroma_extent(h, 2)
    real = np.stack([L[:h, :w]] + [um.upsample(c[:ch, :cw], 2, 2, w, h) for c in C], axis=-1)
    padded = np.stack([L[:h, :w]] + [um.upsample(c, 2, 2, 32, 32)[:h, :w] for c in C], axis=-1)
    assert np.array_equal(got, real), int(np.abs(got.astype(int) - real).max())
    # a smaller even size ends on an odd pixel, whose far tap would be the first padded sample; an odd one on an even pixel, which looks inward
    if (w % 2 == 0 and w < 32) or (h % 2 == 0 and h < 32):
        assert np.abs(got.astype(int) - padded).max() >= 1
    else:
        assert np.array_equal(real, padded)


@pytest.mark.parametrize("subsampling", [2, 1], ids=["420", "422"])
def test_planes_up_to_two_samples_wide_are_replicated(subsampling):
    hs, vs = SUBSAMPLING[subsampling]
    full, C, L = _ramp_picture(16, 8 * vs, hs, vs)  # one MCU per line
    f = _save(full, subsampling)
    h = 8 * vs
    assert np.array_equal(_read(f), np.stack([L] + [um.upsample(c, hs, vs, 16, h) for c in C], axis=-1))
    for w in range(1, 8):
        g = um.patch_sof(f, width=w)
        got = _read(g)
        cw = um.chroma_extent(w, 2)
        fancy = np.stack([L[:, :w]] + [um.upsample(c[:, :cw], hs, vs, w, h) for c in C], axis=-1)
        plain = np.stack([L[:, :w]] + [um.replicate(c[:, :cw], hs, vs, w, h) for c in C], axis=-1)
        assert um.qualifies(g) == (w >= 5)
        assert np.array_equal(got, fancy if w >= 5 else plain), w
        assert np.array_equal(um.filtered(plain, hs, vs), fancy if w >= 5 else plain), w
        if w >= 3:  # (from two chroma columns on, the two expansions differ)
            assert not np.array_equal(fancy, plain), w


# ------------------------------------------------------------------------------------------------ 3: the header arithmetic

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "k3u_taps.h"
using namespace jpgpu;
static const uint32_t kRatios[3][2] = {{2, 1}, {2, 2}, {1, 2}};
static const uint32_t kSizes[4] = {1, 2, 3, 7};
static unsigned long outside = 0;
static void window(uint32_t W, uint32_t H, uint32_t hs, uint32_t vs, uint32_t x, uint32_t y, uint32_t w, uint32_t h) {
    const K3uSpan sx = k3u_fetch_span(x, x + w, W, hs), sy = k3u_fetch_span(y, y + h, H, vs);
    std::printf("F %u %u %u %u %u %u %u %u %u %u %u %u\n", W, H, hs, vs, x, y, w, h, sx.lo, sy.lo, sx.hi - sx.lo, sy.hi - sy.lo);
    const uint32_t cw = k3u_chroma_extent(W, hs), ch = k3u_chroma_extent(H, vs);
    for (uint32_t py = y; py < y + h; py++)
        for (uint32_t px = x; px < x + w; px++) {
            if (px < sx.lo || px >= sx.hi || py < sy.lo || py >= sy.hi) outside++;  // the luma sample
            const K3uTap tx = hs == 2 ? k3u_tap(px, cw) : K3uTap{px, px, true}, ty = vs == 2 ? k3u_tap(py, ch) : K3uTap{py, py, true};
            for (uint32_t i : {tx.near, tx.far})
                for (uint32_t j : {ty.near, ty.far})
                    if (!k3u_sample_in_span(i, hs, sx) || !k3u_sample_in_span(j, vs, sy)) outside++;
        }
}
int main() {
    for (uint32_t W = 1; W <= 20; W++)
        for (uint32_t H = 1; H <= 20; H++)
            for (auto &r : kRatios) {
                const uint32_t hs = r[0], vs = r[1], cw = k3u_chroma_extent(W, hs), ch = k3u_chroma_extent(H, vs);
                std::printf("R %u %u %u %u %u %u %d\n", W, H, hs, vs, cw, ch, (int)k3u_ratio_filtered(hs, vs, W));
                for (uint32_t y = 0; y < H; y++)
                    for (uint32_t x = 0; x < W; x++) {
                        const K3uTap tx = hs == 2 ? k3u_tap(x, cw) : K3uTap{x, x, true}, ty = vs == 2 ? k3u_tap(y, ch) : K3uTap{y, y, true};
                        std::printf("T %u %u %u %u %u %u %u %u\n", x, y, tx.near, tx.far, ty.near, ty.far, k3u_bias(hs, vs, x, y), k3u_shift(hs, vs));
                    }
                for (uint32_t s : kSizes)
                    for (uint32_t y = 0; y + s <= H; y++)
                        for (uint32_t x = 0; x + s <= W; x++) window(W, H, hs, vs, x, y, s, s);
                window(W, H, hs, vs, 0, 0, W, H);
            }
    std::printf("outside %lu\n", outside);
    return outside != 0;
}
"""


def _expected_printout():
    out = []
    for W in range(1, 21):
        for H in range(1, 21):
            for hs, vs in um.RATIOS:
                cw, ch = um.chroma_extent(W, hs), um.chroma_extent(H, vs)
                out.append("R %d %d %d %d %d %d %d" % (W, H, hs, vs, cw, ch, um.ratio_filtered(hs, vs, W)))
                xs, ys = np.arange(W), np.arange(H)
                xn, xf, xe = um.taps(xs, cw) if hs == 2 else (xs, xs, xs == xs)
                yn, yf, ye = um.taps(ys, ch) if vs == 2 else (ys, ys, ys == ys)
                shift = 4 if (hs, vs) == (2, 2) else 2
                for y in range(H):
                    for x in range(W):
                        bias = ((8 if xe[x] else 7) if vs == 2 else (1 if xe[x] else 2)) if hs == 2 else (1 if ye[y] else 2)
                        out.append("T %d %d %d %d %d %d %d %d" % (x, y, xn[x], xf[x], yn[y], yf[y], bias, shift))
                for s in (1, 2, 3, 7):
                    for y in range(H - s + 1):
                        for x in range(W - s + 1):
                            out.append("F %d %d %d %d %d %d %d %d %d %d %d %d" % ((W, H, hs, vs, x, y, s, s) + um.fetch_rect(x, y, s, s, W, H, hs, vs)))
                out.append("F %d %d %d %d 0 0 %d %d %d %d %d %d" % ((W, H, hs, vs, W, H) + um.fetch_rect(0, 0, W, H, W, H, hs, vs)))
    out.append("outside 0")
    return out


def _axis_inside(size, step, p0, n):
    """every sample the model reads for the pixels [p0, p0 + n) of one axis lies inside the model's span (a fetch rectangle is the product of
    two spans, a pixel's samples the product of its taps per axis: the program above counts the same in two dimensions)"""
    lo, hi = um.fetch_span(p0, p0 + n, size, step)
    ps = np.arange(p0, p0 + n)
    at = np.concatenate(um.taps(ps, um.chroma_extent(size, 2))[:2]) * 2 if step == 2 else ps
    return lo <= min(at.min(), p0) and max(at.max(), p0 + n - 1) < hi


@pytest.fixture(scope="module")
def taps_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / c++) on PATH: the enumeration cannot run"
    d = tmp_path_factory.mktemp("k3u_taps")
    src = d / "k3u_taps.cpp"
    src.write_text(PROGRAM)
    exes = {}
    for name, flags in (("plain", ["-O1"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[name] = str(d / ("k3u_taps_" + name))
        subprocess.check_call([cxx, *flags, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exes[name], str(src)])
    return exes


def test_the_header_states_the_models_taps_and_fetch_rectangles(taps_program):
    r = subprocess.run([taps_program["plain"]], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-300:] + r.stderr
    got, want = r.stdout.split("\n"), _expected_printout()
    assert got[-1] == "" and len(got) - 1 == len(want) > 400_000, (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)


def test_every_tap_lies_inside_the_fetch_rectangle():
    for size in range(1, 21):
        for step in (1, 2):
            for n in (1, 2, 3, 7, size):
                for p0 in range(size - n + 1):
                    assert _axis_inside(size, step, p0, n), (size, step, p0, n)
            assert um.fetch_span(0, size, size, step) == (0, size)  # (a whole frame is fetched whole)


def test_the_header_program_runs_clean_under_the_sanitizers(taps_program):
    r = subprocess.run([taps_program["sanitized"]], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.endswith("outside 0\n")


# ------------------------------------------------------------------------------------------------ 4: the ABI without a device

def test_the_library_exports_the_policy_and_the_header_states_its_values():
    import jpeglibrary_amd as jl

    lib = jl._capi.lib
    for name in ("jpgpu_batch_set_upsampling_policy", "jpgpu_batch_image_upsampling"):
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
        assert any(s[0] == name for s in jl._capi.SYMBOLS), name
    header = open(os.path.join(ROOT, "include", "jpgpu.h")).read()
    values = dict(re.findall(r"\b(JPGPU_UPSAMPLE_[A-Z]+)\s*=\s*(\d+)", header))
    assert values == {"JPGPU_UPSAMPLE_REPLICATE": "0", "JPGPU_UPSAMPLE_FANCY": "1"}
    assert jl._capi.UPSAMPLING_POLICIES == ("replicate", "fancy")  # (a policy's value is its index)
    assert lib.jpgpu_batch_set_upsampling_policy(None, 1) == jl._capi.ERR_ARGUMENT  # no batch: refused without a device
    applied = ctypes.c_int(7)
    assert lib.jpgpu_batch_image_upsampling(None, 0, ctypes.byref(applied)) == jl._capi.ERR_ARGUMENT and applied.value == 7
    assert lib.jpgpu_version() == 101


@pytest.mark.parametrize("bad", ["triangle", 1, None, "FANCY", b"fancy"], ids=repr)
def test_the_python_helpers_refuse_a_bad_policy_before_any_library_call(bad):
    import jpeglibrary_amd as jl

    assert [jl.batch._upsampling_policy(p) for p in ("replicate", "fancy")] == [0, 1]
    with pytest.raises(ValueError):
        jl.batch._upsampling_policy(bad)
    b = object.__new__(jl.Batch)  # no context, no handle: a library call would be refused with another exception
    b._h = None
    with pytest.raises(ValueError):
        b.set_upsampling_policy(bad)
    for helper, args in ((jl.decode_batch, ([b"x"],)), (jl.decode_to_tensors, ([b"x"],)), (jl.decode_resized, ([b"x"], (8, 8)))):
        with pytest.raises(ValueError, match="upsampling"):
            helper(*args, upsampling=bad)
