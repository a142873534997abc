"""The encoder's arithmetic policy "libjpeg" without a GPU (include/jpgpu.h, 4d).

1. The numpy restatement (libjpeg_encoder_model.py) writes, SOI to EOI, the file Pillow (libjpeg-turbo) writes: sizes 1 x 1 to 33 x 47, the
   three subsamplings, qualities 30 / 75 / 95 (and the ends of the quality rule), noise and smooth content, grey, "YCbCr" input, restart intervals.
2. The transform's 32-bit integers never overflow for 8-bit samples: int32 equals int64 on extreme blocks, and no result leaves +-2^14.
3. The device's division-free quantisation equals the division for every divisor and every numerator up to that bound.
4. The symbols, the argument checks and the refusals that need no device."""
import ctypes
import inspect
import io
import os
import re

import numpy as np
import pytest

import libjpeg_encoder_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Image = pytest.importorskip("PIL.Image")

# what |8 x DCT| can reach: the DC term is 64 samples of magnitude 128 at most, over 8 (x 8) = 8192, every AC term is smaller; the rounding of
# the two passes adds a few units.  The tests below hold the transform to twice that and check the quantiser over all of it.
COEF_BOUND = 1 << 14

SIZES = [(1, 1), (2, 3), (8, 8), (7, 9), (16, 16), (17, 17), (15, 33), (33, 15), (9, 47), (33, 47)]  # (height, width)
LUMA = {0: (1, 1), 1: (2, 1), 2: (2, 2)}


def picture(height, width, kind, seed=0):
    if kind == "noise":
        return np.random.default_rng(seed + 1000 * height + width).integers(0, 256, (height, width, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:height, 0:width]
    return np.stack([(xx * 5 + yy * 3) % 256, 255 - (xx * 2 + yy * 7) % 256, (xx + yy) * 3 % 256], -1).astype(np.uint8)


def pillow(a, quality, subsampling=None, mode=None, **kw):
    f = io.BytesIO()
    if a.ndim == 2:
        Image.fromarray(a).save(f, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(a, mode).save(f, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return f.getvalue()


# ------------------------------------------------------------------------------------------------ 1: the model is Pillow

@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_model_writes_pillows_file(size, kind):
    a = picture(*size, kind)
    for s, luma in LUMA.items():
        for q in (30, 75, 95):
            assert model.encode(a, luma, q, True) == pillow(a, q, s), (s, q)
    grey = np.ascontiguousarray(a[..., 1])
    for q in (30, 75, 95):
        assert model.encode(grey, (2, 2), q, False) == pillow(grey, q), q
    assert model.encode(a, (2, 2), 75, False) == pillow(a, 75, 2, mode="YCbCr")
    assert model.encode(a, (1, 1), 75, False) == pillow(a, 75, 0, mode="YCbCr")


@pytest.mark.parametrize("interval", [1, 2, 7])
def test_the_model_writes_pillows_restart_intervals(interval):
    for size in ((17, 17), (9, 47), (33, 47)):
        a = picture(*size, "noise", 3)
        for s, luma in LUMA.items():
            assert model.encode(a, luma, 75, True, interval) == pillow(a, 75, s, restart_marker_blocks=interval), (size, s)
        grey = np.ascontiguousarray(a[..., 0])
        assert model.encode(grey, (1, 1), 75, False, interval) == pillow(grey, 75, restart_marker_blocks=interval), size


@pytest.mark.parametrize("quality", [1, 10, 49, 50, 51, 75, 95, 100])
def test_the_quality_rule_gives_pillows_tables(quality):
    a = picture(8, 8, "smooth")
    data = pillow(a, quality, 2)
    tables = model.quant_tables(quality)
    at = 0
    for t in range(2):
        at = data.index(b"\xff\xdb", at) + 2
        assert data[at:at + 3] == bytes([0, 67, t]) and data[at + 3:at + 67] == bytes(int(x) for x in tables[t]), t
    assert model.encode(a, (2, 2), quality, True) == data


# ------------------------------------------------------------------------------------------------ 2: 32 bits suffice

def extreme_blocks():
    yy, xx = np.mgrid[0:8, 0:8]
    blocks = [np.zeros((8, 8)), np.full((8, 8), 255), ((xx + yy) & 1) * 255, 255 - ((xx + yy) & 1) * 255, (xx & 1) * 255, (yy & 1) * 255,
              (xx < 4) * 255, (yy < 4) * 255, ((xx < 4) ^ (yy < 4)) * 255]
    cos = np.cos((2 * np.arange(8) + 1)[:, None] * np.arange(8)[None, :] * np.pi / 16)
    for u in range(8):  # the sign pattern of every basis function, and its negative: what drives one coefficient furthest
        for v in range(8):
            pattern = np.outer(cos[:, u], cos[:, v]) >= 0
            blocks += [pattern * 255, ~pattern * 255]
    rng = np.random.default_rng(5)
    blocks += list(rng.integers(0, 2, (512, 8, 8)) * 255) + list(rng.integers(0, 256, (512, 8, 8)))
    return np.array(blocks, np.uint8)


def test_the_int32_transform_is_the_int64_one_and_stays_inside_the_bound():
    blocks = extreme_blocks()
    narrow, wide = model.fdct_islow(blocks, np.int32), model.fdct_islow(blocks, np.int64)
    assert narrow.dtype == np.int32 and wide.dtype == np.int64
    assert np.array_equal(narrow, wide)
    assert wide[0, 0, 0] == -8192 and wide[1, 0, 0] == 8128  # 8 x the DCT
    assert np.abs(wide).max() < COEF_BOUND, np.abs(wide).max()
    # ... and what the constants (below 2^15) are multiplied with stays far inside 24 bits: the device's 24-bit multiply is the product
    assert model.fdct_multiplicand_bound(blocks) < 1 << 17


# ------------------------------------------------------------------------------------------------ 3: the quantiser without a division

def test_the_multiply_high_quantiser_is_the_division_for_every_divisor_and_numerator():
    q = np.arange(1, 256, dtype=np.int64)[:, None]
    c = np.arange(-COEF_BOUND, COEF_BOUND + 1, dtype=np.int64)[None, :]
    want = model.quantise(np.broadcast_to(c, (255, c.shape[1])), q)
    got = model.quantise_mulhi(np.broadcast_to(c, (255, c.shape[1])), q)
    assert np.array_equal(got, want)
    assert int(model.mulhi_factor(np.array([1]))[0]) == (1 << 29) + 1 and int(model.mulhi_factor(255).max()) < 1 << 32
    # the kernel computes the factor as a double quotient, truncated: the same integer for every divisor
    d = (np.arange(1, 256) << 3).astype(np.float64)
    assert np.array_equal((4294967296.0 / d).astype(np.uint64) + 1, model.mulhi_factor(np.arange(1, 256)))
    # halves round away from zero
    assert model.quantise(np.array([4, -4, 3, -3, 12, -12]), np.array([1] * 6)).tolist() == [1, -1, 0, 0, 2, -2]


# ------------------------------------------------------------------------------------------------ 4: the ABI without a device

def test_the_library_exports_the_encoder_policy_and_the_header_states_the_function():
    import jpeglibrary_amd as jl

    lib = jl._capi.lib
    for name in ("jpgpu_encoder_set_arithmetic_policy", "jpgpu_encoder_image_arithmetic"):
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name
        assert any(s[0] == name for s in jl._capi.SYMBOLS), name
    header = open(os.path.join(ROOT, "include", "jpgpu.h")).read()
    section = header[header.index("(4d) Arithmetic"):header.index("int jpgpu_encoder_set_arithmetic_policy")]
    for c in (19595, 38470, 7471, 11059, 21709, 27439, 5329, 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172):
        assert re.search(r"\b%d\b" % c, section), c
    assert lib.jpgpu_encoder_set_arithmetic_policy(None, 1) == jl._capi.ERR_ARGUMENT  # no encoder: refused without a device
    taken = ctypes.c_int(7)
    assert lib.jpgpu_encoder_image_arithmetic(None, 0, ctypes.byref(taken)) == jl._capi.ERR_ARGUMENT and taken.value == 7
    for f in (jl.encode_batch, jl.encode_tensors):
        assert inspect.signature(f).parameters["arithmetic"].default == "reference"
    for f in (jl.EncodeBatch.upload, jl.EncodeBatch.upload_tensors):
        assert inspect.signature(f).parameters["arithmetic"].default is None
    assert callable(jl.EncodeBatch.set_arithmetic_policy) and callable(jl.EncodeBatch.arithmetic)


@pytest.mark.parametrize("bad", ["islow", 1, None, "LIBJPEG", b"libjpeg"], ids=repr)
def test_the_python_entries_refuse_a_bad_policy_before_any_library_call(bad):
    import jpeglibrary_amd as jl

    b = object.__new__(jl.EncodeBatch)  # no context, no handle: a library call would be refused with another exception
    b._h = None
    with pytest.raises(ValueError, match="arithmetic"):
        b.set_arithmetic_policy(bad)
    if bad is not None:  # (None on an upload: the batch's policy as it stands)
        with pytest.raises(ValueError, match="arithmetic"):
            b.upload([np.zeros((8, 8, 3), np.uint8)], arithmetic=bad)
        with pytest.raises(ValueError, match="arithmetic"):
            b.upload_tensors([], arithmetic=bad)
    with pytest.raises(ValueError, match="arithmetic"):
        jl.encode_batch([np.zeros((8, 8, 3), np.uint8)], arithmetic=bad)
    with pytest.raises(ValueError, match="arithmetic"):
        jl.encode_tensors([], arithmetic=bad)


def test_the_makefile_builds_the_stage_and_its_header():
    make = open(os.path.join(ROOT, "jpeglibrary_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KOBJS\s*=.*\be1j_libjpeg\.o\b", make, re.M) and re.search(r"^HDRS\s*=.*\be1j_islow\.h\b", make, re.M)
