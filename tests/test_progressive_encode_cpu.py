"""The encoder's coding policies "optimized" and "progressive" without a GPU (include/jpgpu.h, 4e).

1. The serial restatement (progressive_encoder_model.py, on libjpeg_encoder_model.quantised_blocks) writes, SOI to EOI, the files Pillow
   (libjpeg-turbo) writes with optimize=True / progressive=True: sizes 1 x 1 to 127 x 65, the three subsamplings and grey, qualities 1, 50, 75,
   100, restart intervals under "optimized".
2. The two engineered inputs, each with its precondition asserted from the model's counters: an EOB run that reaches 0x7FFF, and refinement
   scans of nothing but correction bits that the 937-bit rule flushes.
3. jpgpu_libjpeg_optimal_table against the model's builder.
4. The symbols and the checks that need no device."""
import ctypes
import io

import numpy as np
import pytest

import progressive_encoder_model as pm

Image = pytest.importorskip("PIL.Image")

SIZES = [(1, 1), (8, 8), (16, 16), (33, 17), (40, 24), (127, 65)]  # (width, height)
LUMA = {0: (1, 1), 1: (2, 1), 2: (2, 2)}


def picture(w, h):
    rng = np.random.default_rng(11 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(xx * 5 + yy * 3) % 256, 255 - (xx * 2 + yy * 7) % 256, (xx + yy) * 3 % 256], -1)
    return np.where(rng.random((h, w, 1)) < 0.4, smooth, rng.integers(0, 256, (h, w, 3))).astype(np.uint8)


def pillow(a, quality, subsampling=None, **kw):
    f = io.BytesIO()
    if a.ndim == 2:
        Image.fromarray(a).save(f, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(a).save(f, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return f.getvalue()


def same(got, want, what):
    assert got == want, (what, pm.describe_mismatch(got, want))


# ------------------------------------------------------------------------------------------------ 1: the model is Pillow

@pytest.mark.parametrize("q", [1, 50, 75, 100])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_model_writes_pillows_progressive_and_optimized_files(size, q):
    a = picture(*size)
    for s, luma in LUMA.items():
        same(pm.encode_progressive(a, luma, q), pillow(a, q, s, progressive=True), ("progressive", s))
        same(pm.encode_optimized(a, luma, q), pillow(a, q, s, optimize=True), ("optimized", s))
    grey = np.ascontiguousarray(a[..., 1])
    same(pm.encode_progressive(grey, (1, 1), q), pillow(grey, q, progressive=True), "progressive grey")
    same(pm.encode_optimized(grey, (1, 1), q), pillow(grey, q, optimize=True), "optimized grey")


def test_progressive_with_and_without_optimize_is_one_file():
    a = picture(40, 24)
    assert pillow(a, 75, 2, progressive=True) == pillow(a, 75, 2, progressive=True, optimize=True)


@pytest.mark.parametrize("ri", [1, 3])
def test_the_optimized_coding_takes_restart_intervals(ri):
    for w, h in [(40, 24), (33, 17), (127, 65)]:
        a = picture(w, h)
        for s, luma in LUMA.items():
            same(pm.encode_optimized(a, luma, 75, restart_interval=ri), pillow(a, 75, s, optimize=True, restart_marker_blocks=ri), (w, h, s))
        grey = np.ascontiguousarray(a[..., 1])
        same(pm.encode_optimized(grey, (1, 1), 75, restart_interval=ri), pillow(grey, 75, optimize=True, restart_marker_blocks=ri), (w, h, "L"))


def test_the_scan_order_of_a_33_by_17_image():
    luma = pm.scan_blocks(33, 17, 3, (2, 2), (0,))
    assert len(luma) == 5 * 3 and len(pm.scan_blocks(33, 17, 3, (2, 2), (0, 1, 2))) == 3 * 2 * 6  # real blocks | the padded grid
    assert [b for _, b in luma[:5]] == [0, 1, 6, 7, 12] and luma[5][1] == 2  # raster order through MCUs of 6 blocks
    assert len(pm.scan_blocks(33, 17, 3, (2, 2), (2,))) == 3 * 2


# ------------------------------------------------------------------------------------------------ 2: engineered inputs

def _scan_data_bytes(data):
    return [n - (8 + 2 * data[at + 4]) for m, at, n in pm.split_markers(data) if m == 0xDA]


def test_a_flat_grey_image_runs_into_the_eob_run_limit():
    a = np.full((1024, 2056), 128, np.uint8)  # 257 x 128 = 32 896 blocks
    want = pillow(a, 75, progressive=True)
    same(pm.encode_progressive(a, (1, 1), 75), want, "flat grey")
    assert pm.COUNTERS["eobrun_limit"] == 4 and pm.COUNTERS["max_run"] == 0x7FFF and pm.COUNTERS["block_flush"] == 0
    assert pm.COUNTERS["cross_256"] >= 4 * (32896 // 256 - 1)  # the run goes through every workgroup's 256 blocks
    sizes = _scan_data_bytes(want)
    assert [sizes[k] for k in (1, 2, 3, 5)] == [4, 4, 4, 4]


def test_a_flat_rgb_image_does_the_same_in_luma():
    a = np.full((1024, 2056, 3), 128, np.uint8)
    want = pillow(a, 75, 2, progressive=True)
    same(pm.encode_progressive(a, (2, 2), 75), want, "flat rgb")
    assert pm.COUNTERS["eobrun_limit"] == 4  # the four AC scans of luma; chroma has 129 x 64 blocks
    sizes = _scan_data_bytes(want)
    assert [sizes[k] for k in (1, 4, 5, 9)] == [4, 4, 4, 4]


def test_refinement_scans_of_nothing_but_correction_bits_flush_at_937():
    tile = np.random.default_rng(2).integers(0, 256, (8, 8), dtype=np.uint8)
    a = np.tile(tile, (1, 40))
    blocks = pm.M.quantised_blocks(a, (1, 1), 100, False)
    assert np.abs(blocks[:, 1:]).min() >= 4  # every AC coefficient: non-zero before either refinement scan, never newly so
    want = pillow(a, 100, progressive=True)
    same(pm.encode_progressive(a, (1, 1), 100), want, "tiled")
    # two refinement scans x (blocks 15 and 30: 15 x 63 = 945 > 937) and their ends; nothing else ever flushes in them
    assert pm.COUNTERS["be_limit"] == 4 and pm.COUNTERS["max_run"] == 15 and pm.COUNTERS["zrl_flush"] == 0
    segs = pm.split_markers(want)
    scans = [k for k, (m, _, _) in enumerate(segs) if m == 0xDA]
    assert [_scan_data_bytes(want)[k] for k in (3, 5)] == [317, 322]
    for k in (3, 5):
        m, at, n = segs[scans[k] - 1]
        assert m == 0xC4 and want[at + 4] == 0x10 and want[at + 5:at + 21] == bytes([1] + [0] * 15) and want[at + 21:at + n] == b"\x30"


# ------------------------------------------------------------------------------------------------ 3: the table builder

def _library_table(freq):
    from jpeglibrary_amd import _capi

    f = np.ascontiguousarray(freq, dtype=np.uint32)
    bits, values, n = (ctypes.c_uint8 * 16)(), (ctypes.c_uint8 * 256)(), ctypes.c_int(0)
    assert _capi.lib.jpgpu_libjpeg_optimal_table(f.ctypes.data, bits, values, ctypes.byref(n)) == 0
    return list(bits), list(values)[:n.value]


def test_an_empty_histogram_gives_the_empty_table():
    zeros = np.zeros(256, np.uint32)
    assert _library_table(zeros) == ([0] * 16, []) == pm.optimal_table(zeros)
    from jpeglibrary_amd import encoder

    assert encoder.libjpeg_optimal_table(zeros) == ([0] * 16, [])


def _check_table(freq):
    bits, values = _library_table(freq)
    assert (bits, values) == pm.optimal_table(freq)
    assert sum(bits) == len(values) == int(np.count_nonzero(freq))
    assert sum(b / 2.0 ** (k + 1) for k, b in enumerate(bits)) < 1.0  # Kraft, with room for the all-ones code
    return bits, values


def test_the_librarys_optimal_table_is_the_models():
    rng = np.random.default_rng(5)
    for trial in range(120):
        f = np.zeros(256, np.uint32)
        idx = rng.choice(256, int(rng.integers(2, 257)), replace=False)
        f[idx] = rng.integers(1, (3, 200, 1 << 20)[trial % 3], len(idx))  # many ties | few | none
        _check_table(f)
    for s in (0, 0x30, 255):  # one symbol: a 1-bit code
        f = np.zeros(256, np.uint32)
        f[s] = 1000
        assert _check_table(f) == ([1] + [0] * 15, [s])
    fib = np.zeros(256, np.uint32)
    a, b = 1, 1
    for k in range(40):
        fib[3 * k] = a
        a, b = b, a + b
    assert pm.longest_unlimited_code(fib) > 16  # the limit to 16 bits has work to do
    bits, _ = _check_table(fib)
    assert bits[15] > 0
    assert _library_table(np.zeros(256, np.uint32)) == ([0] * 16, []) == pm.optimal_table(np.zeros(256, np.uint32))  # no symbol: the empty table
    _check_table(np.ones(256, np.uint32))
    _check_table(np.arange(1, 257, dtype=np.uint32))
    _check_table(rng.integers(1, 1 << 24, 256).astype(np.uint32))
    from jpeglibrary_amd import encoder

    assert encoder.libjpeg_optimal_table(fib) == pm.optimal_table(fib)


# ------------------------------------------------------------------------------------------------ 4: symbols and checks

def test_the_new_symbols_exist_and_the_names_are_checked_before_the_library():
    import jpeglibrary_amd as jl
    from jpeglibrary_amd import _capi, encoder

    for name in ("jpgpu_encoder_set_coding_policy", "jpgpu_encoder_image_coding", "jpgpu_libjpeg_optimal_table"):
        assert hasattr(_capi.lib, name), name
    assert _capi.CODING_POLICIES == ("standard", "optimized", "progressive")
    assert _capi.lib.jpgpu_libjpeg_optimal_table(None, None, None, None) != 0
    with pytest.raises(ValueError):
        encoder._coding_policy("baseline")
    with pytest.raises(ValueError):
        jl.encode_batch([np.zeros((8, 8), np.uint8)], coding="baseline")  # (before a context is made)
    header = open(_capi.__file__.replace("jpeglibrary_amd/_capi.py", "include/jpgpu.h")).read()
    assert "JPGPU_CODING_PROGRESSIVE = 2" in header and "jpgpu_encoder_set_coding_policy" in header
