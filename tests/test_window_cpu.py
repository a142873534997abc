"""Windows (jpgpu_batch_set_windows), what holds without a GPU: the C ABI has the new symbols and the rect's size, the version stays 101,
the Python argument checks raise before the library is called, and jpgpu_batch_set_windows refuses a NULL batch."""
import ctypes as C

import pytest

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi, batch

ERR_ARGUMENT = 4


def test_the_abi_has_the_window_symbols_and_keeps_its_version():
    lib = _capi.lib
    for name in ("jpgpu_batch_set_windows", "jpgpu_batch_image_window", "jpgpu_batch_idct_listed_mcus"):
        assert getattr(lib, name) is not None, name
    assert lib.jpgpu_sizeof_rect() == 16 == C.sizeof(_capi.Rect)
    assert [n for n, _ in _capi.Rect._fields_] == ["x", "y", "width", "height"]
    assert lib.jpgpu_version() == 101
    # no existing struct grew
    assert C.sizeof(_capi.ImageInfo) == 160 and lib.jpgpu_sizeof_image_result() == C.sizeof(_capi.ImageResult) == 28
    header = open(_capi.LIB_PATH.replace("jpeglibrary_amd/libjpgpu.so", "include/jpgpu.h")).read()
    assert "#define JPGPU_VERSION 101" in header
    for name in ("jpgpu_rect", "jpgpu_sizeof_rect", "jpgpu_batch_set_windows", "jpgpu_batch_image_window", "jpgpu_batch_idct_listed_mcus"):
        assert name in header, name


def test_a_null_batch_is_refused():
    lib = _capi.lib
    rect = (_capi.Rect * 1)(_capi.Rect(0, 0, 8, 8))
    assert lib.jpgpu_batch_set_windows(None, rect, 1) == ERR_ARGUMENT
    assert lib.jpgpu_batch_set_windows(None, None, 0) == ERR_ARGUMENT
    assert lib.jpgpu_batch_image_window(None, 0, rect) == ERR_ARGUMENT
    assert lib.jpgpu_batch_idct_listed_mcus(None, C.byref(C.c_uint64())) == ERR_ARGUMENT
    # (n < 0 and NULL windows with n > 0 need a batch, which needs a device: tests/test_window_gpu.py)


BAD_RECTS = [(0, 0, 8), (0, 0, 8, 8, 8), (-1, 0, 8, 8), (0, 0, 8, 2 ** 32), (0, 0, 8.0, 8), (0, 0, "8", 8), (0, 0, True, 8), 7, None]


@pytest.mark.parametrize("bad", BAD_RECTS, ids=[repr(b) for b in BAD_RECTS])
def test_a_rect_is_four_non_negative_integers_below_2_32(bad, monkeypatch):
    called = []
    monkeypatch.setattr(batch, "Batch", lambda *a, **k: called.append(1))  # (any library call goes through a Batch)
    with pytest.raises(ValueError):
        batch._window_rects([(0, 0, 8, 8), bad])
    with pytest.raises(ValueError):
        jl.decode_batch([b"x", b"y"], jl.FMT_RGB_U8, windows=[(0, 0, 8, 8), bad])
    with pytest.raises(ValueError):
        jl.decode_to_tensors([b"x", b"y"], windows=[(0, 0, 8, 8), bad])
    assert not called


def test_one_window_per_file(monkeypatch):
    called = []
    monkeypatch.setattr(batch, "Batch", lambda *a, **k: called.append(1))
    for n in (0, 1, 3):
        with pytest.raises(ValueError):
            jl.decode_batch([b"x", b"y"], jl.FMT_RGB_U8, windows=[(0, 0, 8, 8)] * n)
        with pytest.raises(ValueError):
            jl.decode_to_tensors([b"x", b"y"], windows=[(0, 0, 8, 8)] * n)
    assert not called
    assert batch._window_rects([(1, 2, 3, 4), [0, 0, 0, 0], (2 ** 32 - 1, 0, 1, 1)], 3) == [(1, 2, 3, 4), (0, 0, 0, 0), (2 ** 32 - 1, 0, 1, 1)]
    assert batch._window_rects(None, 5) is None


def test_set_windows_checks_before_the_library_is_called():
    b = batch.Batch.__new__(batch.Batch)  # (no context, no handle: a library call would fail on the missing attributes)
    with pytest.raises(ValueError):
        b.set_windows([(0, 0, -8, 8)])
