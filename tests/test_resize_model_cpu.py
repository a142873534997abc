"""The resize stage (jpgpu_batch_set_resize) as far as it goes without a GPU: the numpy model the GPU tests compare against (its identity,
its distance from a float64 evaluation of the same definition and from torch's float path), the tap tables the library builds on the host,
bit for bit against the model's, the new C symbols, and the argument checks that raise before the library is called.

Model against torch, measured on the CPU with the data below (torch 2.10): the largest difference over the seven cases is 0.0023041, at
300x500 -> 224x224 (1024x16 -> 2x5: 2.3e-5, 37x53 -> 1x1: 7.6e-6, 37x53 -> 9x300: 3.8e-4, 9x7 -> 32x24: 7.6e-5, 500x333 -> 17x16: 9.9e-5,
2x3 -> 5x4: 1.5e-5).  It comes from torch forming its weights in float32 and is not derivable; four times the measured maximum is asserted,
which covers torch builds that order the weight arithmetic differently and stays far below half an 8-bit step."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi, batch
import resize_model as rm

ERR_ARGUMENT = 4
CASES = [(1024, 16, 2, 5), (37, 53, 1, 1), (37, 53, 9, 300), (9, 7, 32, 24), (500, 333, 17, 16), (2, 3, 5, 4)]  # H, W -> oh, ow
TORCH_CASES = CASES + [(300, 500, 224, 224)]
TORCH_MEASURED_MAX = 0.0023041
IDS = ["%dx%d_to_%dx%d" % c for c in TORCH_CASES]


def _planes(h, w):
    return np.random.default_rng(20261019 + 131 * h + w).integers(0, 256, (3, h, w), dtype=np.uint8)


_V32 = {}


def _v32(case):
    """the model's float32 result of a case, computed once"""
    if case not in _V32:
        h, w, oh, ow = case
        _V32[case] = rm.resample(_planes(h, w), oh, ow)
    return _V32[case]


@pytest.mark.parametrize("h,w", [(1, 1), (6, 5), (37, 53), (64, 1), (1, 64)])
def test_the_identity_size_returns_the_bytes(h, w):
    u = _planes(h, w)
    v = rm.resample(u, h, w)
    assert v.dtype == np.float32 and np.array_equal(v, u.astype(np.float32))
    assert np.array_equal(rm.model(u, h, w, np.uint8), u)
    assert rm.model(u, h, w, np.float32).tobytes() == u.astype(np.float32).tobytes()
    # every row of weights is {1, 0} (or {1} at the far edge)
    lo, count, weights, _ = rm.axis_table(w, w)
    assert list(lo) == list(range(w)) and all(float(x[0]) == 1.0 and not x[1:].any() for x in weights)


@pytest.mark.parametrize("case", CASES, ids=IDS[:len(CASES)])
def test_the_model_stays_within_the_derived_bound_of_a_float64_evaluation(case):
    h, w, oh, ow = case
    exact = rm.resample(_planes(h, w), oh, ow, np.float64)
    n_h, n_v = rm.max_taps(w, ow), rm.max_taps(h, oh)
    # each tap's multiply and add rounds to float32 once (2^-24 relative each), the weights sum to 1, every intermediate is about 255 at most;
    # the weights' own rounding takes part of the 4
    bound = (n_h + n_v + 4) * 255 * 2.0 ** -24
    worst = float(np.abs(_v32(case).astype(np.float64) - exact).max())
    print("%s: taps %d + %d, model - float64 = %.3g, bound %.3g" % (case, n_h, n_v, worst, bound))
    assert worst <= bound


@pytest.mark.parametrize("case", TORCH_CASES, ids=IDS)
def test_the_model_is_the_picture_torch_computes_in_float(case):
    h, w, oh, ow = case
    want = torch.nn.functional.interpolate(torch.from_numpy(_planes(h, w))[None].float(), (oh, ow), mode="bilinear", antialias=True, align_corners=False)[0].numpy()
    worst = float(np.abs(_v32(case) - want).max())
    print("%s: model - torch = %.3g" % (case, worst))
    assert worst <= 4 * TORCH_MEASURED_MAX


def _library_table(in_len, out_len):
    f = _capi.lib.jpgpu_debug_resize_table  # (tests only: not part of include/jpgpu.h)
    f.restype = C.c_longlong
    f.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_size_t]
    lo, count = (C.c_int32 * out_len)(), (C.c_int32 * out_len)()
    cap = out_len * (in_len + 2)
    weights = (C.c_float * cap)()
    n = f(in_len, out_len, lo, count, weights, cap)
    assert n >= 0
    return np.array(lo[:]), np.array(count[:]), np.frombuffer(weights, dtype=np.float32, count=n).copy()


PAIRS = sorted({(c[1], c[3]) for c in TORCH_CASES} | {(c[0], c[2]) for c in TORCH_CASES} | {(64, 1), (1, 7), (65535, 3), (3, 300), (3840, 224), (2160, 224)})


@pytest.mark.parametrize("in_len,out_len", PAIRS, ids=["%d_to_%d" % p for p in PAIRS])
def test_the_librarys_host_tables_are_the_models_bit_for_bit(in_len, out_len):
    lo, count, weights = _library_table(in_len, out_len)
    m_lo, m_count, m_weights, _ = rm.axis_table(in_len, out_len)
    assert np.array_equal(lo, m_lo) and np.array_equal(count, m_count)
    assert weights.tobytes() == np.concatenate(m_weights).tobytes()
    assert (weights >= 0).all() and not np.signbit(weights).any()  # (every term of a sum is >= +0: a padded tap of weight +0.0 changes no bit)


def test_the_table_entry_refuses_what_it_cannot_build():
    f = _capi.lib.jpgpu_debug_resize_table
    f.restype = C.c_longlong
    f.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_size_t]
    lo, count, w = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_float * 64)()
    assert f(0, 4, lo, count, w, 64) == -1 and f(4, 0, lo, count, w, 64) == -1 and f(8, 4, lo, count, w, 3) == -1 and f(8, 4, None, count, w, 64) == -1


def test_the_abi_has_the_resize_symbols_and_keeps_its_version():
    lib = _capi.lib
    names = ("jpgpu_batch_set_resize", "jpgpu_batch_resized_device", "jpgpu_batch_download_resized", "jpgpu_batch_resize_ms")
    assert set(names) <= {name for name, _, _ in _capi.SYMBOLS}
    header = open(_capi.LIB_PATH.replace("jpeglibrary_amd/libjpgpu.so", "include/jpgpu.h")).read()
    for name in names:
        assert getattr(lib, name) is not None and name in header, name
    assert lib.jpgpu_version() == 101 and "#define JPGPU_VERSION 101" in header
    # no existing struct changed size
    assert C.sizeof(_capi.ImageInfo) == 160 and lib.jpgpu_sizeof_image_result() == C.sizeof(_capi.ImageResult) == 28
    assert lib.jpgpu_sizeof_plan_stats() == 44 and lib.jpgpu_sizeof_rect() == 16 and lib.jpgpu_sizeof_device_ingest_stats() == 40
    for name in ("set_resize", "resized", "resized_tensor", "resize_ms"):
        assert callable(getattr(jl.Batch, name)), name
    assert callable(jl.decode_resized) and "decode_resized" in jl.__all__


def test_a_null_batch_is_refused():
    lib = _capi.lib
    assert lib.jpgpu_batch_set_resize(None, 8, 8, jl.FMT_RGB_PLANAR_U8) == ERR_ARGUMENT
    assert lib.jpgpu_batch_set_resize(None, 0, 0, 0) == ERR_ARGUMENT
    assert lib.jpgpu_batch_resized_device(None, C.byref(C.c_void_p()), C.byref(C.c_uint64())) == ERR_ARGUMENT
    assert lib.jpgpu_batch_download_resized(None, 0, None, 0) == ERR_ARGUMENT
    assert lib.jpgpu_batch_resize_ms(None, C.byref(C.c_float())) == ERR_ARGUMENT
    # (the refusals that need a batch need a device: tests/test_resize_gpu.py)


BAD_SIZES = [(8,), (8, 8, 8), (0, 8), (8, 0), (-1, 8), (8, 65536), (8.0, 8), ("8", 8), (True, 8), 8, None]
BAD_DTYPES = [torch.int8, torch.float64, torch.bfloat16, np.uint8, "uint8", None]


@pytest.mark.parametrize("bad", BAD_SIZES, ids=[repr(b) for b in BAD_SIZES])
def test_a_size_is_two_integers_from_1_to_65535(bad, monkeypatch):
    called = []
    monkeypatch.setattr(batch, "Batch", lambda *a, **k: called.append(1))  # (any library call goes through a Batch)
    with pytest.raises(ValueError):
        batch._resize_setting(bad, torch.uint8)
    with pytest.raises(ValueError):
        jl.decode_resized([b"x", b"y"], bad)
    assert not called
    if bad is not None:  # (None withdraws the setting)
        b = jl.Batch.__new__(jl.Batch)  # (no context, no handle: a library call would fail on the missing attributes)
        with pytest.raises(ValueError):
            b.set_resize(bad, torch.uint8)


@pytest.mark.parametrize("bad", BAD_DTYPES, ids=[repr(b) for b in BAD_DTYPES])
def test_a_dtype_is_uint8_float16_or_float32(bad, monkeypatch):
    called = []
    monkeypatch.setattr(batch, "Batch", lambda *a, **k: called.append(1))
    with pytest.raises(ValueError):
        batch._resize_setting((8, 8), bad)
    if bad is not None:  # (None is the helpers' default)
        with pytest.raises(ValueError):
            jl.decode_resized([b"x"], (8, 8), dtype=bad)
        b = jl.Batch.__new__(jl.Batch)
        with pytest.raises(ValueError):
            b.set_resize((8, 8), bad)
    assert not called


def test_a_well_formed_setting_passes_through():
    assert batch._resize_setting((224, 320), torch.float16) == (224, 320, jl.FMT_RGB_PLANAR_F16, np.float16)
    assert batch._resize_setting([1, 65535], torch.uint8) == (1, 65535, jl.FMT_RGB_PLANAR_U8, np.uint8)
    assert batch._resize_setting((np.int64(7), 5), torch.float32) == (7, 5, jl.FMT_RGB_PLANAR_F32, np.float32)


def test_the_helper_refuses_mean_and_std_it_cannot_apply(monkeypatch):
    called = []
    monkeypatch.setattr(batch, "Batch", lambda *a, **k: called.append(1))
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    with pytest.raises(ValueError, match="float samples"):
        jl.decode_resized([b"x"], (8, 8), dtype=torch.uint8, mean=mean, std=std)
    with pytest.raises(ValueError, match="go together"):
        jl.decode_resized([b"x"], (8, 8), mean=mean)
    with pytest.raises(ValueError, match="go together"):
        jl.decode_resized([b"x"], (8, 8), dtype=torch.float32, std=std)
    with pytest.raises(ValueError):
        jl.decode_resized([b"x"], (8, 8), mean=(0.5, 0.5), std=std)  # (affine_from_mean_std: three values each)
    with pytest.raises(ValueError):
        jl.decode_resized([b"x", b"y"], (8, 8), windows=[(0, 0, 8, 8)])  # (one window per file)
    with pytest.raises(ValueError, match="mix"):
        jl.decode_resized([b"x", torch.zeros(4, dtype=torch.uint8)], (8, 8))
    assert not called
