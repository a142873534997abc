"""Grey output (jpgpu_batch_set_channels_policy), what holds without a GPU: the C ABI has the three new symbols, the version stays 101 and no
public struct changed its size; the model's L (tests/luma_model.py) is Pillow's convert("L"), on random RGB and on the RGB color_model gives
for a CMYK fixture; the Python argument checks of mode= and of mean / std under "gray" raise before the library is called."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi, batch
import color_model as cm
import luma_model as lm

ERR_ARGUMENT = 4


def test_the_abi_has_the_channels_symbols_and_keeps_its_version_and_struct_sizes():
    lib = _capi.lib
    header = open(_capi.LIB_PATH.replace("jpeglibrary_amd/libjpgpu.so", "include/jpgpu.h")).read()
    for name in ("jpgpu_batch_set_channels_policy", "jpgpu_batch_image_channels", "jpgpu_batch_luma_work"):
        assert getattr(lib, name) is not None, name
        assert name in header, name
    assert "JPGPU_CHANNELS_RGB = 0" in header and "JPGPU_CHANNELS_LUMA = 1" in header
    assert _capi.CHANNELS_POLICIES == ("rgb", "gray")
    assert lib.jpgpu_version() == 101 and "#define JPGPU_VERSION 101" in header
    assert C.sizeof(_capi.ImageInfo) == 160 and lib.jpgpu_sizeof_image_result() == C.sizeof(_capi.ImageResult) == 28
    assert lib.jpgpu_sizeof_plan_stats() == C.sizeof(_capi.PlanStats) == 44 and lib.jpgpu_sizeof_progressive_plan() == C.sizeof(_capi.ProgressivePlan) == 56
    assert lib.jpgpu_sizeof_rect() == C.sizeof(_capi.Rect) == 16 and lib.jpgpu_sizeof_device_ingest_stats() == C.sizeof(_capi.DeviceIngestStats) == 40


def test_a_null_batch_is_refused():
    lib = _capi.lib
    assert lib.jpgpu_batch_set_channels_policy(None, 1) == ERR_ARGUMENT
    assert lib.jpgpu_batch_image_channels(None, 0, C.byref(C.c_int())) == ERR_ARGUMENT
    assert lib.jpgpu_batch_luma_work(None, (C.c_int32 * 2)()) == ERR_ARGUMENT


def test_the_models_l_is_pillows_convert_l_on_random_rgb():
    from PIL import Image

    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 256, (257, 255, 3), dtype=np.uint8)
    rgb[0, :8] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1], [254, 255, 254], [128, 127, 129]]
    want = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
    assert np.array_equal(lm.L(rgb), want)
    assert lm.L(np.array([255, 255, 255])) == 255 and lm.L(np.array([0, 0, 0])) == 0  # (the weights sum to 65536: white stays white)


def test_the_models_l_is_pillows_convert_l_on_the_rgb_of_a_cmyk_fixture():
    from PIL import Image

    f, kind = cm.kind_file("cmyk")
    assert kind == "cmyk"
    # the file's own samples, as Pillow decodes them (C M Y K stored inverted by the Adobe convention: the bytes the frame holds)
    samples = 255 - np.asarray(Image.open(io.BytesIO(f)))
    assert samples.shape == (67, 45, 4)
    rgb = cm.model("cmyk", samples)
    want = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
    assert np.array_equal(lm.gray("cmyk", samples), want)
    assert np.array_equal(lm.plane("cmyk", samples, (3, 5, 20, 30), 6)[0], np.rot90(want, -1)[5:35, 3:23])  # (orientation 6: a quarter turn clockwise)
    # the kinds that carry luma give component 0
    assert np.array_equal(lm.gray("ycbcr", samples[..., :3]), samples[..., 0]) and np.array_equal(lm.gray("gray", samples[..., :1]), samples[..., 0])


def test_the_float_forms_use_one_scale_and_one_bias():
    u = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    assert lm.as_dtype(u, np.uint8) is u
    for dt in (np.float16, np.float32):
        got = lm.as_dtype(u, dt, -0.75, 100.25)
        assert got.dtype == dt and got.shape == u.shape
        assert np.array_equal(got, (u.astype(np.float32) * np.float32(-0.75) + np.float32(100.25)).astype(dt))


BAD_MODES = ["grey", "GRAY", "luma", "", None, 1, True, b"gray"]


@pytest.mark.parametrize("bad", BAD_MODES, ids=[repr(b) for b in BAD_MODES])
def test_mode_is_rgb_or_gray(bad, monkeypatch):
    called = []
    monkeypatch.setattr(batch, "Batch", lambda *a, **k: called.append(1))  # (any library call goes through a Batch)
    with pytest.raises(ValueError):
        batch._channels_policy(bad)
    with pytest.raises(ValueError):
        jl.decode_batch([b"x"], jl.FMT_RGB_PLANAR_U8, mode=bad)
    with pytest.raises(ValueError):
        jl.decode_to_tensors([b"x"], mode=bad)
    with pytest.raises(ValueError):
        jl.decode_resized([b"x"], (8, 8), mode=bad)
    assert not called
    assert batch._channels_policy("rgb") == 0 and batch._channels_policy("gray") == 1


OTHER_FORMATS = [jl.FMT_INTERLEAVED_U8, jl.FMT_PLANAR_U8, jl.FMT_PLANAR_I16, jl.FMT_RGB_U8, jl.FMT_RGBA_U8, jl.FMT_EXTENDED_U16, jl.FMT_INTERLEAVED_U8_SCALED]


@pytest.mark.parametrize("fmt", OTHER_FORMATS)
def test_gray_with_a_format_that_is_not_rgb_planar_raises(fmt, monkeypatch):
    called = []
    monkeypatch.setattr(batch, "Batch", lambda *a, **k: called.append(1))
    with pytest.raises(ValueError):
        jl.decode_batch([b"x"], fmt, mode="gray")
    with pytest.raises(ValueError):
        jl.decode_to_tensors([b"x"], fmt=fmt, mode="gray")
    assert not called
    for ok in (jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_PLANAR_F32):
        assert batch._channels_policy("gray", ok) == 1
    assert batch._channels_policy("rgb", fmt) == 0  # (the default composes with every format)


BAD_STATS = [([0.5, 0.5, 0.5], [0.2, 0.2, 0.2]), ([0.5, 0.5], 0.2), (0.5, [0.2, 0.2, 0.2]), ([], [])]


@pytest.mark.parametrize("mean,std", BAD_STATS, ids=[repr(b) for b in BAD_STATS])
def test_mean_and_std_under_gray_are_one_value_each(mean, std, monkeypatch):
    import torch

    called = []
    monkeypatch.setattr(batch, "Batch", lambda *a, **k: called.append(1))
    with pytest.raises(ValueError):
        jl.decode_to_tensors([b"x"], dtype=torch.float32, mean=mean, std=std, mode="gray")
    with pytest.raises(ValueError):
        jl.decode_resized([b"x"], (8, 8), mean=mean, std=std, mode="gray")
    assert not called
    for m, s in ((0.5, 0.25), ([0.5], [0.25]), (np.float32(0.5), (0.25,))):
        mm, ss = batch._gray_mean_std(m, s)
        assert mm == [0.5] * 3 and ss == [0.25] * 3
    scale, bias = jl.affine_from_mean_std(*batch._gray_mean_std(0.5, 0.25))
    assert scale[0] == np.float32(1.0 / (255.0 * 0.25)) and bias[0] == np.float32(-2.0)
    with pytest.raises(ValueError):  # (both or neither, as under "rgb")
        jl.decode_to_tensors([b"x"], dtype=torch.float32, mean=0.5, mode="gray")
