"""The resize stage (jpgpu_batch_set_resize, K4): a ragged batch resampled to one [N, 3, oh, ow] buffer in one launch behind K3.

The expectation is always the numpy model (tests/resize_model.py) applied to Batch.output(i) of the same RGB_PLANAR_U8 upload -- K3's bytes
are pinned elsewhere -- and the comparison is by bit pattern.  Covered: 4:2:0, 4:4:4, grey and progressive sources; whole frames and windows
that are MCU-aligned, unaligned, 7 x 9, one pixel, one line and one column; output sizes 1x1, 5x7, 16x16, the identity, 32x24 (enlarging),
9x300 (more than 256 columns, one more row than a band); a 16 x 1024 image to 2x5 (about 770 vertical taps) and a 4200 x 8 one to 3x5 (a row longer
than the piece K4 stages at a time); uint8, float16 and float32
samples, the floats with the default constants, ImageNet's and a set that drives float16 into subnormals and to infinity; a mixed batch
with a file that fails; the setting as launch state, its withdrawal and the refusals; the one-call helper; the timings."""
import ctypes as C
import gc
import io

import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from jpeglibrary_amd.errors import ArgumentException, InvalidOperationException
from float_sink_model import DEFAULT, IMAGENET, TIES
from tools import jpegsynth
import resize_model as rm

pytestmark = pytest.mark.gpu

NP = {torch.uint8: np.uint8, torch.float16: np.float16, torch.float32: np.float32}
VARIANTS = [("u8", torch.uint8, DEFAULT), ("f16", torch.float16, DEFAULT), ("f32", torch.float32, DEFAULT), ("f16_imagenet", torch.float16, IMAGENET),
            ("f32_imagenet", torch.float32, IMAGENET), ("f16_edges", torch.float16, TIES), ("f32_edges", torch.float32, TIES)]
V_IDS = [v[0] for v in VARIANTS]


def _progressive(w, h):
    from PIL import Image

    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([(xx * 7) % 256, (yy * 5) % 256, (xx * 3 + yy * 2) % 256], axis=-1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=85, progressive=True)
    assert b"\xff\xc2" in buf.getvalue()
    return buf.getvalue()


_FILES = {}


def _source(name):
    """-> (file, W, H)"""
    if name not in _FILES:
        if name == "progressive":
            _FILES[name] = (_progressive(48, 40), 48, 40)
        else:
            w, h, sub, dri = {"420": (64, 48, "420", 2), "444": (40, 56, "444", 0), "gray": (43, 37, "gray", 3), "tall": (16, 1024, "420", 4), "wide": (4200, 8, "444", 0)}[name]
            _FILES[name] = (bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=w * 7 + h)), w, h)
    return _FILES[name]


def _windows(W, H):
    """whole frame, MCU-aligned, unaligned, 7 wide by 9 tall, one pixel, one line, one column"""
    return [(0, 0, 0, 0), (16, 16, 16, 16), (5, 3, min(37, W - 5), min(29, H - 3)), (3, 2, 7, 9), (W - 1, H - 1, 1, 1), (0, 7, W, 1), (9, 0, 1, H)]


def _sizes(W, H):
    """(oh, ow): 1x1, 5x7, 16x16, the identity of the whole frame and of the unaligned window, 32x24 (9x7 enlarged), 9x300"""
    return [(1, 1), (5, 7), (16, 16), (H, W), (min(29, H - 3), min(37, W - 5)), (32, 24), (9, 300)]


_MODEL_V = {}


def _model_v(key, planes, oh, ow):
    """the model's float32 result for (source, window, size), computed once and shared by the sample types"""
    key = key + (oh, ow)
    if key not in _MODEL_V:
        _MODEL_V[key] = rm.resample(planes, oh, ow)
    return _MODEL_V[key]


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(-1), want.reshape(-1)
        bad = np.flatnonzero(g.view(np.dtype("u%d" % g.itemsize)) != w.view(np.dtype("u%d" % w.itemsize)))
        raise AssertionError("%s: %d of %d samples differ, the first at %d: %r, not %r" % (what, len(bad), g.size, bad[0], g[bad[0]], w[bad[0]]))


def _check_resized(b, keys, sources, oh, ow, dtype, consts):
    """the resized buffer of batch b against the model over b.output(i); sources[i]: uint8[3, h, w] or None for an image that failed"""
    got = b.resized()
    assert got.shape == (len(sources), 3, oh, ow) and got.dtype == NP[dtype]
    for i, planes in enumerate(sources):
        if planes is None:
            assert not got[i].view(np.uint8).any(), i
            continue
        want = rm.sample(_model_v(keys[i], planes, oh, ow), NP[dtype], *consts)
        _assert_bits(got[i], want, "image %d %r -> %dx%d %s" % (i, keys[i], oh, ow, NP[dtype].__name__))


# ------------------------------------------------------------------------------------------------ 1: sources x windows x sizes x sample types

@pytest.mark.parametrize("variant", VARIANTS, ids=V_IDS)
@pytest.mark.parametrize("source", ["420", "444", "gray", "progressive"])
def test_every_window_at_every_size(source, variant):
    _, dtype, consts = variant
    f, W, H = _source(source)
    windows = _windows(W, H)
    b = jl.Batch().set_output_affine(*consts).set_windows(windows).upload([f] * len(windows), jl.FMT_RGB_PLANAR_U8)
    planes = None
    for oh, ow in _sizes(W, H):
        b.set_resize((oh, ow), dtype).decode().sync()  # (one upload: the setting is launch state)
        if planes is None:
            planes = [b.output(i) for i in range(len(windows))]
            assert [p.shape for p in planes] == [(3, r[3] or H, r[2] or W) for r in windows]
        _check_resized(b, [(source, i) for i in range(len(windows))], planes, oh, ow, dtype, consts)
        for i in range(len(windows)):  # the per-image outputs stay what they are
            assert np.array_equal(b.output(i), planes[i])


@pytest.mark.parametrize("variant", VARIANTS, ids=V_IDS)
def test_many_vertical_taps(variant):
    _, dtype, consts = variant
    f, W, H = _source("tall")
    assert rm.max_taps(H, 2) >= 760
    b = jl.Batch().set_output_affine(*consts).set_resize((2, 5), dtype).upload([f], jl.FMT_RGB_PLANAR_U8).decode().sync()
    _check_resized(b, [("tall", 0)], [b.output(0)], 2, 5, dtype, consts)


@pytest.mark.parametrize("variant", VARIANTS[:3], ids=V_IDS[:3])
def test_a_row_longer_than_one_staged_piece(variant):
    """K4 stages 4096 bytes of a plane's row at a time: a 4200-wide frame to 5 columns (about 1680 taps each) walks two pieces per row, and a
    window of it to 600 columns walks three column chunks"""
    _, dtype, consts = variant
    f, W, H = _source("wide")
    assert rm.max_taps(W, 5) > 1600
    windows = [(0, 0, 0, 0), (3, 1, 4190, 6)]
    b = jl.Batch().set_windows(windows).upload([f, f], jl.FMT_RGB_PLANAR_U8)
    planes = None
    for oh, ow in [(3, 5), (8, 600)]:
        b.set_resize((oh, ow), dtype).decode().sync()
        planes = planes or [b.output(0), b.output(1)]
        _check_resized(b, [("wide", 0), ("wide", 1)], planes, oh, ow, dtype, consts)


# ------------------------------------------------------------------------------------------------ 2: the identity

@pytest.mark.parametrize("dtype,fmt", [(torch.uint8, jl.FMT_RGB_PLANAR_U8), (torch.float16, jl.FMT_RGB_PLANAR_F16), (torch.float32, jl.FMT_RGB_PLANAR_F32)],
                         ids=["u8", "f16", "f32"])
def test_at_its_own_size_an_image_is_what_the_plain_formats_hold(dtype, fmt):
    W, H = 40, 56
    files = [bytes(jpegsynth.encode(W, H, sub, 75, dri, seed=11 + dri)) for sub, dri in (("444", 0), ("420", 2), ("gray", 1))] + [_progressive(W, H)]
    plain = jl.Batch().set_output_affine(*IMAGENET).upload(files, fmt).decode()
    b = jl.Batch().set_output_affine(*IMAGENET).set_resize((H, W), dtype).upload(files, jl.FMT_RGB_PLANAR_U8).decode()
    t = b.resized_tensor()
    assert t.shape == (len(files), 3, H, W) and t.dtype == dtype and t.device.type == "cuda"
    for i in range(len(files)):
        want = plain.output_tensor(i)
        assert want.dtype == dtype and torch.equal(t[i].view(torch.uint8), want.view(torch.uint8)), i


# ------------------------------------------------------------------------------------------------ 3: a mixed batch with a file that fails

def _twelve_bit(f):
    """the frame header says 12 bits: RGB output refuses such a file on the host, by itself"""
    at = f.index(b"\xff\xc0")
    return f[:at + 4] + b"\x0c" + f[at + 5:]


@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[3], VARIANTS[4]], ids=[V_IDS[0], V_IDS[3], V_IDS[4]])
def test_a_mixed_batch_with_one_file_that_fails(variant):
    _, dtype, consts = variant
    names = ["420", "444", "gray", "progressive", "420", "444", "gray", "progressive"]
    files = [_source(n)[0] for n in names]
    files[5] = _twelve_bit(files[5])
    windows = [(0, 0, 0, 0), (5, 3, 31, 29), (8, 8, 24, 16), (1, 0, 47, 1), (63, 47, 1, 1), (2, 2, 20, 20), (0, 0, 43, 37), (16, 0, 16, 40)]
    oh, ow = 12, 20
    without = jl.Batch().set_windows(windows).upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    b = jl.Batch().set_output_affine(*consts).set_windows(windows).set_resize((oh, ow), dtype).upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    fields = lambda r: tuple(getattr(r, k) for k, _ in r._fields_)
    assert [fields(b.result(i)) for i in range(8)] == [fields(without.result(i)) for i in range(8)]
    assert b.image_info(5).status != 0 and b.result(5).status != 0 and all(b.result(i).status == 0 for i in range(8) if i != 5)
    planes = [None if i == 5 else b.output(i) for i in range(8)]
    for i in range(8):
        if i != 5:
            assert np.array_equal(planes[i], without.output(i))
    _check_resized(b, [("mixed", i) for i in range(8)], planes, oh, ow, dtype, consts)
    t = b.resized_tensor()
    assert not t[5].view(torch.uint8).any()


# ------------------------------------------------------------------------------------------------ 4: state and refusals

def test_the_setting_and_the_constants_are_launch_state():
    f, W, H = _source("420")
    b = jl.Batch().set_resize((10, 12), torch.float32).upload([f], jl.FMT_RGB_PLANAR_U8).decode().sync()
    planes = b.output(0)
    _check_resized(b, [("420", 0)], [planes], 10, 12, torch.float32, DEFAULT)
    b.set_output_affine(*IMAGENET).decode().sync()  # no upload in between: the constants changed take effect
    _check_resized(b, [("420", 0)], [planes], 10, 12, torch.float32, IMAGENET)
    b.set_resize((7, 3), torch.float16).run_idct().sync()  # ... and so does another size, behind run_idct too
    _check_resized(b, [("420", 0)], [planes], 7, 3, torch.float16, IMAGENET)
    # a refused setting leaves the one in force
    for bad in [(-1, 8, jl.FMT_RGB_PLANAR_U8), (8, -1, jl.FMT_RGB_PLANAR_U8), (0, 8, jl.FMT_RGB_PLANAR_U8), (8, 0, jl.FMT_RGB_PLANAR_U8),
                (65536, 8, jl.FMT_RGB_PLANAR_U8), (8, 65536, jl.FMT_RGB_PLANAR_U8), (8, 8, jl.FMT_RGB_U8), (8, 8, jl.FMT_PLANAR_U8), (8, 8, 99), (8, 8, -1)]:
        assert _capi.lib.jpgpu_batch_set_resize(b._h, *bad) == 4, bad
    b.decode().sync()
    _check_resized(b, [("420", 0)], [planes], 7, 3, torch.float16, IMAGENET)
    # the next upload takes it too
    g, _, _ = _source("gray")
    b.upload([g, f], jl.FMT_RGB_PLANAR_U8)
    with pytest.raises(InvalidOperationException):
        b.resized_tensor()  # (the upload's own decode has not run)
    b.decode().sync()
    _check_resized(b, [("gray", 0), ("420", 0)], [b.output(0), planes], 7, 3, torch.float16, IMAGENET)


def test_withdrawing_the_resize():
    f, W, H = _source("444")
    b = jl.Batch().set_resize((8, 8), torch.uint8).upload([f], jl.FMT_RGB_PLANAR_U8).decode().sync()
    before = b.output_tensor(0).clone()
    assert b.resized_tensor().shape == (1, 3, 8, 8)
    b.set_resize(None)
    for call in (b.resized_tensor, b.resized, b.resize_ms):
        with pytest.raises(InvalidOperationException):
            call()
    assert torch.equal(b.output_tensor(0), before)
    b.decode().sync()  # a decode without a resize: as ever
    with pytest.raises(InvalidOperationException):
        b.resized_tensor()
    assert torch.equal(b.output_tensor(0), before)
    # ... and any other format decodes again
    assert b.upload([f], jl.FMT_RGB_U8).decode().sync().output(0).shape == (H, W, 3)


def test_an_upload_of_another_format_is_refused_while_a_resize_is_set():
    f, W, H = _source("420")
    b = jl.Batch().set_resize((8, 8), torch.uint8)
    with pytest.raises(InvalidOperationException):
        b.resized_tensor()  # before any decode
    for fmt in (jl.FMT_RGB_U8, jl.FMT_RGB_PLANAR_F16, jl.FMT_INTERLEAVED_U8):
        b.upload([f], fmt)
        with pytest.raises(ArgumentException, match="RGB_PLANAR_U8"):
            b.decode()
        with pytest.raises(ArgumentException, match="RGB_PLANAR_U8"):
            b.run_idct()
        with pytest.raises(InvalidOperationException):
            b.stage_ms()  # nothing was enqueued: no decode has run
        with pytest.raises(InvalidOperationException):
            b.resized_tensor()
    b.sync()
    b.upload([f], jl.FMT_RGB_PLANAR_U8).decode().sync()  # the batch is still usable
    _check_resized(b, [("420", 0)], [b.output(0)], 8, 8, torch.uint8, DEFAULT)


def test_the_c_accessors():
    f, W, H = _source("gray")
    b = jl.Batch().set_resize((6, 10), torch.float16).upload([f, f], jl.FMT_RGB_PLANAR_U8)
    ptr, total = C.c_void_p(), C.c_uint64()
    assert _capi.lib.jpgpu_batch_resized_device(b._h, C.byref(ptr), C.byref(total)) == 2  # InvalidOperationException
    buf = np.zeros(3 * 6 * 10, np.float16)
    assert _capi.lib.jpgpu_batch_download_resized(b._h, 0, buf.ctypes.data, buf.nbytes) == 2
    b.decode()
    assert _capi.lib.jpgpu_batch_resized_device(b._h, C.byref(ptr), C.byref(total)) == 0
    assert ptr.value and ptr.value % 256 == 0 and total.value == 2 * 3 * 6 * 10 * 2
    assert _capi.lib.jpgpu_batch_resized_device(b._h, None, C.byref(total)) == 4
    assert _capi.lib.jpgpu_batch_download_resized(b._h, 2, buf.ctypes.data, buf.nbytes) == 4
    assert _capi.lib.jpgpu_batch_download_resized(b._h, -1, buf.ctypes.data, buf.nbytes) == 4
    assert _capi.lib.jpgpu_batch_download_resized(b._h, 0, buf.ctypes.data, buf.nbytes - 1) == 4
    assert _capi.lib.jpgpu_batch_download_resized(b._h, 0, None, buf.nbytes) == 4
    assert _capi.lib.jpgpu_batch_download_resized(b._h, 1, buf.ctypes.data, buf.nbytes) == 0  # (waits for the decode itself)
    assert buf.tobytes() == b.resized()[1].tobytes()
    assert _capi.lib.jpgpu_batch_resize_ms(b._h, None) == 4


# ------------------------------------------------------------------------------------------------ 5: the one-call helper

def test_the_helper_gives_the_same_from_bytes_and_from_device_tensors():
    names = ["420", "gray", "progressive", "444"]
    files = [_source(n)[0] for n in names]
    windows = [(5, 3, 37, 29), (0, 0, 0, 0), (8, 0, 24, 40), (0, 0, 0, 0)]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    t, results = jl.decode_resized(files, (14, 18), mean=mean, std=std, windows=windows)
    gc.collect()  # the tensor survives the helper's return: its batch lives with it
    assert t.shape == (4, 3, 14, 18) and t.dtype == torch.float16 and [r.status for r in results] == [0] * 4
    dev = [torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda() for f in files]
    t2, results2 = jl.decode_resized(dev, (14, 18), mean=mean, std=std, windows=windows)
    assert torch.equal(t.view(torch.uint8), t2.view(torch.uint8)) and [r.status for r in results2] == [0] * 4
    plain, _ = jl.decode_to_tensors(files, windows=windows)
    consts = jl.affine_from_mean_std(mean, std)
    for i in range(4):
        want = rm.model(plain[i].cpu().numpy(), 14, 18, np.float16, *consts)
        _assert_bits(t[i].cpu().numpy(), want, "image %d" % i)
    # uint8 and float32; the tensor aliases the batch's resized buffer
    for dtype in (torch.uint8, torch.float32):
        t3, _ = jl.decode_resized(files, (14, 18), dtype=dtype, windows=windows)
        for i in range(4):
            _assert_bits(t3[i].cpu().numpy(), rm.model(plain[i].cpu().numpy(), 14, 18, NP[dtype]), "image %d" % i)


def test_the_tensor_aliases_the_resized_buffer():
    f, W, H = _source("444")
    b = jl.Batch().set_resize((9, 11), torch.float32).upload([f, f, f], jl.FMT_RGB_PLANAR_U8).decode()  # (no sync: resized_tensor does it)
    t = b.resized_tensor()
    ptr, total = C.c_void_p(), C.c_uint64()
    assert _capi.lib.jpgpu_batch_resized_device(b._h, C.byref(ptr), C.byref(total)) == 0
    assert t.data_ptr() == ptr.value and t.numel() * t.element_size() == total.value and t.is_contiguous()
    want = b.resized()
    del b
    gc.collect()
    assert t.cpu().numpy().tobytes() == want.tobytes()  # the tensor keeps the batch alive
    borrowed = jl.Batch._borrowed(0, 0, jl.FMT_RGB_PLANAR_U8)
    with pytest.raises(ValueError, match="borrowed"):
        borrowed.resized_tensor()


# ------------------------------------------------------------------------------------------------ 6: timings

def test_the_resize_has_a_time_of_its_own():
    f, W, H = _source("420")
    b = jl.Batch().set_resize((16, 16), torch.float16).upload([f] * 6, jl.FMT_RGB_PLANAR_U8).decode().sync()
    assert b.resize_ms() > 0
    ms = b.stage_ms()
    assert set(ms) == {"marker_index", "huffman", "idct", "total"} and ms["total"] > 0 and ms["idct"] > 0
    assert ms["total"] >= ms["idct"]
    assert b.resize_ms() > 0  # (still the last launch's)
