"""The encoder's coding policies "optimized" and "progressive" on the device (include/jpgpu.h, 4e; encode_progressive.hip): under
arithmetic="libjpeg" the stream of an image is, byte for byte, the file Pillow (libjpeg-turbo) writes with optimize=True / progressive=True
for the same pixels, quality and subsampling.

Sizes: 1 x 1, 8 x 8, 16 x 16, 33 x 17 (5 x 3 real luma blocks in a padded 6 x 4 at 4:2:0), 40 x 24, 127 x 65 (more than one workgroup of
256 blocks at 4:4:4); the two engineered inputs (an EOB run that reaches 32767 and crosses every workgroup of its scan; refinement scans of
nothing but correction bits, flushed by the 937-bit rule); one 1024 x 768 picture whose scans span many workgroups.  Pillow's files are
computed once per case (lru_cache) and shared; on a mismatch the failure names the scan."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeglibrary_amd as jl
import progressive_encoder_model as pm
from tools.bench_encode import image as bench_image

pytestmark = pytest.mark.gpu

LUMA = {0: (1, 1), 1: (2, 1), 2: (2, 2), "L": (1, 1)}
SIZES = [(1, 1), (8, 8), (16, 16), (33, 17), (40, 24), (127, 65)]  # (width, height)
CODINGS = {"optimized": {"optimize": True}, "progressive": {"progressive": True}}


@functools.lru_cache(maxsize=None)
def _rgb(w, h):
    rng = np.random.default_rng(11 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(xx * 5 + yy * 3) % 256, 255 - (xx * 2 + yy * 7) % 256, (xx + yy) * 3 % 256], -1)
    a = np.where(rng.random((h, w, 1)) < 0.4, smooth, rng.integers(0, 256, (h, w, 3))).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _grey(w, h):
    a = np.ascontiguousarray(_rgb(w, h)[..., 1])
    a.setflags(write=False)
    return a


def _save(a, s, q, **kw):
    f = io.BytesIO()
    if a.ndim == 2:
        Image.fromarray(a).save(f, "JPEG", quality=q, **kw)
    else:
        Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s, **kw)
    return f.getvalue()


@functools.lru_cache(maxsize=None)
def _pillow(w, h, s, coding, q=75, ri=0):
    kw = dict(CODINGS.get(coding, {}))
    if ri:
        kw["restart_marker_blocks"] = ri
    return _save(_grey(w, h) if s == "L" else _rgb(w, h), s, q, **kw)


def _pixels(w, h, s):
    return _grey(w, h) if s == "L" else _rgb(w, h)


def _same(got, want, what):
    assert got == want, (what, pm.describe_mismatch(got, want))


def _device():
    return torch.device("cuda", jl.default_context().device)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(_device())


def _encode(images, s, coding, q=75, ri=0):
    return jl.encode_batch(list(images), LUMA[s], q, rgb=s != "L", restart_interval=ri, arithmetic="libjpeg", coding=coding)


# ------------------------------------------------------------------------------------------------ the size list

@pytest.mark.parametrize("coding", ["optimized", "progressive"])
@pytest.mark.parametrize("s", [0, 1, 2, "L"])
def test_sizes_alone_and_as_one_mixed_batch(s, coding):
    want = [_pillow(w, h, s, coding) for w, h in SIZES]
    b = jl.EncodeBatch().upload([_pixels(w, h, s) for w, h in SIZES], LUMA[s], 75, rgb=s != "L", arithmetic="libjpeg", coding=coding).encode()
    assert [b.coding(i) for i in range(len(b))] == [coding] * len(SIZES)
    for i, size in enumerate(SIZES):
        _same(b.output(i), want[i], ("mixed", size))
    b.close()
    for size, ref in zip(SIZES, want):
        _same(_encode([_pixels(*size, s)], s, coding)[0], ref, ("alone", size))


@pytest.mark.parametrize("coding", ["optimized", "progressive"])
@pytest.mark.parametrize("q", [1, 50, 100])
def test_qualities(q, coding):
    sizes = [(33, 17), (40, 24), (16, 16)]
    for s in (0, 1, 2, "L"):
        got = _encode([_pixels(w, h, s) for w, h in sizes], s, coding, q)
        for size, g in zip(sizes, got):
            _same(g, _pillow(*size, s, coding, q), (s, size))


@pytest.mark.parametrize("ri", [1, 3])
def test_restart_intervals_under_optimized(ri):
    sizes = [(40, 24), (33, 17), (127, 65)]
    for s in (0, 1, 2, "L"):
        got = _encode([_pixels(w, h, s) for w, h in sizes], s, "optimized", ri=ri)
        for size, g in zip(sizes, got):
            _same(g, _pillow(*size, s, "optimized", 75, ri), (s, size))


# ------------------------------------------------------------------------------------------------ every source form

@pytest.mark.parametrize("coding", ["optimized", "progressive"])
def test_tensor_forms(coding):
    sizes = [(33, 17), (127, 65)]
    want = [_pillow(w, h, 2, coding) for w, h in sizes]
    hwc = [_dev(_rgb(w, h)) for w, h in sizes]
    assert jl.encode_tensors(hwc, (2, 2), 75, layout="hwc", arithmetic="libjpeg", coding=coding) == want
    chw = [t.permute(2, 0, 1).contiguous() for t in hwc]
    assert jl.encode_tensors(chw, (2, 2), 75, layout="chw", arithmetic="libjpeg", coding=coding) == want
    rgba = [torch.cat([t, torch.full_like(t[..., :1], 77)], -1).contiguous() for t in hwc]
    assert jl.encode_tensors(rgba, (2, 2), 75, layout="hwc", arithmetic="libjpeg", coding=coding) == want
    w, h = sizes[0]
    store = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device=_device())
    store[1:] = hwc[0].reshape(-1)
    odd = store[1:].view(h, w, 3)  # a view at an odd byte offset
    assert jl.encode_tensors([odd], (2, 2), 75, layout="hwc", arithmetic="libjpeg", coding=coding) == want[:1]
    grey = [_dev(_grey(w, h)) for w, h in sizes]
    assert jl.encode_tensors(grey, (1, 1), 75, rgb=False, layout="hwc", arithmetic="libjpeg", coding=coding) == [_pillow(w, h, "L", coding) for w, h in sizes]


def test_output_tensor_holds_the_progressive_file():
    b = jl.EncodeBatch().upload([_rgb(40, 24), _rgb(33, 17)], (2, 2), 75, rgb=True, arithmetic="libjpeg", coding="progressive").encode()
    for i, size in enumerate([(40, 24), (33, 17)]):
        assert bytes(b.output_tensor(i).cpu().numpy()) == _pillow(*size, 2, "progressive")
    b.close()


# ------------------------------------------------------------------------------------------------ engineered inputs

@functools.lru_cache(maxsize=None)
def _flat(rgb):
    a = np.full((1024, 2056, 3) if rgb else (1024, 2056), 128, np.uint8)
    a.setflags(write=False)
    return a


def test_a_flat_grey_image_is_one_run_through_every_workgroup_of_a_scan():
    want = _save(_flat(False), 0, 75, progressive=True)
    ac = [n for m, _, n in pm.split_markers(want) if m == 0xDA][1:]
    assert [n - 10 for n in ac if n < 100] == [4, 4, 4, 4]  # each AC scan: EOB14 of 32767 blocks, then the other 129
    _same(_encode([_flat(False)], "L", "progressive")[0], want, "flat grey")


def test_a_flat_rgb_image_does_the_same_in_luma():
    _same(_encode([_flat(True)], 2, "progressive")[0], _save(_flat(True), 2, 75, progressive=True), "flat rgb 4:2:0")


def test_refinement_scans_of_nothing_but_correction_bits():
    tile = np.random.default_rng(2).integers(0, 256, (8, 8), dtype=np.uint8)
    a = np.tile(tile, (1, 40))
    want = _save(a, 0, 100, progressive=True)
    _same(_encode([a], "L", "progressive", q=100)[0], want, "tiled 8 x 320")


@functools.lru_cache(maxsize=None)
def _picture():
    a = np.ascontiguousarray(bench_image(1024, 768, 3))
    a.setflags(write=False)
    return a


def test_a_picture_whose_runs_cross_workgroup_edges():
    a = _picture()
    want = _save(a, 2, 75, progressive=True)
    _same(_encode([a], 2, "progressive")[0], want, "1024 x 768")
    _same(_encode([a], 2, "optimized")[0], _save(a, 2, 75, optimize=True), "1024 x 768 optimized")
    assert pm.encode_progressive(a, (2, 2), 75) == want
    assert pm.COUNTERS["cross_256"] >= 1  # a run that goes on from one workgroup's 256 blocks into the next


# ------------------------------------------------------------------------------------------------ round trip, coefficients

def test_the_decoder_reads_the_progressive_file_as_the_standard_one():
    imgs = [_rgb(127, 65), _rgb(33, 17)]
    std = jl.encode_batch(imgs, (2, 2), 75, rgb=True, arithmetic="libjpeg")
    prog = _encode(imgs, 2, "progressive")
    opt = _encode(imgs, 2, "optimized")
    a, ra = jl.decode_batch(std, jl.FMT_INTERLEAVED_U8)
    for files in (prog, opt):
        b, rb = jl.decode_batch(files, jl.FMT_INTERLEAVED_U8)
        assert [r.status for r in ra + rb] == [0] * 4
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_the_coefficients_do_not_depend_on_the_coding():
    imgs = [_rgb(33, 17), _rgb(127, 65)]
    got = {}
    for coding in ("standard", "optimized", "progressive"):
        b = jl.EncodeBatch().upload(imgs, (2, 2), 75, rgb=True, arithmetic="libjpeg", coding=coding).encode()
        got[coding] = [b.coefficients(i) for i in range(2)]
        b.close()
    for coding in ("optimized", "progressive"):
        for x, y in zip(got["standard"], got[coding]):
            assert np.array_equal(x, y), coding


# ------------------------------------------------------------------------------------------------ refusals, reuse, defaults

def test_refusals_leave_the_encoder_usable():
    b = jl.EncodeBatch()
    img = _rgb(40, 24)
    for coding in ("optimized", "progressive"):
        with pytest.raises(jl.ArgumentException):
            b.upload([img], (2, 2), 75, rgb=True, arithmetic="reference", coding=coding)
    with pytest.raises(jl.ArgumentException):
        b.upload([img], (2, 2), 75, rgb=True, restart_interval=2, arithmetic="libjpeg", coding="progressive")
    with pytest.raises(jl.ArgumentException):  # (the refusal of 4d stays)
        b.upload([img], (2, 2), 75, rgb=True, optimize_coding=True, arithmetic="libjpeg", coding="optimized")
    with pytest.raises(ValueError):
        b.set_coding_policy("arithmetic")
    _same(b.upload([img], (2, 2), 75, rgb=True, arithmetic="libjpeg", coding="progressive").encode().output(0), _pillow(40, 24, 2, "progressive"), "after refusals")
    b.close()


def test_one_batch_reused_across_codings_and_arithmetics_gives_a_fresh_encoders_bytes():
    big, small = _rgb(127, 65), _rgb(16, 16)
    steps = [("libjpeg", "standard", big), ("libjpeg", "progressive", big), ("libjpeg", "optimized", small), ("reference", "standard", big),
             ("libjpeg", "progressive", small), ("libjpeg", "standard", small), ("libjpeg", "optimized", big), ("libjpeg", "progressive", big)]
    b = jl.EncodeBatch()
    for arithmetic, coding, img in steps:
        got = b.upload([img, small], (2, 2), 75, rgb=True, arithmetic=arithmetic, coding=coding).encode()
        fresh = jl.encode_batch([img, small], (2, 2), 75, rgb=True, arithmetic=arithmetic, coding=coding)
        assert [got.output(0), got.output(1)] == fresh, (arithmetic, coding, img.shape)
    b.close()


def test_the_default_and_standard_write_what_they_always_wrote():
    imgs = [_rgb(33, 17), _rgb(40, 24)]
    for arithmetic in ("reference", "libjpeg"):
        plain = jl.EncodeBatch().upload(imgs, (2, 2), 75, rgb=True, arithmetic=arithmetic).encode()
        assert [plain.coding(i) for i in range(2)] == ["standard"] * 2
        assert [plain.output(i) for i in range(2)] == jl.encode_batch(imgs, (2, 2), 75, rgb=True, arithmetic=arithmetic, coding="standard")
        plain.close()
    assert jl.encode_batch(imgs, (2, 2), 75, rgb=True, arithmetic="libjpeg") == [_pillow(33, 17, 2, "standard"), _pillow(40, 24, 2, "standard")]


@pytest.mark.parametrize("coding", ["optimized", "progressive"])
def test_a_callers_quantisation_table_reaches_the_dqt_and_the_blocks(coding):
    img = _rgb(40, 24)
    table = (np.arange(64) % 23 + 3).astype(np.uint16)  # zig-zag order
    b = jl.EncodeBatch().upload([img], (2, 2), 75, rgb=True, arithmetic="libjpeg", coding=coding)
    b.set_quantization_table(0, 0, table).encode()
    got = b.output(0)
    b.close()
    natural = np.empty(64, np.int64)
    natural[np.array(pm.M.NATURAL)] = table
    chroma = np.empty(64, np.int64)
    chroma[np.array(pm.M.NATURAL)] = pm.M.quant_tables(75)[1]
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", subsampling=2, qtables=[[int(x) for x in natural], [int(x) for x in chroma]], **CODINGS[coding])
    _same(got, f.getvalue(), "caller's table")
