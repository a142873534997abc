"""The encoder's arithmetic policy "libjpeg" on the device (include/jpgpu.h, 4d; stage E1J, e1j_libjpeg.hip): the stream of an image is,
byte for byte from SOI to EOI, the file Pillow (libjpeg-turbo) writes for the same pixels, quality and subsampling.

Sizes: 1 x 1, 8 x 8, 7 x 9, 16 x 16; 17 x 17 (a 4:2:0 MCU with a dummy luma block on the right and below); 15 x 33, 33 x 15, 9 x 47; 2080 x 17
for 4:2:0 and 1048 x 9 for 4:4:4 (130 and 131 MCUs per line: past one workgroup's 128); a tensor view at an odd byte offset.  Every source
kind, the three subsamplings and grey, qualities 1, 50, 75, 100, both emit paths (a batch of one: two kernels; a mixed batch: one pass),
restart intervals, a caller's table, the coefficients, the refusals, the default policy, and the loop through the decoder.

Pillow's files and the model's blocks are computed once per case (lru_cache) and shared."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import encoder_arrangements as ea
import encoder_model as em
import jpeglibrary_amd as jl
import libjpeg_encoder_model as model

pytestmark = pytest.mark.gpu

LUMA = {0: (1, 1), 1: (2, 1), 2: (2, 2)}  # Pillow's subsampling -> luma factors
SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 17), (33, 15), (15, 33), (47, 9)]  # (width, height)
WIDE = {2: (2080, 17), 0: (1048, 9), 1: (2080, 9)}  # 130, 131, 130 MCUs per line


@functools.lru_cache(maxsize=None)
def _rgb(w, h):
    rng = np.random.default_rng(7 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(xx * 5 + yy * 3) % 256, 255 - (xx * 2 + yy * 7) % 256, (xx + yy) * 3 % 256], -1)
    a = np.where(rng.random((h, w, 1)) < 0.5, smooth, rng.integers(0, 256, (h, w, 3))).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _grey(w, h):
    a = np.ascontiguousarray(_rgb(w, h)[..., 1])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _pillow(w, h, s, q=75, ri=0, mode=None):
    """s = 0, 1, 2, or "L" for grey; mode "YCbCr": the samples as they are"""
    f = io.BytesIO()
    kw = {"restart_marker_blocks": ri} if ri else {}
    if s == "L":
        Image.fromarray(_grey(w, h)).save(f, "JPEG", quality=q, **kw)
    else:
        Image.fromarray(_rgb(w, h), mode).save(f, "JPEG", quality=q, subsampling=s, **kw)
    return f.getvalue()


def _device():
    return torch.device("cuda", jl.default_context().device)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(_device())  # (a writable copy: the cached pictures are read-only)


def _sizes(s):
    return SIZES + [WIDE[s]]


# ------------------------------------------------------------------------------------------------ host arrays, both emit paths

@pytest.mark.parametrize("s", [0, 1, 2])
def test_host_arrays_give_pillows_files_alone_and_in_a_mixed_batch(s):
    sizes = _sizes(s)
    want = [_pillow(w, h, s) for w, h in sizes]
    b = jl.EncodeBatch().upload([_rgb(w, h) for w, h in sizes], LUMA[s], 75, rgb=True, arithmetic="libjpeg").encode()
    assert [b.arithmetic(i) for i in range(len(b))] == [1] * len(sizes)
    for i, size in enumerate(sizes):
        assert b.output(i) == want[i], ("mixed", size)
    assert b.emit_passes()[0] == 1  # one pass over the blocks
    b.close()
    for size, ref in zip(sizes, want):
        one = jl.EncodeBatch().upload([_rgb(*size)], LUMA[s], 75, rgb=True, arithmetic="libjpeg").encode()
        assert one.output(0) == ref, ("alone", size)
        assert one.emit_passes() == (0, 0)  # a batch of one: the two kernels
        one.close()


def test_grey_host_arrays_give_pillows_files_whatever_luma_says():
    sizes = SIZES + [(1048, 9)]
    want = [_pillow(w, h, "L") for w, h in sizes]
    for luma in ((2, 2), (1, 1)):
        got = jl.encode_batch([_grey(w, h) for w, h in sizes], luma, 75, arithmetic="libjpeg")
        for size, g, ref in zip(sizes, got, want):
            assert g == ref, (luma, size)
    assert jl.encode_batch([_grey(17, 17)], (2, 1), 75, arithmetic="libjpeg") == [_pillow(17, 17, "L")]


@pytest.mark.parametrize("q", [1, 50, 100])
def test_the_quality_rule_on_the_device(q):
    sizes = [(17, 17), (47, 9), (16, 16)]
    for s in (0, 1, 2):
        got = jl.encode_batch([_rgb(w, h) for w, h in sizes], LUMA[s], q, rgb=True, arithmetic="libjpeg")
        assert got == [_pillow(w, h, s, q) for w, h in sizes], s
    assert jl.encode_batch([_grey(17, 17), _grey(9, 7)], (1, 1), q, arithmetic="libjpeg") == [_pillow(17, 17, "L", q), _pillow(9, 7, "L", q)]


def test_ycbcr_samples_are_taken_as_they_are():
    sizes = [(17, 17), (33, 15)]
    for s in (0, 2):
        got = jl.encode_batch([_rgb(w, h) for w, h in sizes], LUMA[s], 75, rgb=False, arithmetic="libjpeg")
        assert got == [_pillow(w, h, s, mode="YCbCr") for w, h in sizes], s


# ------------------------------------------------------------------------------------------------ tensors

@pytest.mark.parametrize("s", [0, 1, 2])
def test_tensors_of_every_kind_give_pillows_files(s):
    sizes = _sizes(s)
    want = [_pillow(w, h, s) for w, h in sizes]
    chw = [_dev(_rgb(w, h).transpose(2, 0, 1)) for w, h in sizes]
    hwc = [_dev(_rgb(w, h)) for w, h in sizes]
    rgba = [_dev(np.concatenate([_rgb(w, h), np.full((h, w, 1), 201 + (w & 7), np.uint8)], -1)) for w, h in sizes]
    assert jl.encode_tensors(chw, LUMA[s], 75, arithmetic="libjpeg") == want
    assert jl.encode_tensors(hwc, LUMA[s], 75, layout="hwc", arithmetic="libjpeg") == want
    assert jl.encode_tensors(rgba, LUMA[s], 75, layout="hwc", arithmetic="libjpeg") == want
    for k in (0, 4, len(sizes) - 1):  # ... and alone: the two-kernel emit
        assert jl.encode_tensors([chw[k]], LUMA[s], 75, arithmetic="libjpeg") == [want[k]], sizes[k]
        assert jl.encode_tensors([rgba[k]], LUMA[s], 75, layout="hwc", arithmetic="libjpeg") == [want[k]], sizes[k]


def test_grey_tensors_give_pillows_files():
    sizes = SIZES + [(1048, 9)]
    want = [_pillow(w, h, "L") for w, h in sizes]
    assert jl.encode_tensors([_dev(_grey(w, h)) for w, h in sizes], (2, 2), 75, rgb=False, layout="hwc", arithmetic="libjpeg") == want
    assert jl.encode_tensors([_dev(_grey(w, h)[None]) for w, h in sizes], (1, 1), 75, rgb=False, arithmetic="libjpeg") == want


@pytest.mark.parametrize("s", [0, 2])
def test_a_tensor_view_at_an_odd_byte_offset(s):
    for (w, h), offset in (((33, 15), 1), ((47, 9), 3), ((17, 17), 5)):
        flat = torch.zeros(h * w * 3 + offset, dtype=torch.uint8, device=_device())
        view = flat[offset:].view(h, w, 3)
        view.copy_(_dev(_rgb(w, h)))
        assert view.data_ptr() % 2 == 1 and view.is_contiguous()
        assert jl.encode_tensors([view], LUMA[s], 75, layout="hwc", arithmetic="libjpeg") == [_pillow(w, h, s)], (w, h)


# ------------------------------------------------------------------------------------------------ restart intervals, tables, coefficients

@pytest.mark.parametrize("ri", [1, 3])
def test_restart_intervals_are_pillows_restart_marker_blocks(ri):
    sizes = [(17, 17), (47, 9), (33, 15)]
    for s in (0, 1, 2):
        got = jl.encode_batch([_rgb(w, h) for w, h in sizes], LUMA[s], 75, rgb=True, restart_interval=ri, arithmetic="libjpeg")
        assert got == [_pillow(w, h, s, 75, ri) for w, h in sizes], s
    got = jl.encode_batch([_grey(w, h) for w, h in sizes], (1, 1), 75, restart_interval=ri, arithmetic="libjpeg")
    assert got == [_pillow(w, h, "L", 75, ri) for w, h in sizes]


def test_a_callers_table_reaches_the_dqt_and_the_blocks():
    rng = np.random.default_rng(11)
    t0, t1 = rng.integers(1, 256, 64).astype(np.uint16), rng.integers(1, 40, 64).astype(np.uint16)
    t0[0], t1[0] = 1, 255
    w, h = 33, 15
    b = jl.EncodeBatch().upload([_rgb(w, h), _rgb(17, 17)], (2, 2), 75, rgb=True, arithmetic="libjpeg")
    b.set_quantization_table(0, 0, t0).set_quantization_table(0, 1, t1).encode()
    got = b.output(0)
    assert got == model.encode(_rgb(w, h), (2, 2), 75, True, tables=(t0, t1))
    at = got.index(b"\xff\xdb")
    assert got[at:at + 5] == b"\xff\xdb\x00\x43\x00" and got[at + 5:at + 69] == bytes(t0.astype(np.uint8))
    assert got[at + 69:at + 74] == b"\xff\xdb\x00\x43\x01" and got[at + 74:at + 138] == bytes(t1.astype(np.uint8))
    assert np.array_equal(b.coefficients(0), model.quantised_blocks(_rgb(w, h), (2, 2), 75, True, tables=(t0, t1)))
    assert b.output(1) == _pillow(17, 17, 2)  # (the other image keeps the scaled standard tables)
    b.close()
    g = jl.EncodeBatch().upload([_grey(w, h)], (1, 1), 75, arithmetic="libjpeg").set_quantization_table(0, 0, t0).encode()
    assert g.output(0) == model.encode(_grey(w, h), (1, 1), 75, False, tables=(t0, t1))
    g.close()


@pytest.mark.parametrize("s", [0, 1, 2])
def test_the_downloaded_coefficients_are_the_models_blocks(s):
    sizes = [(17, 17), (47, 9), (1, 1)] + [WIDE[s]]
    b = jl.EncodeBatch().upload([_rgb(w, h) for w, h in sizes], LUMA[s], 75, rgb=True, arithmetic="libjpeg").encode()
    for i, (w, h) in enumerate(sizes):
        assert np.array_equal(b.coefficients(i), model.quantised_blocks(_rgb(w, h), LUMA[s], 75, True)), (w, h)
    b.close()
    g = jl.EncodeBatch().upload([_grey(17, 17)], (2, 2), 75, arithmetic="libjpeg").encode()
    assert np.array_equal(g.coefficients(0), model.quantised_blocks(_grey(17, 17), (2, 2), 75, False))
    g.close()


# ------------------------------------------------------------------------------------------------ refusals and the default policy

def test_every_refusal_leaves_the_encoder_usable():
    a = _rgb(33, 15)
    fresh = jl.encode_batch([a], (2, 2), 75, rgb=True)
    b = jl.EncodeBatch().set_arithmetic_policy("libjpeg")
    with pytest.raises(jl.ArgumentException, match="optimize_coding"):
        b.upload([a], (2, 2), 75, rgb=True, optimize_coding=True)
    for luma in ((4, 1), (1, 2), (4, 4), (2, 4)):
        with pytest.raises(jl.ArgumentException, match="luma sampling"):
            b.upload([a], luma, 75, rgb=True)
    with pytest.raises(jl.ArgumentException, match="luma sampling"):
        b.upload_tensors([_dev(a)], (1, 2), 75, rgb=True, layout="hwc")
    desc = ea.to_description(em.encode_action(2, 2, 3, 75), 33, 15)
    with pytest.raises(jl.InvalidOperationException, match="described"):
        b.upload_described([a], [desc])
    with pytest.raises(jl.InvalidOperationException, match="described"):
        b.upload_described_tensors([_dev(a)], [desc], layout="hwc")
    assert b.upload([a], (2, 2), 75, rgb=True).encode().output(0) == _pillow(33, 15, 2)  # (the policy is still the one that was set)
    b.set_arithmetic_policy("reference")
    assert b.upload([a], (2, 2), 75, rgb=True).encode().output(0) == fresh[0]
    assert b.arithmetic(0) == 0
    assert b.upload([a], (2, 2), 75, rgb=True, optimize_coding=True).encode().output(0) == jl.encode_batch([a], (2, 2), 75, rgb=True, optimize_coding=True)[0]
    b.close()


@pytest.mark.parametrize("luma", [(2, 2), (2, 1), (1, 1)])
def test_the_default_policy_writes_the_streams_it_always_wrote(luma):
    sizes = [(17, 17), (47, 9)]
    want = [em.encode(_rgb(w, h), em.encode_action(luma[0], luma[1], 3, 75))[0] for w, h in sizes]
    images = [_rgb(w, h) for w, h in sizes]
    assert jl.encode_batch(images, luma, 75) == want
    assert jl.encode_batch(images, luma, 75, arithmetic="reference") == want
    assert jl.encode_tensors([_dev(a) for a in images], luma, 75, rgb=False, layout="hwc") == want
    assert jl.encode_tensors([_dev(a) for a in images], luma, 75, rgb=False, layout="hwc", arithmetic="reference") == want
    b = jl.EncodeBatch().upload(images, luma, 75, arithmetic="libjpeg").upload(images, luma, 75, arithmetic="reference").encode()
    assert [b.output(i) for i in range(2)] == want and [b.arithmetic(i) for i in range(2)] == [0, 0]
    b.close()
    assert want[0] != _pillow(17, 17, {v: k for k, v in LUMA.items()}[luma], mode="YCbCr")


# ------------------------------------------------------------------------------------------------ the loop

@pytest.mark.parametrize("s", [0, 1, 2])
def test_encode_then_decode_gives_the_pixels_pillow_reads_from_its_own_file(s):
    sizes = [(33, 15), (47, 9), (16, 16), (64, 48)]
    x = [_dev(_rgb(w, h).transpose(2, 0, 1)) for w, h in sizes]
    files = jl.encode_tensors(x, LUMA[s], 75, arithmetic="libjpeg")
    tensors, results = jl.decode_to_tensors(files, arithmetic="libjpeg", upsampling="fancy")
    for (w, h), f, t, r in zip(sizes, files, tensors, results):
        assert r.status == 0 and f == _pillow(w, h, s)
        want = np.asarray(Image.open(io.BytesIO(_pillow(w, h, s))).convert("RGB"))
        assert np.array_equal(t.cpu().numpy().transpose(1, 2, 0), want), (w, h)
