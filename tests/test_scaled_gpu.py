"""The scaled decode on the GPU: libjpeg's reduced transforms in K3R (include/jpgpu.h, "Scaled decode").

Every expected value is, bit for bit, tests/scaled_model.py -- shown to be libjpeg's scaled decode by tests/test_scaled_cpu.py -- over the
oracle's coefficients of the same file, and where Pillow decodes the file the way the policies ask (upsampling="fancy", a layout libjpeg
filters or does not sub-sample) Pillow's draft() decode as well.  Covered: the three denominators on grey, 4:4:4, 4:2:0, 4:2:2, 4:4:0 and
4:1:1 files with DRI 0 and 4; widths 1..8 at 1/8; block rows around a workgroup's 256 blocks; the five RGB formats with mean / std; which
pictures are filtered; progressive and three-scan files; windows on the reduced frame; the eight orientations; mode="gray"; CMYK, YCCK and
Adobe-RGB files; a truncated and a corrupted file; a mixed batch with a 12-bit file; the fit rule; decode_resized; and the policy's hygiene."""
import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from tools import jpegsynth
import color_model as cm
import islow_model as im
import luma_model as lm
import orient_model as om
import policy_model as pm
import resize_model as rm
import scaled_model as sm
from test_color_gpu import _assert_bits
from test_libjpeg_gpu import _file

pytestmark = pytest.mark.gpu

FMT = jl.FMT_RGB_PLANAR_U8
PILLOW_RATIOS = ("gray", "444", "422", "420", "440")  # where upsampling="fancy" is libjpeg's output
_MODEL = {}


def _model(f, denom, upsampling="replicate", kind=None):
    """uint8[H', W', 3], computed once per (file, denominator, upsampling, kind)"""
    key = (f, denom, upsampling, kind)
    if key not in _MODEL:
        _MODEL[key] = sm.decode(f, denom, upsampling, kind) if denom > 1 else im.decode(f, upsampling, kind)
    return _MODEL[key]


def _decode(files, denom, fmt=FMT, consts=None, upsampling="replicate", windows=None, orientations=None, color="ycc", mode="rgb", arithmetic="libjpeg", fit=None):
    b = jl.Batch().set_color_policy(color).set_upsampling_policy(upsampling).set_channels_policy(mode).set_arithmetic_policy(arithmetic)
    b.set_scale_policy(denom)
    if fit is not None:
        b.set_scale_fit(fit)
    if consts is not None:
        b.set_output_affine(*consts)
    if orientations is not None:
        b.set_orientations(orientations)
    if windows is not None:
        b.set_windows(windows)
    return b.upload(files, fmt).decode().sync()


def _check(b, i, f, denom, what, upsampling="replicate", fmt=FMT, pillow=False):
    assert b.result(i).status == 0 and b.arithmetic(i) == 1 and b.scale(i) == denom, (what, b.result(i).status, b.arithmetic(i), b.scale(i))
    W, H = im.frame(f)[:2]
    info = b.image_info(i)
    assert (info.width, info.height) == (W, H) and b.window(i) == (0, 0) + sm.out_size(W, H, denom), (what, b.window(i))
    want = _model(f, denom, upsampling)
    _assert_bits(b.output(i), cm.as_format(want, fmt), what)
    if pillow:
        p = sm.pillow_draft(f, denom, "RGB", strict=False)  # (None where draft() does not pick this scale: a side below 8 / denom pixels)
        if p is not None:
            _assert_bits(b.output(i), cm.as_format(p, fmt), "Pillow: " + what)


# ------------------------------------------------------------------------------------------------ 1: values

def _value_files():
    cases = [("gray", 9, 9), ("gray", 8, 8), ("444", 8, 8), ("444", 17, 9), ("420", 16, 16), ("420", 17, 17), ("420", 24, 17), ("422", 16, 8), ("422", 33, 17),
             ("440", 8, 16), ("411", 32, 8)]
    files, what, subs = [], [], []
    for k, (sub, w, h) in enumerate(cases):
        for dri in (0, 4):
            files.append(_file(w, h, sub, 75, dri, seed=20 + k))
            what.append("%dx%d %s dri %d" % (w, h, sub, dri))
            subs.append(sub)
    return files, what, subs


@pytest.mark.parametrize("upsampling", ["replicate", "fancy"])
@pytest.mark.parametrize("denom", sm.DENOMS)
def test_every_layout_equals_the_model_and_pillow(denom, upsampling):
    files, what, subs = _value_files()
    b = _decode(files, denom, upsampling=upsampling)
    stats = b.plan_stats()
    assert stats["idct_work"] == [0] * len(stats["idct_work"]) and stats["idct_listed_mcus"] == 0  # (no K3 list names a scan K3R takes)
    for i, f in enumerate(files):
        assert b.upsampling(i) == (1 if upsampling == "fancy" and sm.filters(f, denom) else 0), what[i]
        _check(b, i, f, denom, "%s at 1/%d, %s" % (what[i], denom, upsampling), upsampling, pillow=upsampling == "fancy" and subs[i] in PILLOW_RATIOS)
    b.close()


def test_widths_1_to_8_give_one_pixel_at_an_eighth():
    files = [_file(w, 9 - w, sub, 75, 0, seed=w) for w in range(1, 9) for sub in ("gray", "420")]
    b = _decode(files, 8, upsampling="fancy")
    for i, f in enumerate(files):
        assert b.window(i) == (0, 0, 1, 1)
        _check(b, i, f, 8, "file %d" % i, "fancy", pillow=True)
    b.close()


@pytest.mark.parametrize("denom", sm.DENOMS)
def test_block_rows_around_a_workgroups_256_blocks(denom):
    files = [_file(688, 16, "420", 75, 4, seed=31), _file(688, 8, "444", 75, 0, seed=32), _file(2056, 8, "gray", 75, 0, seed=5)]  # 43 and 86 MCUs, 257 blocks
    b = _decode(files, denom, upsampling="fancy")
    for i, f in enumerate(files):
        _check(b, i, f, denom, "file %d at 1/%d" % (i, denom), "fancy", pillow=True)
    b.close()


@pytest.mark.parametrize("fmt", [jl.FMT_RGB_U8, jl.FMT_RGBA_U8, jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_PLANAR_F32],
                         ids=["rgb_u8", "rgba_u8", "planar_u8", "planar_f16", "planar_f32"])
def test_the_five_rgb_formats(fmt):
    files = [_file(33, 17, "422", 75, 4, seed=27), _file(24, 17, "420", 75, 0, seed=25), _file(9, 9, "gray", 75, 0, seed=20)]
    consts = jl.affine_from_mean_std([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]) if fmt in (jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_PLANAR_F32) else None
    for denom in sm.DENOMS:
        b = _decode(files, denom, fmt, consts=consts, upsampling="fancy")
        for i, f in enumerate(files):
            assert b.result(i).status == 0 and b.scale(i) == denom
            _assert_bits(b.output(i), cm.as_format(_model(f, denom, "fancy"), fmt, consts), "file %d at 1/%d" % (i, denom))
        b.close()


def test_which_pictures_are_filtered():
    f422, f420, f440 = _file(33, 17, "422", 75, 4, seed=27), _file(24, 17, "420", 75, 0, seed=25), _file(8, 16, "440", 75, 0, seed=29)
    for denom in sm.DENOMS:
        b = _decode([f422, f420, f440], denom, upsampling="fancy")
        assert [b.upsampling(i) for i in range(3)] == [int(denom < 8), 0, int(denom < 8)], denom  # (4:2:0 has no ratio left; no filter at 1/8)
        rep = _decode([f422], denom)
        assert (b.output(0).tobytes() != rep.output(0).tobytes()) == (denom < 8)
        rep.close()
        b.close()


def test_progressive_and_three_scan_files():
    files = [_file(33, 17, "420", 75, 0, seed=9, progressive=True), _file(33, 17, "420", 75, 0, seed=10, noninterleaved=True),
             _file(33, 17, "420", 75, 4, seed=11, noninterleaved=True), _file(33, 17, "422", 75, 0, seed=12, progressive=True),
             _file(17, 13, "gray", 75, 0, seed=13, progressive=True), _file(33, 17, "422", 75, 0, seed=14, noninterleaved=True)]
    try:
        from test_libjpeg_cpu import pillow_file
        files.append(pillow_file(33, 17, 2, 75, progressive=True))
        files.append(pillow_file(33, 17, 1, 75, progressive=True))
    except ImportError:
        pass
    for denom in sm.DENOMS:
        b = _decode(files, denom, upsampling="fancy")
        for i, f in enumerate(files):
            _check(b, i, f, denom, "file %d at 1/%d" % (i, denom), "fancy", pillow=i >= 6)
        b.close()


# ------------------------------------------------------------------------------------------------ 2: composition

def test_windows_are_slices_of_the_reduced_picture():
    f = _file(47, 31, "422", 75, 4, seed=12)
    wide = _file(688, 16, "420", 75, 4, seed=31)  # 43 MCUs per row, 16 per workgroup: seams at reduced pixels 128 m, 256 m
    for denom in (2, 4):
        m = 8 // denom
        W, H = sm.out_size(47, 31, denom)
        windows = [(0, 0, 0, 0), (1, 1, W - 2, H - 2), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (3, 1, 5, 3), (W, 0, 1, 1)]
        for upsampling in ("replicate", "fancy"):
            b = _decode([f] * len(windows), denom, upsampling=upsampling, windows=windows)
            whole = cm.as_format(_model(f, denom, upsampling), FMT)
            _assert_bits(b.output(0), whole, "whole")
            for i, (x, y, w, h) in enumerate(windows[1:-1], 1):
                assert b.result(i).status == 0 and b.scale(i) == denom and b.window(i) == (x, y, w, h), i
                _assert_bits(b.output(i), np.ascontiguousarray(whole[:, y:y + h, x:x + w]), "window %r at 1/%d, %s" % (windows[i], denom, upsampling))
            assert b.image_info(len(windows) - 1).status == _capi.ERR_ARGUMENT and b.scale(len(windows) - 1) == 1  # (outside the REDUCED frame: fails alone)
            b.close()
        seam = [(0, 0, 0, 0), (16 * 2 * m - 1, 1, 3, 2 * m - 1), (16 * 2 * m - 3, 0, 16 * 2 * m + 7, 2 * m), (32 * 2 * m, 1, 5, 1)]
        b = _decode([wide] * len(seam), denom, windows=seam)
        whole = cm.as_format(_model(wide, denom), FMT)
        for i, (x, y, w, h) in enumerate(seam[1:], 1):
            _assert_bits(b.output(i), np.ascontiguousarray(whole[:, y:y + h, x:x + w]), "seam window %r at 1/%d" % (seam[i], denom))
        b.close()


@pytest.mark.parametrize("size", [(17, 9), (130, 70)], ids=["17x9", "130x70"])
def test_orientations_turn_the_reduced_picture(size):
    f = _file(size[0], size[1], "422", 75, 4, seed=40)
    for denom in sm.DENOMS:
        for upsampling in ("replicate", "fancy"):
            stored = cm.as_format(_model(f, denom, upsampling), FMT)
            b = _decode([f] * 8, denom, upsampling=upsampling, orientations=list(range(1, 9)))
            for i, o in enumerate(range(1, 9)):
                assert b.result(i).status == 0 and b.orientation(i) == o and b.scale(i) == denom
                _assert_bits(b.output(i), om.orient_output(o, stored, FMT), "orientation %d at 1/%d, %s" % (o, denom, upsampling))
            b.close()


def test_gray_gives_component_0s_reduced_samples():
    f, g = _file(47, 31, "420", 75, 4, seed=12), _file(17, 13, "gray", 75, 0, seed=2)
    for denom in sm.DENOMS:
        W, H = sm.out_size(47, 31, denom)
        win = (1, 1, W - 2, H - 1)
        b = _decode([f, g, f], denom, mode="gray", upsampling="fancy", windows=[(0, 0, 0, 0), (0, 0, 0, 0), win])
        assert b.luma_work() == (0, 3) and [b.scale(i) for i in range(3)] == [denom] * 3
        _assert_bits(b.output(0), lm.plane("ycbcr", sm.samples(f, denom)), "4:2:0")
        _assert_bits(b.output(1), lm.plane("gray", sm.samples(g, denom)), "grey")
        _assert_bits(b.output(2), lm.plane("ycbcr", sm.samples(f, denom), win), "window")
        p = sm.pillow_draft(g, denom, "L")
        if p is not None:
            _assert_bits(b.output(1), p[None], "Pillow's L of a grey file")
        b.close()


def test_cmyk_ycck_and_adobe_rgb_files_under_the_colour_policy():
    pytest.importorskip("PIL")  # (color_model builds these files with Pillow)
    names = ("cmyk", "ycck", "rgb_adobe")
    files = [cm.kind_file(n)[0] for n in names] + [cm.subsampled_ycck()]
    kinds = [cm.kind_file(n)[1] for n in names] + ["ycck"]
    for denom in sm.DENOMS:
        b = _decode(files, denom, color="file", upsampling="fancy")
        for i, f in enumerate(files):
            assert b.result(i).status == 0 and b.scale(i) == denom and b.color(i) == kinds[i] and b.upsampling(i) == 0, i
            _assert_bits(b.output(i), cm.as_format(im.rgb(kinds[i], sm.samples(f, denom)), FMT), "%s at 1/%d" % (kinds[i], denom))
        b.close()


# ------------------------------------------------------------------------------------------------ 3: failing files and mixed batches

def test_a_truncated_and_a_corrupted_file_leave_zero_blocks_where_k3j_leaves_them():
    base = _file(136, 96, "gray", 75, 4, seed=4)
    cut = base[:len(base) * 6 // 10] + b"\xff\xd9"
    sos = base.index(b"\xff\xda")
    flipped = bytearray(base)
    for at in range(sos + 200, sos + 206):
        flipped[at] ^= 0x5A
    for f in (cut, bytes(flipped)):
        full = _decode([f], 1)
        assert full.result(0).status != 0 and full.image_info(0).status == 0
        y = full.output(0)[0]  # R = G = B = Y of a grey file
        zero = (y.reshape(12, 8, 17, 8) == 0).all(axis=(1, 3))  # the blocks K3J left zero
        assert zero.any() and not zero.all()
        coefs = full.coefficients(0)
        for denom in sm.DENOMS:
            m = 8 // denom
            b = _decode([f], denom)
            ra, rb = full.result(0), b.result(0)
            assert (ra.status, ra.detail, ra.error_block, ra.decoded_mcus) == (rb.status, rb.detail, rb.error_block, rb.decoded_mcus) and b.scale(0) == denom
            want = sm.samples(f, denom, blocks=coefs)[..., 0].copy()
            want[np.repeat(np.repeat(zero, m, axis=0), m, axis=1)] = 0
            _assert_bits(b.output(0), np.repeat(want[None], 3, axis=0), "at 1/%d" % denom)
            b.close()
        full.close()


def test_a_failing_progressive_file_reports_as_at_full_size_and_leaves_its_neighbour_alone():
    """its scans are issued a second time, literally (no transform is listed for a reduced image then): the statuses are the full-size
    decode's, the picture has the reduced size, and the good image beside it is the model's"""
    pytest.importorskip("PIL")
    from test_libjpeg_cpu import pillow_file

    good = _file(33, 17, "420", 75, 0, seed=9, progressive=True)
    bad = bytearray(pillow_file(47, 31, 1, 75, progressive=True))
    sos = [k for k in range(len(bad) - 1) if bad[k] == 0xFF and bad[k + 1] == 0xDA]
    for at in range(sos[2] + 40, sos[2] + 44):  # inside the third scan's entropy data: "Invalid Huffman code encountered." in the reference
        bad[at] ^= 0x5A
    bad = bytes(bad)
    full = _decode([bad, good], 1)
    ra = full.result(0)
    assert ra.status != 0 and full.image_info(0).status == 0 and full.progressive_replays() >= 1
    for denom in sm.DENOMS:
        b = _decode([bad, good], denom)
        rb = b.result(0)
        assert (ra.status, ra.detail, ra.error_block, ra.decoded_mcus) == (rb.status, rb.detail, rb.error_block, rb.decoded_mcus), denom
        assert b.progressive_replays() == full.progressive_replays()
        assert b.scale(0) == denom and b.output(0).shape == (3,) + sm.out_size(47, 31, denom)[::-1]
        _check(b, 1, good, denom, "the good file beside it at 1/%d" % denom)
        b.close()
    full.close()


def test_a_mixed_batch_keeps_full_size_for_what_does_not_take_the_transform():
    twelve = cm.patch_precision(_file(33, 17, "420", 75, 0, seed=7), 12)
    base = _file(136, 96, "420", 75, 4, seed=4)
    cut = base[:len(base) * 6 // 10] + b"\xff\xd9"
    odd = bytes(jpegsynth.encode(70, 33, "444", 75, 3, seed=44, sampling=((2, 1), (4, 1), (1, 1))))  # keeps the float transform
    files = [_file(33, 17, "422", 75, 4, seed=27), twelve, cut, _file(24, 17, "420", 75, 0, seed=25), odd, _file(9, 9, "gray", 75, 0, seed=20)]
    for denom in (2, 8):
        b = _decode(files, denom, upsampling="fancy")
        ref = _decode(files, 1, upsampling="fancy")
        assert [b.scale(i) for i in range(len(files))] == [denom, 1, denom, denom, 1, denom]
        assert b.image_info(1).status != 0 and b.arithmetic(1) == 0  # the 12-bit file: refused under an RGB format as ever
        assert b.result(2).status != 0 and b.result(2).status == ref.result(2).status
        assert b.arithmetic(4) == 0 and b.result(4).status == 0 and b.window(4) == (0, 0, 70, 33)
        _assert_bits(b.output(4), ref.output(4), "the odd layout comes out full size, as without a scale")
        _assert_bits(b.output(4), pm.expected(odd, arithmetic="libjpeg", scale=denom, upsampling="fancy", color="ycc", mode="rgb", orientation=1, window=None, fmt=FMT, consts=None, resize=None).output, "the odd layout against the composed model")
        for i in (0, 3, 5):
            solo = _decode([files[i]], denom, upsampling="fancy")
            _assert_bits(b.output(i), solo.output(0), "image %d against its solo decode" % i)
            _assert_bits(b.output(i), cm.as_format(_model(files[i], denom, "fancy"), FMT), "image %d against the model" % i)
            solo.close()
        ref.close()
        b.close()
    # a 12-bit file that does decode (a sample format) reports 1 and full size under a scale policy
    s = jl.Batch().set_arithmetic_policy("libjpeg").set_scale_policy(4).upload([twelve, files[0]], jl.FMT_INTERLEAVED_U8_SCALED).decode().sync()
    assert [s.scale(i) for i in range(2)] == [1, 1] and s.image_info(0).status == 0 and s.window(0) == (0, 0, 33, 17)
    s.close()


def _fit_rule(w, h, min_w, min_h):
    k = min(w // min_w, h // min_h)
    return 8 if k >= 8 else 4 if k >= 4 else 2 if k >= 2 else 1


def test_the_fit_rule_on_a_ragged_set():
    sizes = [(9, 9), (16, 16), (31, 33), (64, 20), (65, 130), (127, 128), (128, 64), (300, 200), (200, 300), (255, 257)]
    files = [_file(w, h, ("420", "422", "gray", "444")[k % 4], 75, (0, 4)[k & 1], seed=60 + k) for k, (w, h) in enumerate(sizes)]
    for orientation in (1, 6):
        for fit in ((16, 16), (32, 8), (7, 40)):  # (h, w)
            b = _decode(files, 1, upsampling="fancy", fit=fit, orientations=[orientation] * len(files))
            for i, ((w, h), f) in enumerate(zip(sizes, files)):
                ow, oh = (h, w) if orientation == 6 else (w, h)
                denom = _fit_rule(ow, oh, fit[1], fit[0])
                assert b.scale(i) == denom and b.result(i).status == 0, (i, fit, orientation, b.scale(i), denom)
                stored = cm.as_format(_model(f, denom, "fancy"), FMT)
                _assert_bits(b.output(i), om.orient_output(orientation, stored, FMT), "file %d, fit %r, orientation %d" % (i, fit, orientation))
            b.close()
    b = jl.Batch().set_arithmetic_policy("libjpeg").set_scale_policy(2).set_scale_fit((16, 16)).set_scale_fit(None).upload(files[:3], FMT).decode().sync()
    assert [b.scale(i) for i in range(3)] == [2, 2, 2]  # (switched off: the policy holds again)
    assert _capi.lib.jpgpu_batch_set_scale_fit(b._h, 0, 5) == _capi.ERR_ARGUMENT
    b.close()


def test_decode_resized_resamples_the_reduced_picture():
    files = [_file(300, 200, "420", 75, 4, seed=67), _file(64, 20, "422", 75, 0, seed=63), _file(9, 9, "gray", 75, 0, seed=20)]
    for scale in (1, 2, 4, 8):
        out, results = jl.decode_resized(files, (7, 5), upsampling="fancy", arithmetic="libjpeg", scale=scale)
        assert tuple(out.shape) == (3, 3, 7, 5) and [r.status for r in results] == [0, 0, 0]
        for i, f in enumerate(files):
            planes = cm.as_format(_model(f, scale, "fancy"), FMT)
            _assert_bits(out.cpu().numpy()[i], rm.model(planes, 7, 5, np.float16), "file %d at 1/%d" % (i, scale))
    out, results = jl.decode_resized(files, (32, 32), dtype=torch.float32, upsampling="fancy", arithmetic="libjpeg", scale="fit")
    assert tuple(out.shape) == (3, 3, 32, 32) and [r.status for r in results] == [0, 0, 0]
    for i, (f, (w, h)) in enumerate(zip(files, [(300, 200), (64, 20), (9, 9)])):
        planes = cm.as_format(_model(f, _fit_rule(w, h, 32, 32), "fancy"), FMT)
        _assert_bits(out.cpu().numpy()[i], rm.model(planes, 32, 32, np.float32), "file %d under fit" % i)
    t, results = jl.decode_to_tensors(files[:1], arithmetic="libjpeg", upsampling="fancy", scale=4)
    assert results[0].status == 0 and tuple(t[0].shape) == (3, 50, 75)
    p = sm.pillow_draft(files[0], 4, "RGB")
    if p is not None:
        _assert_bits(t[0].cpu().numpy(), cm.as_format(p, FMT), "decode_to_tensors against Pillow's draft")


# ------------------------------------------------------------------------------------------------ 4: hygiene

def _bytes(b, i):
    o = b.output(i)
    return [p.tobytes() for p in (o if isinstance(o, list) else [o])]


def _same(a, b, n, what):
    assert a.plan_stats()["idct_work"] == b.plan_stats()["idct_work"] and a.plan_stats()["idct_listed_mcus"] == b.plan_stats()["idct_listed_mcus"], what
    for i in range(n):
        ia, ib = a.image_info(i), b.image_info(i)
        assert (ia.status, ia.width, ia.height, ia.out_bytes, ia.out_offset) == (ib.status, ib.width, ib.height, ib.out_bytes, ib.out_offset), (what, i)
        assert b.scale(i) == 1 and a.result(i).status == b.result(i).status and a.arithmetic(i) == b.arithmetic(i), (what, i)
        if ia.status == 0:
            assert a.window(i) == b.window(i) and _bytes(a, i) == _bytes(b, i), (what, i)


def test_without_a_scale_nothing_changes():
    base = _file(136, 96, "420", 75, 4, seed=4)
    files = [_file(33, 17, "422", 75, 4, seed=27), _file(24, 17, "420", 75, 0, seed=25), _file(9, 9, "gray", 75, 0, seed=20),
             _file(33, 17, "420", 75, 0, seed=9, progressive=True), base[:len(base) * 6 // 10] + b"\xff\xd9"]
    n = len(files)
    for fmt, arithmetic in ((FMT, "libjpeg"), (FMT, "reference"), (jl.FMT_RGB_U8, "reference"), (jl.FMT_INTERLEAVED_U8, "libjpeg"), (jl.FMT_PLANAR_U8, "libjpeg")):
        untouched = jl.Batch().set_arithmetic_policy(arithmetic).upload(files, fmt).decode().sync()
        one = jl.Batch().set_arithmetic_policy(arithmetic).set_scale_policy(1).upload(files, fmt).decode().sync()
        _same(untouched, one, n, "policy 1, format %d, %s" % (fmt, arithmetic))
        one.close()
        if fmt != FMT or arithmetic != "libjpeg":  # a scale set where the arithmetic policy is not read: at the C level, the helpers refuse it
            eight = jl.Batch().set_arithmetic_policy(arithmetic)
            assert _capi.lib.jpgpu_batch_set_scale_policy(eight._h, 8) == 0 and _capi.lib.jpgpu_batch_set_scale_fit(eight._h, 2, 2) == 0
            eight.upload(files, fmt).decode().sync()
            _same(untouched, eight, n, "policy 8 and a fit rule, format %d, %s" % (fmt, arithmetic))
            eight.close()
        untouched.close()


def test_the_policy_is_state_of_the_batch_and_a_bad_value_is_refused():
    f = _file(33, 17, "422", 75, 4, seed=27)
    b = jl.Batch().set_arithmetic_policy("libjpeg")
    for bad in (0, 3, 16, -2):
        assert _capi.lib.jpgpu_batch_set_scale_policy(b._h, bad) == _capi.ERR_ARGUMENT
    with pytest.raises(ValueError):
        b.set_scale_policy(3)
    b.upload([f], FMT).decode().sync()
    assert b.scale(0) == 1
    b.set_scale_policy(4)
    for _ in range(2):  # it holds for every later upload
        b.upload([f], FMT).decode().sync()
        assert b.scale(0) == 4
        _assert_bits(b.output(0), cm.as_format(_model(f, 4), FMT), "under the policy")
    assert _capi.lib.jpgpu_batch_set_scale_policy(b._h, 5) == _capi.ERR_ARGUMENT  # (a refusal leaves it as it is)
    b.set_arithmetic_policy("reference").upload([f], FMT).decode().sync()
    assert b.scale(0) == 1 and b.window(0) == (0, 0, 33, 17)
    b.set_arithmetic_policy("libjpeg").set_scale_policy(1).upload([f], FMT).decode().sync()
    assert b.scale(0) == 1
    _assert_bits(b.output(0), cm.as_format(_model(f, 1), FMT), "set back")
    assert _capi.lib.jpgpu_batch_image_scale(b._h, 0, None) == _capi.ERR_ARGUMENT
    with pytest.raises(jl.ArgumentException):
        b.scale(1)  # (no such image)
    b.close()
