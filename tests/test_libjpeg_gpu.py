"""The arithmetic policy "libjpeg" on the GPU: jpeg_idct_islow in K3J and libjpeg's colour constants (include/jpgpu.h, "Arithmetic").

Every expected value is, bit for bit, tests/islow_model.py -- shown to be libjpeg's decode by tests/test_libjpeg_cpu.py -- over the oracle's
coefficients of the same file, and where Pillow decodes the file the way the policies ask (upsampling="fancy", a ratio K3U filters or no
sub-sampling at all) Pillow's convert("RGB") / "L" as well.  Covered: grey and YCbCr files of five sizes, five samplings, DRI 0 and 4, two
qualities, both upsamplings; RGB_U8 and RGBA_U8; block rows around a workgroup's 256 blocks and windows across its seams; sampling layouts
that take the byte-store way or keep the float transform; progressive and three-scan files; windows,
orientations, mode="gray", float samples and decode_resized on one file; CMYK, YCCK and Adobe-RGB files; hand-made coefficients up to the
extremes; a mixed batch with a truncated and a 12-bit file; and the policy's hygiene."""
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
import resize_model as rm
import upsample_model as um
from test_color_gpu import _assert_bits

pytestmark = pytest.mark.gpu

FMT = jl.FMT_RGB_PLANAR_U8
SIZES = [(1, 1), (8, 8), (17, 13), (33, 17), (136, 96)]
SAMPLING = {"444": ((1, 1), (1, 1), (1, 1)), "422": ((2, 1), (1, 1), (1, 1)), "420": ((2, 2), (1, 1), (1, 1)), "411": ((4, 1), (1, 1), (1, 1))}
PILLOW_RATIOS = ("gray", "444", "422", "420", "440")  # where upsampling="fancy" is libjpeg's default output
_FILES, _MODEL = {}, {}


def _file(w, h, sub, quality=75, dri=0, seed=0, **kw):
    key = (w, h, sub, quality, dri, seed, tuple(sorted(kw.items())))
    if key not in _FILES:
        if sub == "gray":
            f = jpegsynth.encode(w, h, "gray", quality, dri, seed=seed, **kw)
        elif sub == "440":  # a 4:2:2 file of the same MCU grid, its frame header patched: (Y, Y, Cb, Cr) per MCU either way
            f = um.patch_sof(bytes(jpegsynth.encode(-(-w // 8) * 16, -(-h // 16) * 8, "444", quality, dri, seed=seed, sampling=SAMPLING["422"], **kw)),
                             width=w, height=h, luma=0x12)
        else:
            f = jpegsynth.encode(w, h, "444", quality, dri, seed=seed, sampling=SAMPLING[sub], **kw)
        _FILES[key] = bytes(f)
    return _FILES[key]


def _model(f, upsampling="replicate", kind=None):
    """uint8[H, W, 3], computed once per (file, upsampling, kind)"""
    key = (f, upsampling, kind)
    if key not in _MODEL:
        _MODEL[key] = im.decode(f, upsampling, kind)
    return _MODEL[key]


def _decode(files, fmt=FMT, consts=None, upsampling="replicate", windows=None, orientations=None, color="ycc", mode="rgb", arithmetic="libjpeg",
            partial_flush=True):
    b = jl.Batch().set_color_policy(color).set_upsampling_policy(upsampling).set_channels_policy(mode).set_arithmetic_policy(arithmetic)
    b.set_partial_flush(partial_flush)
    if consts is not None:
        b.set_output_affine(*consts)
    if orientations is not None:
        b.set_orientations(orientations)
    if windows is not None:
        b.set_windows(windows)
    return b.upload(files, fmt).decode().sync()


def _check(b, i, f, what, upsampling="replicate", fmt=FMT, pillow=False):
    assert b.result(i).status == 0 and b.arithmetic(i) == 1, (what, b.result(i).status, b.arithmetic(i))
    want = _model(f, upsampling)
    _assert_bits(b.output(i), cm.as_format(want, fmt), what)
    if pillow:
        p = im.pillow_rgb(f)
        if p is not None:
            _assert_bits(b.output(i), cm.as_format(p, fmt), "Pillow: " + what)


# ------------------------------------------------------------------------------------------------ 1: values

def _value_files():
    files, what, subs = [], [], []
    for k, (w, h) in enumerate(SIZES):
        for sub in ("gray", "444", "422", "420", "440", "411"):
            for dri in (0, 4):
                for q in (25, 95):
                    files.append(_file(w, h, sub, q, dri, seed=k))
                    what.append("%dx%d %s dri %d Q%d" % (w, h, sub, dri, q))
                    subs.append(sub)
    return files, what, subs


@pytest.mark.parametrize("upsampling", ["replicate", "fancy"])
def test_grey_and_ycbcr_files_equal_the_model_and_pillow(upsampling):
    files, what, subs = _value_files()
    b = _decode(files, upsampling=upsampling)
    assert b.luma_work() == (0, 0)
    stats = b.plan_stats()
    assert stats["idct_work"] == [0] * len(stats["idct_work"]) and stats["idct_listed_mcus"] == 0  # (no K3 list names a scan K3J takes)
    other = 0
    for i, f in enumerate(files):
        assert b.upsampling(i) == (1 if upsampling == "fancy" and subs[i] != "gray" and um.qualifies(f) else 0), what[i]
        _check(b, i, f, what[i], upsampling, pillow=upsampling == "fancy" and subs[i] in PILLOW_RATIOS)
    ref = _decode(files, upsampling=upsampling, arithmetic="reference")
    for i in range(len(files)):
        assert ref.arithmetic(i) == 0
        other += ref.output(i).tobytes() != b.output(i).tobytes()
    assert other > len(files) // 2  # (the integer transform is another picture than the float one, on most files)
    ref.close()
    b.close()


@pytest.mark.parametrize("fmt", [jl.FMT_RGB_U8, jl.FMT_RGBA_U8], ids=["rgb_u8", "rgba_u8"])
def test_rgb_u8_and_rgba_u8(fmt):
    files = [_file(33, 17, "420", 95, 4, seed=3), _file(17, 13, "gray", 25, 0, seed=2)]
    for upsampling in ("replicate", "fancy"):
        b = _decode(files, fmt, upsampling=upsampling)
        for i, f in enumerate(files):
            _check(b, i, f, "file %d, %s" % (i, upsampling), upsampling, fmt, pillow=upsampling == "fancy")
        b.close()


def test_block_rows_around_a_workgroups_256_blocks():
    files = [_file(2056, 8, "gray", 75, 0, seed=5), _file(2040, 8, "gray", 75, 4, seed=6), _file(16, 640, "420", 75, 0, seed=7),
             _file(2056, 24, "444", 75, 4, seed=8)]  # 257 and 255 blocks per row; one MCU wide, 40 tall; 771 blocks per MCU row
    b = _decode(files, upsampling="fancy")
    for i, f in enumerate(files):
        _check(b, i, f, "file %d" % i, "fancy", pillow=True)
    b.close()


def test_windows_across_the_workgroups_seams_of_a_wide_file():
    f = _file(2056, 24, "444", 75, 4, seed=8)  # 257 MCUs per row: 85 per workgroup, seams at pixels 680, 1360, 2040
    windows = [(0, 0, 0, 0), (3, 1, 2050, 20), (679, 5, 3, 3), (680, 0, 681, 24), (1357, 7, 699, 9), (2039, 23, 17, 1), (1, 8, 2055, 8)]
    for upsampling in ("replicate", "fancy"):
        b = _decode([f] * len(windows), upsampling=upsampling, windows=windows)
        whole = cm.as_format(_model(f, upsampling), FMT)
        _assert_bits(b.output(0), whole, "whole")
        for i, (x, y, w, h) in enumerate(windows[1:], 1):
            assert b.result(i).status == 0 and b.arithmetic(i) == 1
            _assert_bits(b.output(i), np.ascontiguousarray(whole[:, y:y + h, x:x + w]), "window %r" % (windows[i],))
        b.close()


def test_layouts_no_encoder_here_defaults_to():
    """a strip that does not fit the staging (byte stores), unequal chroma factors, luma below chroma (the assembly with mixed replication) --
    and a layout whose blocks overlap in the reference, which keeps the float transform and takes libjpeg's constants all the same"""
    layouts = [((4, 2), (1, 1), (1, 1)), ((2, 2), (2, 1), (1, 1)), ((1, 1), (2, 2), (2, 2)), ((2, 2), (1, 2), (2, 1))]
    files = [bytes(jpegsynth.encode(70 + 3 * k, 33 + k, "444", 75, (0, 3)[k & 1], seed=50 + k, sampling=s)) for k, s in enumerate(layouts)]
    files += [bytes(jpegsynth.encode(2100, 40, "444", 75, 4, seed=60, sampling=layouts[0]))]  # three workgroups per MCU row on the byte-store way
    for upsampling in ("replicate", "fancy"):
        b = _decode(files, upsampling=upsampling)
        for i, f in enumerate(files):
            assert b.upsampling(i) == 0
            _check(b, i, f, "layout %d, %s" % (i, upsampling), upsampling)
        b.close()
    odd = bytes(jpegsynth.encode(70, 33, "444", 75, 3, seed=44, sampling=((2, 1), (4, 1), (1, 1))))  # component 0: two blocks per MCU line, each repeated twice
    b = _decode([odd])
    samples = jl.Batch().upload([odd], jl.FMT_INTERLEAVED_U8).decode().sync()
    assert b.result(0).status == 0 and b.arithmetic(0) == 0
    _assert_bits(b.output(0), cm.as_format(im.ycc_rgb(samples.output(0)), FMT), "the float transform under libjpeg's constants")
    samples.close()
    b.close()


def test_progressive_and_three_scan_files():
    files = [_file(33, 17, "420", 75, 0, seed=9, progressive=True), _file(33, 17, "420", 75, 0, seed=10, noninterleaved=True),
             _file(33, 17, "420", 75, 4, seed=11, noninterleaved=True)]
    try:
        from test_libjpeg_cpu import pillow_file
        files.append(pillow_file(33, 17, 2, 75, progressive=True))
    except ImportError:
        pass
    for upsampling in ("replicate", "fancy"):
        b = _decode(files, upsampling=upsampling)
        for i, f in enumerate(files):
            _check(b, i, f, "file %d, %s" % (i, upsampling), upsampling, pillow=upsampling == "fancy" and i == 3)
        b.close()


# ------------------------------------------------------------------------------------------------ 2: composition, on one 4:2:0 file of 47 x 31

W, H = 47, 31


def _one():
    return _file(W, H, "420", 75, 4, seed=12)


@pytest.mark.parametrize("upsampling", ["replicate", "fancy"])
def test_windows_are_slices_of_the_whole_decode(upsampling):
    f = _one()
    windows = [(0, 0, 0, 0), (5, 3, 41, 27), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (23, 15, 1, 1), (16, 16, 16, 15),
               (W - 29, H - 21, 29, 21), (1, 1, W - 1, H - 1), (31, 15, 3, 3), (7, 0, 40, 17), (W, 0, 1, 1)]
    b = _decode([f] * len(windows), upsampling=upsampling, windows=windows)
    whole = cm.as_format(_model(f, upsampling), FMT)
    _assert_bits(b.output(0), whole, "whole")
    for i, (x, y, w, h) in enumerate(windows[1:-1], 1):
        assert b.result(i).status == 0 and b.arithmetic(i) == 1 and b.window(i) == (x, y, w, h), i
        _assert_bits(b.output(i), np.ascontiguousarray(whole[:, y:y + h, x:x + w]), "window %r" % (windows[i],))
    assert b.image_info(len(windows) - 1).status == _capi.ERR_ARGUMENT and b.arithmetic(len(windows) - 1) == 0  # (fails alone)
    b.close()


@pytest.mark.parametrize("upsampling", ["replicate", "fancy"])
def test_orientations_turn_the_models_picture(upsampling):
    f = _one()
    stored = cm.as_format(_model(f, upsampling), FMT)
    b = _decode([f] * 8, upsampling=upsampling, orientations=list(range(1, 9)))
    for i, o in enumerate(range(1, 9)):
        assert b.result(i).status == 0 and b.orientation(i) == o and b.arithmetic(i) == 1
        _assert_bits(b.output(i), om.orient_output(o, stored, FMT), "orientation %d" % o)
    b.close()


def test_gray_gives_component_0s_islow_samples():
    f, g = _one(), _file(17, 13, "gray", 75, 0, seed=2)
    b = _decode([f, g, f], mode="gray", upsampling="fancy", windows=[(0, 0, 0, 0), (0, 0, 0, 0), (5, 3, 41, 27)])
    assert b.luma_work() == (0, 3)  # (never K3Y's fast road: that runs K3's transform)
    _assert_bits(b.output(0), lm.plane("ycbcr", im.samples(f)), "4:2:0")
    _assert_bits(b.output(1), lm.plane("gray", im.samples(g)), "grey")
    _assert_bits(b.output(2), lm.plane("ycbcr", im.samples(f), (5, 3, 41, 27)), "window")
    p = im.pillow_l(g)
    if p is not None:
        _assert_bits(b.output(1), p[None], "Pillow's L of a grey file")
    b.close()


def test_float16_with_mean_and_std_and_decode_resized():
    f = _one()
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    consts = jl.affine_from_mean_std(mean, std)
    for upsampling in ("replicate", "fancy"):
        planes = cm.as_format(_model(f, upsampling), FMT)
        t, results = jl.decode_to_tensors([f], dtype=torch.float16, mean=mean, std=std, upsampling=upsampling, arithmetic="libjpeg")
        assert results[0].status == 0 and t[0].dtype == torch.float16
        _assert_bits(t[0].cpu().numpy(), cm.as_format(_model(f, upsampling), jl.FMT_RGB_PLANAR_F16, consts), "float16, " + upsampling)
        out, results = jl.decode_resized([f], (8, 8), upsampling=upsampling, arithmetic="libjpeg")
        assert results[0].status == 0 and tuple(out.shape) == (1, 3, 8, 8)
        _assert_bits(out.cpu().numpy()[0], rm.model(planes, 8, 8, np.float16), "decode_resized, " + upsampling)
    outs, _ = jl.decode_batch([f], FMT, arithmetic="libjpeg")
    _assert_bits(outs[0], cm.as_format(_model(f), FMT), "decode_batch")
    p = im.pillow_rgb(f)
    if p is not None:
        t, _ = jl.decode_to_tensors([f], arithmetic="libjpeg", upsampling="fancy")
        _assert_bits(t[0].cpu().numpy(), cm.as_format(p, FMT), "decode_to_tensors against Pillow")


def test_cmyk_ycck_and_adobe_rgb_files_under_the_colour_policy():
    pytest.importorskip("PIL")  # (color_model builds these files with Pillow)
    names = ("cmyk", "ycck", "rgb_adobe")
    files = [cm.kind_file(n)[0] for n in names] + [cm.subsampled_ycck()]
    kinds = [cm.kind_file(n)[1] for n in names] + ["ycck"]
    b = _decode(files, color="file")
    for i, f in enumerate(files):
        assert b.result(i).status == 0 and b.arithmetic(i) == 1 and b.color(i) == kinds[i], i
        _assert_bits(b.output(i), cm.as_format(im.rgb(kinds[i], im.samples(f)), FMT), kinds[i])
    b.close()


# ------------------------------------------------------------------------------------------------ 3: hand-made coefficients

def test_coefficients_up_to_the_extremes_on_an_8x8_grey_file():
    f = _file(8, 8, "gray", 75, 0, seed=1)
    q = im.tables(f)[im.frame(f)[3][0][3]]
    blocks = np.zeros((6, 64), np.int16)
    blocks[0, 0], blocks[1, 0] = 1023, -1023
    blocks[2], blocks[3], blocks[4] = 32767, -32768, np.where(np.arange(64) & 1, -32768, 32767)
    blocks[5] = np.random.default_rng(3).integers(-32768, 32768, 64)
    b = jl.Batch().set_arithmetic_policy("libjpeg").upload([f] * len(blocks), FMT)
    for i in range(len(blocks)):
        assert b.image_info(i).status == 0 and b.image_info(i).total_blocks == 1 and b.arithmetic(i) == 1
        b.set_coefficients(i, blocks[i:i + 1])
    b.run_idct().sync()
    want = im.islow(blocks, q)
    assert (want[0] == 255).all() and (want[1] == 0).all()  # the clamp saturates: no wrapped value
    for i in range(len(blocks)):
        _assert_bits(b.output(i), np.repeat(want[i][None], 3, axis=0), "block %d" % i)
    b.close()


# ------------------------------------------------------------------------------------------------ 4: a mixed batch

def _mixed():
    good = [_file(33, 17, "420", 75, 4, seed=3), _file(17, 13, "gray", 25, 0, seed=2), _file(136, 96, "422", 95, 0, seed=4),
            _file(33, 17, "420", 75, 0, seed=9, progressive=True), _file(33, 17, "420", 75, 0, seed=10, noninterleaved=True), _file(17, 13, "411", 25, 4, seed=2),
            _file(17, 13, "440", 95, 0, seed=2), _file(2056, 8, "gray", 75, 0, seed=5), _file(8, 8, "444", 95, 4, seed=1)]
    base = _file(136, 96, "420", 75, 4, seed=4)
    cut = base[:len(base) * 6 // 10] + b"\xff\xd9"
    twelve = cm.patch_precision(_file(33, 17, "420", 75, 0, seed=7), 12)
    return good[:5] + [cut] + good[5:] + [twelve]


def test_a_mixed_batch_keeps_statuses_and_every_good_image_equals_its_solo_decode():
    files = _mixed()
    n = len(files)
    ref = _decode(files, upsampling="fancy", arithmetic="reference")
    b = _decode(files, upsampling="fancy")
    c = _decode(files, upsampling="fancy")  # (deterministic, the failing file included)
    for i in range(n):
        ra, rb = ref.result(i), b.result(i)
        assert (ref.image_info(i).status, ra.status, ra.detail, ra.error_block, ra.decoded_mcus) == (b.image_info(i).status, rb.status, rb.detail, rb.error_block, rb.decoded_mcus), i
        if b.image_info(i).status == 0:
            assert b.output(i).tobytes() == c.output(i).tobytes(), i
    assert b.result(5).status != 0 and b.arithmetic(5) == 1  # the truncated file is planned and fails in its scan
    assert b.image_info(n - 1).status != 0 and b.arithmetic(n - 1) == 0  # the 12-bit file: refused as ever, and not K3J's
    for i in [k for k in range(n) if k not in (5, n - 1)]:
        solo = _decode([files[i]], upsampling="fancy")
        assert b.arithmetic(i) == 1
        _assert_bits(b.output(i), solo.output(0), "image %d against its solo decode" % i)
        _assert_bits(b.output(i), cm.as_format(_model(files[i], "fancy"), FMT), "image %d against the model" % i)
        solo.close()
    for x in (ref, b, c):
        x.close()


# ------------------------------------------------------------------------------------------------ 5: hygiene

def _bytes(b, i):
    o = b.output(i)
    return [p.tobytes() for p in (o if isinstance(o, list) else [o])]


@pytest.mark.parametrize("fmt", range(10))
def test_the_default_and_reference_leave_every_formats_bytes_alone(fmt):
    files = _mixed()[:9]
    untouched = jl.Batch().upload(files, fmt).decode().sync()
    for policy in ("reference", None):
        b = jl.Batch()
        if policy:
            b.set_arithmetic_policy(policy)
        b.upload(files, fmt).decode().sync()
        assert b.plan_stats()["idct_work"] == untouched.plan_stats()["idct_work"]
        for i in range(len(files)):
            ia, ib = untouched.image_info(i), b.image_info(i)
            assert (ia.status, ia.out_bytes, ia.out_offset) == (ib.status, ib.out_bytes, ib.out_offset) and b.arithmetic(i) == 0, i
            assert untouched.result(i).status == b.result(i).status
            if ia.status == 0:
                assert _bytes(untouched, i) == _bytes(b, i), i
        b.close()
    untouched.close()


@pytest.mark.parametrize("fmt", [jl.FMT_INTERLEAVED_U8, jl.FMT_PLANAR_U8], ids=["interleaved", "planar"])
def test_the_sample_formats_ignore_the_policy(fmt):
    files = _mixed()[:9]
    untouched = jl.Batch().upload(files, fmt).decode().sync()
    b = jl.Batch().set_arithmetic_policy("libjpeg").upload(files, fmt).decode().sync()
    assert b.plan_stats()["idct_work"] == untouched.plan_stats()["idct_work"]
    for i in range(len(files)):
        assert b.arithmetic(i) == 0 and untouched.result(i).status == b.result(i).status
        if b.image_info(i).status == 0:
            assert _bytes(untouched, i) == _bytes(b, i), i
    untouched.close()
    b.close()


def test_the_policy_is_state_of_the_batch_and_a_bad_value_is_refused():
    f = _file(33, 17, "420", 75, 4, seed=3)
    want, plain = cm.as_format(_model(f), FMT), None
    b = jl.Batch()
    for bad in (2, -1, 7):
        assert _capi.lib.jpgpu_batch_set_arithmetic_policy(b._h, bad) == _capi.ERR_ARGUMENT
    with pytest.raises(ValueError):
        b.set_arithmetic_policy("islow")
    b.upload([f], FMT).decode().sync()
    plain = b.output(0).copy()
    assert b.arithmetic(0) == 0 and plain.tobytes() != want.tobytes()
    b.set_arithmetic_policy("libjpeg")
    for _ in range(2):  # it holds for every later upload
        b.upload([f], FMT).decode().sync()
        assert b.arithmetic(0) == 1 and b.luma_work() == (0, 0)
        _assert_bits(b.output(0), want, "under the policy")
    assert _capi.lib.jpgpu_batch_set_arithmetic_policy(b._h, 5) == _capi.ERR_ARGUMENT  # (a refusal leaves it as it is)
    b.upload([f], jl.FMT_INTERLEAVED_U8).decode().sync()
    assert b.arithmetic(0) == 0
    b.set_arithmetic_policy("reference").upload([f], FMT).decode().sync()
    assert b.arithmetic(0) == 0
    _assert_bits(b.output(0), plain, "set back")
    assert _capi.lib.jpgpu_batch_image_arithmetic(b._h, 0, None) == _capi.ERR_ARGUMENT
    with pytest.raises(jl.ArgumentException):
        b.arithmetic(1)  # (no such image)
    b.close()
