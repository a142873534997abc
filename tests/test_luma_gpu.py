"""Grey output on the GPU: mode="gray" / Batch.set_channels_policy("gray") over RGB_PLANAR_U8 / _F16 / _F32 (include/jpgpu.h, "Grey output").

Every comparison is bit for bit.  For the kinds GRAY and YCBCR the expected plane is channel 0 of the FMT_INTERLEAVED_U8 decode of the same files
with the same windows and partial-flush setting (the parity suite pins that path to the oracle; one file is compared to the oracle here as
well); for CMYK, YCCK and Adobe-RGB files it is tests/luma_model.py over those samples.  Batch.luma_work() is asserted in every case, so that no
case of the fast road (K3Y's luma_idct_kernel) passes by falling to the scratch road (luma_plane_kernel) or the other way round."""
import os

import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from tools import jpegsynth
import color_model as cm
import luma_model as lm
import orient_model as om
import policy_model as pm
import resize_model as rm
from test_color_gpu import _assert_bits
from test_planar_rgb_gpu import _progressive_file

pytestmark = pytest.mark.gpu

ERR_ARGUMENT = _capi.ERR_ARGUMENT
NP = {jl.FMT_RGB_PLANAR_U8: np.uint8, jl.FMT_RGB_PLANAR_F16: np.float16, jl.FMT_RGB_PLANAR_F32: np.float32}
CONSTS = (np.array([-0.75, 1.5, 0.003], np.float32), np.array([100.25, -3.5, 0.1], np.float32))  # (only [0] is read under "gray")
S420, S422, S444 = ((2, 2), (1, 1), (1, 1)), ((2, 1), (1, 1), (1, 1)), ((1, 1), (1, 1), (1, 1))
S411, S440 = ((4, 1), (1, 1), (1, 1)), ((1, 2), (1, 1), (1, 1))
# (w, h, sampling or "gray"): the shapes of the fast road -- one MCU, partial edges both ways, widths that are no multiple of 8, every chroma layout
FAST = [(8, 8, S444), (16, 16, S420), (16, 8, S422), (32, 8, S411), (8, 16, S440), (9, 9, "gray"), (24, 17, S420), (500, 375, S420),
        (1048, 40, S420),                   # 131 luma blocks per row: a row crosses waves and workgroups, several block rows
        (40, 24, ((2, 2), (1, 1), (1, 1))),  # 2 x 2 luma over 1 x 1 chroma
        (40, 24, ((2, 1), (1, 2), (1, 2)))]  # (2, 1) luma beside (1, 2) chroma: the chroma factors are ignored, the luma rows repeated
_FILES, _SAMPLES = {}, {}


def _file(w, h, sampling, seed=0, dri=0, **kw):
    key = (w, h, sampling, seed, dri, tuple(sorted(kw.items())))
    if key not in _FILES:
        if sampling == "gray":
            _FILES[key] = bytes(jpegsynth.encode(w, h, "gray", 85, dri, seed=seed, **kw))
        else:
            _FILES[key] = bytes(jpegsynth.encode(w, h, "444", 85, dri, seed=seed, sampling=sampling, **kw))
    return _FILES[key]


def _samples(files, partial_flush=True, windows=None):
    """(status, INTERLEAVED_U8 output or None) of every file under the default policies, through the same windows; whole frames are decoded once"""
    if windows is None:
        missing = [f for f in dict.fromkeys(files) if (f, partial_flush) not in _SAMPLES]
        if missing:
            b = jl.Batch()
            b.set_partial_flush(partial_flush)
            b.upload(missing, jl.FMT_INTERLEAVED_U8).decode().sync()
            for i, f in enumerate(missing):
                st = b.result(i).status
                _SAMPLES[(f, partial_flush)] = (st, b.output(i) if b.image_info(i).status == 0 else None)
            b.close()
        return [_SAMPLES[(f, partial_flush)] for f in files]
    b = jl.Batch()
    b.set_partial_flush(partial_flush)
    b.set_windows(windows)
    b.upload(files, jl.FMT_INTERLEAVED_U8).decode().sync()
    out = [(b.result(i).status, b.output(i) if b.image_info(i).status == 0 else None) for i in range(len(files))]
    b.close()
    return out


def _gray(files, fmt=jl.FMT_RGB_PLANAR_U8, consts=None, windows=None, orientation="stored", orientations=None, color="ycc", upsampling="replicate",
          partial_flush=True, mode="gray"):
    b = jl.Batch().set_color_policy(color).set_orientation_policy(orientation).set_upsampling_policy(upsampling).set_channels_policy(mode)
    b.set_partial_flush(partial_flush)
    if consts is not None:
        b.set_output_affine(*consts)
    if orientations is not None:
        b.set_orientations(orientations)
    if windows is not None:
        b.set_windows(windows)
    return b.upload(files, fmt).decode().sync()


def _check_plan(b, i, w, h, fmt=jl.FMT_RGB_PLANAR_U8):
    info = b.image_info(i)
    size = np.dtype(NP[fmt]).itemsize
    assert b.channels(i) == 1 and b.upsampling(i) == 0, i
    assert info.out_bytes == w * h * size and info.out_offset % 256 == 0, (i, info.out_bytes, info.out_offset)
    assert [(p.offset, p.width, p.height, p.pitch) for p in info.plane][:3] == [(0, w, h, w), (0, 0, 0, 0), (0, 0, 0, 0)], i


def _check_channel0(b, files, what, fmt=jl.FMT_RGB_PLANAR_U8, consts=None, windows=None, partial_flush=True):
    ref = _samples(files, partial_flush, windows)
    for i in range(len(files)):
        st, s = ref[i]
        assert b.result(i).status == st, (what[i], b.result(i).status, st)
        if s is None:
            assert b.image_info(i).status != 0, what[i]
            continue
        want = lm.as_dtype(np.ascontiguousarray(s[..., 0])[None], NP[fmt], *((consts[0][0], consts[1][0]) if consts is not None else ()))
        _check_plan(b, i, s.shape[1], s.shape[0], fmt)
        _assert_bits(b.output(i), want, what[i])


# ------------------------------------------------------------------------------------------------ 1: the fast road

def _fast_files():
    files, what = [], []
    for dri in (0, 4):
        for k, (w, h, samp) in enumerate(FAST):
            files.append(_file(w, h, samp, seed=k, dri=dri))
            what.append("%dx%d %s dri %d" % (w, h, samp, dri))
    return files, what


@pytest.mark.parametrize("fmt", list(NP), ids=["u8", "f16", "f32"])
def test_every_shape_of_the_fast_road(fmt):
    files, what = _fast_files()
    consts = None if fmt == jl.FMT_RGB_PLANAR_U8 else CONSTS
    b = _gray(files, fmt, consts)
    assert b.luma_work() == (len(files), 0)
    stats = b.plan_stats()
    assert stats["idct_work"] == [0] * len(stats["idct_work"]) and stats["idct_listed_mcus"] == 0  # (no K3 list names a scan of the fast road)
    _check_channel0(b, files, what, fmt, consts)
    for i, f in enumerate(files):  # the tensor's shape, and the bytes it aliases
        t = b.output_tensor(i)
        assert tuple(t.shape) == b.output(i).shape and t.shape[0] == 1, what[i]
        assert t.cpu().numpy().tobytes() == b.output(i).tobytes(), what[i]
    b.close()


def test_one_file_straight_against_the_oracle_and_a_grey_file_against_todays_plane():
    from oracle import pyoracle

    f, g = _file(16, 16, S420, seed=1), _file(9, 9, "gray", seed=5)
    b = _gray([f, g])
    assert b.luma_work() == (2, 0)
    want, _ = pyoracle.decode_8bit(f)
    _assert_bits(b.output(0), np.ascontiguousarray(want[..., 0])[None], "16x16 4:2:0 against the oracle")
    for fmt, consts in ((jl.FMT_RGB_PLANAR_U8, None), (jl.FMT_RGB_PLANAR_F16, CONSTS), (jl.FMT_RGB_PLANAR_F32, CONSTS)):
        today = _gray([g], fmt, consts, mode="rgb")
        now = _gray([g], fmt, consts)
        assert today.channels(0) == 3 and today.output(0).shape == (3, 9, 9)
        _assert_bits(now.output(0), today.output(0)[:1], "a 1-component file: plane 0 of today's output")
        today.close()
        now.close()
    b.close()


WINDOWS = [(0, 0, 1, 1), (79, 47, 1, 1), (16, 0, 32, 48), (5, 3, 61, 40), (72, 40, 8, 8)]


@pytest.mark.parametrize("dri", [0, 4])
@pytest.mark.parametrize("fmt", list(NP), ids=["u8", "f16", "f32"])
def test_windows_on_the_fast_road_mixed_with_whole_frames(fmt, dri):
    f = _file(80, 48, S420, seed=3, dri=dri)
    files = [f] * len(WINDOWS) + [f, _file(24, 17, S420, seed=6, dri=dri)]
    windows = WINDOWS + [(0, 0, 0, 0), (0, 0, 0, 0)]
    consts = None if fmt == jl.FMT_RGB_PLANAR_U8 else CONSTS
    b = _gray(files, fmt, consts, windows=windows)
    assert b.luma_work() == (len(files), 0)
    whole = _samples([f])[0][1]
    for i, (x, y, w, h) in enumerate(WINDOWS):  # a window is that slice of the whole decode
        assert b.window(i) == (x, y, w, h)
        _assert_bits(b.output(i), lm.as_dtype(lm.plane("ycbcr", whole, (x, y, w, h)), NP[fmt], *((consts[0][0], consts[1][0]) if consts else ())), "window %r" % ((x, y, w, h),))
    _check_channel0(b, files, ["window %r" % (w,) for w in windows], fmt, consts, windows=windows)
    b.close()


def test_one_batch_of_seventy_mixed_files():
    shapes = [(8, 8, S444), (33, 17, S420), (16, 9, S422), (41, 8, S411), (9, 9, "gray"), (64, 64, S420), (7, 23, S440)]
    files, what = [], []
    for k in range(70):
        w, h, samp = shapes[k % len(shapes)]
        files.append(_file(w + k // 7, h + k % 5, samp, seed=k, dri=(0, 4, 1)[k % 3]))
        what.append("file %d" % k)
    b = _gray(files)
    assert b.luma_work() == (70, 0)
    offsets = [b.image_info(i).out_offset for i in range(70)]
    assert all(o % 256 == 0 for o in offsets) and all(b1 >= a + b.image_info(i).out_bytes for i, (a, b1) in enumerate(zip(offsets, offsets[1:])))
    _check_channel0(b, files, what)
    b.close()


def _failing(dri):
    whole = _file(120, 72, S420, seed=20 + dri, dri=dri)
    d = bytearray(whole)
    sos = d.index(b"\xff\xda")
    first = sos + 4 + d[sos + 3]
    cut = bytes(d[:first + (len(d) - first) // 2]) + b"\xff\xd9"  # truncated in the middle of its scan, EOI kept
    if dri == 0:  # a corrupted code: the stress corpus' file whose scan meets a code no table holds, late in its data (4:4:4, one scan)
        bad = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stress", "dri0_invalid_code_late.jpg"), "rb").read()
    else:         # three bytes of the scan flipped: the interval loses its place and the restart check fails
        bad = bytearray(whole)
        at = first + (len(d) - first) // 3
        for k in range(3):
            v = bad[at + 7 * k] ^ 0x5A
            bad[at + 7 * k] = v if v != 0xFF else 0x5A
    return [cut, bytes(bad), whole]


@pytest.mark.parametrize("partial_flush", [True, False], ids=["flush", "noflush"])
@pytest.mark.parametrize("dri", [0, 4])
def test_failing_files_leave_what_the_reference_decode_leaves(dri, partial_flush):
    files = _failing(dri)
    b = _gray(files, partial_flush=partial_flush)
    assert b.luma_work() == (3, 0)  # (all three are planned: they fail in their scans, on the device)
    ref = _samples(files, partial_flush)
    assert ref[0][0] != 0 and ref[1][0] != 0 and ref[2][0] == 0  # (the files do fail, and the comparison is not of zeros alone)
    for k in (0, 1):
        assert ref[k][1] is not None and ref[k][1][..., 0].any() and not ref[k][1][-1, -1, 0]
    _check_channel0(b, files, ["truncated", "corrupted", "whole"], partial_flush=partial_flush)
    b.close()


# ------------------------------------------------------------------------------------------------ 2: the scratch road

def _scratch_files():
    files = [_progressive_file(), _file(65, 67, S420, seed=41, progressive=True), _file(65, 67, S420, seed=40, noninterleaved=True),
             _file(67, 35, S422, seed=42, dri=4, noninterleaved=True),
             _file(70, 33, ((1, 1), (2, 2), (2, 2)), seed=43),           # the luma below the chroma: hs = vs = 2
             _file(70, 33, ((2, 1), (4, 1), (1, 1)), seed=44, dri=3)]    # component 0 at hs = 2 under a maximum of 4
    what = ["progressive (Pillow)", "progressive", "three scans", "three scans, dri 4", "luma below chroma", "luma hs 2 of 4"]
    return files, what


@pytest.mark.parametrize("fmt", list(NP), ids=["u8", "f16", "f32"])
def test_what_is_not_one_scan_at_the_maxima_takes_the_scratch_road(fmt):
    files, what = _scratch_files()
    consts = None if fmt == jl.FMT_RGB_PLANAR_U8 else CONSTS
    b = _gray(files, fmt, consts)
    assert b.luma_work() == (0, len(files))
    _check_channel0(b, files, what, fmt, consts)
    b.close()


KIND_FILES = ("cmyk", "ycck", "rgb_adobe")


def _kind_plane(name, window=None, orientation=1):
    f, kind = cm.kind_file(name)
    return lm.plane(kind, _samples([f])[0][1], window, orientation)


@pytest.mark.parametrize("fmt", list(NP), ids=["u8", "f16", "f32"])
def test_cmyk_ycck_and_adobe_rgb_files_give_l_of_their_rgb(fmt):
    files = [cm.kind_file(n)[0] for n in KIND_FILES] + [cm.subsampled_ycck()]
    consts = None if fmt == jl.FMT_RGB_PLANAR_U8 else CONSTS
    b = _gray(files, fmt, consts, color="file")
    assert b.luma_work() == (0, len(files))
    args = (consts[0][0], consts[1][0]) if consts else ()
    for i, n in enumerate(KIND_FILES):
        assert b.color(i) == cm.kind_file(n)[1]
        _check_plan(b, i, 45, 67, fmt)
        _assert_bits(b.output(i), lm.as_dtype(_kind_plane(n), NP[fmt], *args), n)
        _assert_bits(b.output(i), pm.expected(files[i], arithmetic="reference", scale=1, upsampling="replicate", color="file", mode="gray", orientation=1, window=None, fmt=fmt, consts=consts, resize=None).output, n + ", the composed model")
    _assert_bits(b.output(3), lm.as_dtype(lm.plane("ycck", _samples([files[3]])[0][1]), NP[fmt], *args), "sub-sampled YCCK")
    # the same files under the default colour policy: 4 components fail as ever, the Adobe-RGB file is YCbCr and gives component 0
    c = _gray(files[:3], fmt, consts)
    assert c.image_info(0).status != 0 and c.image_info(1).status != 0 and c.luma_work() == (1, 0)
    _assert_bits(c.output(2), lm.as_dtype(lm.plane("ycbcr", _samples([files[2]])[0][1]), NP[fmt], *args), "Adobe RGB under ycc")
    b.close()
    c.close()


@pytest.mark.parametrize("size", [(17, 9), (130, 70)], ids=["17x9", "130x70"])
@pytest.mark.parametrize("windowed", [False, True], ids=["whole", "window"])
def test_orientations_2_to_8_given_and_from_the_file(size, windowed):
    w, h = size
    ycc = _file(w, h, S420, seed=w, dri=4)
    cmyk = cm.kind_file("cmyk", w, h)[0]
    sy, sc = _samples([ycc])[0][1], _samples([cmyk])[0][1]
    files, given, windows, want = [], [], [], []
    for o in range(2, 9):
        ow, oh = (h, w) if o >= 5 else (w, h)
        win = (ow // 3, oh // 4, ow - ow // 3 - 1, oh - oh // 4 - 2) if windowed else None
        for f, s, kind in ((ycc, sy, "ycbcr"), (cmyk, sc, "cmyk")):
            files.append(f)
            given.append(o)
            windows.append(win if win else (0, 0, 0, 0))
            want.append(lm.plane(kind, s, win, o))
    for how in ("given", "file"):
        if how == "given":
            b = _gray(files, color="file", orientations=given, windows=windows if windowed else None)
        else:
            b = _gray([om.with_orientation(f, o, "MM" if o & 1 else "II") for f, o in zip(files, given)], color="file", orientation="file",
                      windows=windows if windowed else None)
        assert b.luma_work() == (0, len(files))
        for i in range(len(files)):
            assert b.result(i).status == 0 and b.orientation(i) == given[i], (how, i)
            _check_plan(b, i, want[i].shape[2], want[i].shape[1])
            _assert_bits(b.output(i), want[i], "%s: orientation %d, file %d" % (how, given[i], i))
        b.close()
    # float samples of a turned image: one case per type
    for fmt in (jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_PLANAR_F32):
        b = _gray(files[8:10], fmt, CONSTS, color="file", orientations=given[8:10], windows=windows[8:10] if windowed else None)
        for i in range(2):
            _assert_bits(b.output(i), lm.as_dtype(want[8 + i], NP[fmt], CONSTS[0][0], CONSTS[1][0]), "orientation 6, %s" % NP[fmt].__name__)
        b.close()


def test_a_batch_that_mixes_both_roads():
    fast, _ = _fast_files()
    slow, _ = _scratch_files()
    files = [f for pair in zip(fast[:6], slow) for f in pair] + [cm.kind_file("cmyk")[0], _file(33, 17, S420, seed=2)]
    orientations = [0] * 12 + [0, 6]
    b = _gray(files, color="file", orientations=orientations)
    assert b.luma_work() == (6, 8)  # (the turned 4:2:0 file takes the scratch road)
    _check_channel0(b, files[:12], ["mixed %d" % i for i in range(12)])
    _assert_bits(b.output(12), _kind_plane("cmyk"), "CMYK in the mixed batch")
    _assert_bits(b.output(13), lm.plane("ycbcr", _samples([files[13]])[0][1], None, 6), "turned 4:2:0 in the mixed batch")
    b.close()


# ------------------------------------------------------------------------------------------------ 3: the policy

def _same_batches(a, b, n):
    assert a.plan_stats()["idct_work"] == b.plan_stats()["idct_work"]
    for i in range(n):
        ia, ib = a.image_info(i), b.image_info(i)
        assert (ia.status, ia.width, ia.height, ia.out_bytes, ia.out_offset, ia.num_components) == (ib.status, ib.width, ib.height, ib.out_bytes, ib.out_offset, ib.num_components), i
        assert [(p.offset, p.width, p.height, p.pitch) for p in ia.plane] == [(p.offset, p.width, p.height, p.pitch) for p in ib.plane], i
        assert a.result(i).status == b.result(i).status
        if ia.status == 0:
            oa, ob = a.output(i), b.output(i)  # (PLANAR_U8: a list of planes)
            assert [p.tobytes() for p in (oa if isinstance(oa, list) else [oa])] == [p.tobytes() for p in (ob if isinstance(ob, list) else [ob])], i


@pytest.mark.parametrize("fmt,mode", [(jl.FMT_RGB_PLANAR_U8, "rgb"), (jl.FMT_RGB_PLANAR_F16, "rgb"), (jl.FMT_RGB_U8, "gray"), (jl.FMT_INTERLEAVED_U8, "gray"),
                                      (jl.FMT_RGBA_U8, "gray"), (jl.FMT_PLANAR_U8, "gray")],
                         ids=["planar_u8-unset", "planar_f16-unset", "rgb_u8-set", "interleaved-set", "rgba-set", "planar-set"])
def test_unset_or_on_a_format_that_does_not_read_it_nothing_changes(fmt, mode):
    files = _fast_files()[0][:11] + _scratch_files()[0] + _failing(4)[:2]
    untouched = jl.Batch().upload(files, fmt).decode().sync()
    b = jl.Batch().set_channels_policy(mode).upload(files, fmt).decode().sync()
    assert b.luma_work() == (0, 0) and all(b.channels(i) == 3 for i in range(len(files)))
    _same_batches(untouched, b, len(files))
    untouched.close()
    b.close()


def test_the_policy_is_state_of_the_batch_and_a_bad_value_is_refused():
    f = _file(24, 17, S420, seed=6)
    b = jl.Batch()
    for bad in (2, -1, 7):
        assert _capi.lib.jpgpu_batch_set_channels_policy(b._h, bad) == ERR_ARGUMENT
    with pytest.raises(ValueError):
        b.set_channels_policy("luma")
    b.set_channels_policy("gray")
    for _ in range(2):  # it holds for every later upload
        b.upload([f], jl.FMT_RGB_PLANAR_U8).decode().sync()
        assert b.channels(0) == 1 and b.output(0).shape == (1, 17, 24) and b.luma_work() == (1, 0)
    assert _capi.lib.jpgpu_batch_set_channels_policy(b._h, 5) == ERR_ARGUMENT  # (a refusal leaves it as it is)
    b.upload([f], jl.FMT_RGB_U8).decode().sync()
    assert b.channels(0) == 3 and b.output(0).shape == (17, 24, 3)
    b.set_channels_policy("rgb").upload([f], jl.FMT_RGB_PLANAR_U8).decode().sync()
    assert b.channels(0) == 3 and b.output(0).shape == (3, 17, 24) and b.luma_work() == (0, 0)
    assert _capi.lib.jpgpu_batch_image_channels(b._h, 0, None) == ERR_ARGUMENT and _capi.lib.jpgpu_batch_luma_work(b._h, None) == ERR_ARGUMENT
    with pytest.raises(jl.ArgumentException):
        b.channels(1)  # (no such image)
    b.close()


def test_fancy_upsampling_with_gray_changes_nothing():
    files = _fast_files()[0][:11] + _scratch_files()[0][:3] + [_file(33, 17, S420, seed=2)]
    orientations = [0] * 14 + [6]
    a = _gray(files, orientations=orientations)
    b = _gray(files, orientations=orientations, upsampling="fancy")
    assert a.luma_work() == b.luma_work() == (11, 4)
    assert all(b.upsampling(i) == 0 for i in range(len(files)))
    _same_batches(a, b, len(files))
    a.close()
    b.close()


def test_the_one_call_helpers():
    files = [_file(24, 17, S420, seed=6), _file(9, 9, "gray", seed=5), _failing(4)[0], cm.kind_file("cmyk")[0]]
    windows = [(3, 2, 20, 11), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    tensors, results = jl.decode_to_tensors(files, mode="gray", windows=windows, color="file", upsampling="fancy")
    outs, _ = jl.decode_batch(files, jl.FMT_RGB_PLANAR_U8, mode="gray", windows=windows, color="file")
    assert [r.status for r in results] == [0, 0, results[2].status, 0] and results[2].status != 0
    assert [tuple(t.shape) for t in (tensors[0], tensors[1], tensors[3])] == [(1, 11, 20), (1, 9, 9), (1, 67, 45)]
    assert tensors[0].dtype == torch.uint8 and tensors[0].cpu().numpy().tobytes() == outs[0].tobytes()
    _assert_bits(outs[0], lm.plane("ycbcr", _samples([files[0]])[0][1], windows[0]), "decode_batch, window")
    _assert_bits(outs[3], _kind_plane("cmyk"), "decode_batch, CMYK")
    mean, std = 0.45, [0.225]
    scale, bias = jl.affine_from_mean_std([mean] * 3, std * 3)
    for dtype in (torch.float16, torch.float32):
        t, _ = jl.decode_to_tensors(files[:2], dtype=dtype, mean=mean, std=std, mode="gray")
        for i in range(2):
            want = lm.as_dtype(lm.plane("ycbcr" if i == 0 else "gray", _samples([files[i]])[0][1]), NP[{torch.float16: jl.FMT_RGB_PLANAR_F16, torch.float32: jl.FMT_RGB_PLANAR_F32}[dtype]], scale[0], bias[0])
            assert t[i].dtype == dtype and tuple(t[i].shape) == want.shape
            _assert_bits(t[i].cpu().numpy(), want, "mean / std, %s" % dtype)


# ------------------------------------------------------------------------------------------------ 4: the resize stage on one plane

def _ragged():
    shapes = [(9, 9, "gray"), (24, 17, S420), (300, 200, S420), (130, 70, S422), (63, 65, S444), (41, 8, S411)]
    files = [_file(w, h, s, seed=30 + k, dri=(0, 4)[k & 1]) for k, (w, h, s) in enumerate(shapes)]
    files.insert(3, _failing(4)[0][:200])  # a file that fails at upload or in its scan: its slab is zeros
    files.append(_file(65, 67, S420, seed=41, progressive=True))
    windows = [(0, 0, 0, 0)] * len(files)
    windows[2] = (17, 30, 222, 133)
    windows[4] = (64, 3, 66, 67)
    return files, windows


def _gray_u8_planes(files, windows):
    b = _gray(files, windows=windows)
    planes = [b.output(i) if b.image_info(i).status == 0 and b.result(i).status == 0 else None for i in range(len(files))]
    b.close()
    return planes


@pytest.mark.parametrize("size", [(7, 5), (224, 224)], ids=["7x5", "224x224"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16], ids=["u8", "f16"])
def test_decode_resized_gray_is_the_resize_model_on_the_gray_plane(size, dtype):
    files, windows = _ragged()
    planes = _gray_u8_planes(files, windows)
    assert sum(p is None for p in planes) == 1
    kw = {} if dtype == torch.uint8 else {"mean": 0.45, "std": 0.225}
    t, results = jl.decode_resized(files, size, dtype=dtype, windows=windows, mode="gray", **kw)
    assert tuple(t.shape) == (len(files), 1, size[0], size[1]) and t.dtype == dtype
    got = t.cpu().numpy()
    npd = np.uint8 if dtype == torch.uint8 else np.float16
    consts = jl.affine_from_mean_std([0.45] * 3, [0.225] * 3) if kw else (None, None)
    for i, p in enumerate(planes):
        if p is None:
            assert results[i].status != 0 and not got[i].any(), i
            continue
        want = rm.model(np.repeat(p, 3, axis=0), size[0], size[1], npd, *consts)[:1]  # (the model takes three planes: the same function per plane)
        _assert_bits(got[i], want, "image %d at %r" % (i, size))


def test_resized_gray_of_a_grey_file_is_channel_0_of_todays_and_own_size_is_the_plain_decode():
    g = _file(9, 9, "gray", seed=5)
    today, _ = jl.decode_resized([g], (7, 5), mean=[0.45] * 3, std=[0.225] * 3)
    now, _ = jl.decode_resized([g], (7, 5), mean=0.45, std=0.225, mode="gray")
    assert tuple(today.shape) == (1, 3, 7, 5) and tuple(now.shape) == (1, 1, 7, 5)
    _assert_bits(now.cpu().numpy()[0], today.cpu().numpy()[0, :1], "a 1-component file")
    f = _file(24, 17, S420, seed=6)
    for dtype, fmt in ((torch.uint8, jl.FMT_RGB_PLANAR_U8), (torch.float16, jl.FMT_RGB_PLANAR_F16), (torch.float32, jl.FMT_RGB_PLANAR_F32)):
        kw = {} if dtype == torch.uint8 else {"mean": 0.45, "std": 0.225}
        t, _ = jl.decode_resized([f], (17, 24), dtype=dtype, mode="gray", **kw)
        plain, _ = jl.decode_to_tensors([f], dtype=dtype, mode="gray", **kw)
        _assert_bits(t.cpu().numpy()[0], plain[0].cpu().numpy(), "at its own size, %s" % dtype)
    # the batch interface: resized() downloads [N, 1, oh, ow]
    b = jl.Batch().set_channels_policy("gray").set_resize((5, 6))
    b.upload([f, g], jl.FMT_RGB_PLANAR_U8).decode().sync()
    assert b.resized().shape == (2, 1, 5, 6) and tuple(b.resized_tensor().shape) == (2, 1, 5, 6)
    assert b.resized().tobytes() == b.resized_tensor().cpu().numpy().tobytes()
    b.close()
