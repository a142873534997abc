"""Windows (jpgpu_batch_set_windows): every image of a batch decoded through a rectangle of its frame.  The oracle is the decoder itself:
a window's output is, byte for byte, the slice [y : y + h, x : x + w] of what the same files give without windows in the same test -- the
existing suites pin that to the reference.  Covered: the five layout classes under every whole-pixel format; windows that are aligned,
free in y, unaligned, one MCU, one pixel, one line, one MCU column; which class the planner picks and how many MCUs K3 lists; both
hand-off forms; progressive frames, their partial flush, a baseline file cut short, multi-scan baseline files; mixed batches; the
one-shot rule; the refusals; the torch hand-over."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from jpeglibrary_amd.errors import ArgumentException
from test_planar_rgb_gpu import _progressive_file
from test_split_handoff_gpu import SMALL
from tools import jpegsynth

pytestmark = pytest.mark.gpu

GENERIC, H1V1, H2V1, H2V2, GRAY, SAMPLES = range(6)
CLASS_OF = {"444": H1V1, "422": H2V1, "420": H2V2, "gray": GRAY}
MCU = {"444": (8, 8), "422": (16, 8), "420": (16, 16), "gray": (8, 8)}  # pixels of an MCU: width, height
PLANES = (jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_PLANAR_F32)
FAST_FORMATS = PLANES + (jl.FMT_RGB_U8,)  # the formats whose fast classes have a window form
FORMATS = FAST_FORMATS + (jl.FMT_RGBA_U8, jl.FMT_INTERLEAVED_U8, jl.FMT_INTERLEAVED_U8_SCALED)
FMT_IDS = {jl.FMT_RGB_PLANAR_U8: "planar_u8", jl.FMT_RGB_PLANAR_F16: "planar_f16", jl.FMT_RGB_PLANAR_F32: "planar_f32", jl.FMT_RGB_U8: "rgb",
           jl.FMT_RGBA_U8: "rgba", jl.FMT_INTERLEAVED_U8: "ycc", jl.FMT_INTERLEAVED_U8_SCALED: "ycc_scaled"}
AFFINE = jl.affine_from_mean_std((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))  # (only RGB_PLANAR_F16 reads it here)
ERR_ARGUMENT = 4

FRAMES = [(256, 160, "420"), (256, 160, "422"), (256, 160, "444"), (256, 160, "gray"), (250, 150, "420")]


def _windows(W, H):
    """the matrix's windows for a W x H frame (the issue's figures for 256 x 160; the frame-relative ones follow a smaller frame)"""
    return [(0, 0, 0, 0), (0, 0, W, H), (32, 16, 128, 96), (32, 19, 128, 83), (37, 19, 101, 83), (240, 144, W - 240, H - 144), (W - 1, H - 1, 1, 1),
            (0, 0, W, 1), (16, 0, 16, H)]


assert _windows(256, 160)[5:] == [(240, 144, 16, 16), (255, 159, 1, 1), (0, 0, 256, 1), (16, 0, 16, 160)]

_FILES = {}


def _file(w, h, sub, dri, seed=None, **kw):
    key = (w, h, sub, dri, seed, tuple(sorted(kw.items())))
    if key not in _FILES:
        _FILES[key] = bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=seed if seed is not None else w + h + dri, **kw))
    return _FILES[key]


def _decode(files, fmt, windows=None):
    b = jl.Batch()
    if fmt == jl.FMT_RGB_PLANAR_F16:
        b.set_output_affine(*AFFINE)
    if windows is not None:
        b.set_windows(windows)
    return b.upload(files, fmt).decode().sync()


def _slice(full, fmt, rect):
    x, y, w, h = rect
    return full[:, y:y + h, x:x + w] if fmt in PLANES else full[y:y + h, x:x + w]


def _fields(s):
    return tuple(getattr(s, k) for k, _ in s._fields_)


def _assert_window_of(whole, wi, win, i, fmt, rect):
    """image i of the windowed batch `win` against image wi of the unwindowed batch `whole`: geometry, result, window, pixels"""
    a, b = whole.image_info(wi), win.image_info(i)
    if a.status != 0:  # an image whose headers fail keeps the status it has without windows
        assert (b.status, b.detail, b.out_bytes) == (a.status, a.detail, 0) and _fields(win.result(i)) == _fields(whole.result(wi)), (i, rect)
        return
    W, H = a.width, a.height
    x, y, w, h = rect if rect != (0, 0, 0, 0) else (0, 0, W, H)
    assert (b.status, b.width, b.height, b.num_components, b.total_blocks) == (0, W, H, a.num_components, a.total_blocks), (i, rect)
    assert win.window(i) == (x, y, w, h), (i, rect)
    assert b.out_offset % 256 == 0
    if fmt in PLANES:
        size = np.dtype({jl.FMT_RGB_PLANAR_F16: np.float16, jl.FMT_RGB_PLANAR_F32: np.float32}.get(fmt, np.uint8)).itemsize
        assert b.out_bytes == 3 * w * h * size, (i, rect)
        assert [(p.offset, p.width, p.height, p.pitch) for p in b.plane][:3] == [(c * w * h * size, w, h, w) for c in range(3)], (i, rect)
    else:
        channels = {jl.FMT_RGB_U8: 3, jl.FMT_RGBA_U8: 4}.get(fmt, a.num_components)
        assert b.out_bytes == w * h * channels, (i, rect)
    assert _fields(win.result(i)) == _fields(whole.result(wi)), (i, rect)
    got, want = win.output(i), np.ascontiguousarray(_slice(whole.output(wi), fmt, (x, y, w, h)))
    assert got.shape == want.shape and got.dtype == want.dtype, (i, rect, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))
        raise AssertionError("image %d, window %r: %d bytes differ, the first at %d" % (i, rect, len(bad), bad[0][0]))


def _check(files, fmt, windows):
    """files[i] through windows[i] against the same files without windows -> (the unwindowed batch, the windowed one)"""
    distinct = list(dict.fromkeys(files))
    whole, win = _decode(distinct, fmt), _decode(files, fmt, windows)
    assert len(win) == len(files)
    for i, (f, rect) in enumerate(zip(files, windows)):
        _assert_window_of(whole, distinct.index(f), win, i, fmt, rect)
    return whole, win


# ------------------------------------------------------------------------------------------------ 1: the matrix

@pytest.mark.parametrize("fmt", FORMATS, ids=[FMT_IDS[f] for f in FORMATS])
def test_every_window_of_every_layout_class(fmt):
    files, windows = [], []
    for (w, h, sub) in FRAMES:
        for dri in (0, 3):
            for rect in _windows(w, h):
                files.append(_file(w, h, sub, dri))
                windows.append(rect)
    _check(files, fmt, windows)


# ------------------------------------------------------------------------------------------------ 2: classes and work

def _cover(rect, sub):
    x, y, w, h = rect
    mw, mh = MCU[sub]
    return (-(-(x + w) // mw) - x // mw) * (-(-(y + h) // mh) - y // mh)


@pytest.mark.parametrize("fmt", FAST_FORMATS, ids=[FMT_IDS[f] for f in FAST_FORMATS])
def test_aligned_windows_take_their_fast_class_and_list_their_cover(fmt):
    for (w, h, sub) in FRAMES:
        mw, mh = MCU[sub]
        f = _file(w, h, sub, 3)
        grid = -(-w // mw) * -(-h // mh)
        b = jl.Batch().upload([f], fmt)
        whole_class = CLASS_OF[sub] if w % mw == 0 else GENERIC
        stats = b.plan_stats()
        assert stats["idct_listed_mcus"] == grid and [c for c in range(6) if stats["idct_work"][c]] == [whole_class], (w, h, sub, stats)
        for rect in _windows(w, h):
            x, y, ww, hh = rect
            stats = b.set_windows([rect]).upload([f], fmt).plan_stats()
            if rect in ((0, 0, 0, 0), (0, 0, w, h)):
                want_class, want_mcus = whole_class, grid
            else:
                want_class, want_mcus = (CLASS_OF[sub] if x % mw == 0 and ww % mw == 0 else GENERIC), _cover(rect, sub)
            assert [c for c in range(6) if stats["idct_work"][c]] == [want_class], (w, h, sub, rect, stats)
            assert stats["idct_listed_mcus"] == want_mcus, (w, h, sub, rect, stats)
            assert sum(stats["idct_split_work"]) == 0 or rect in ((0, 0, 0, 0), (0, 0, w, h)), (rect, stats)
    # ... and summed over a batch
    files = [_file(w, h, sub, 3) for (w, h, sub) in FRAMES]
    rects = [(32, 16, 128, 96), (32, 19, 128, 83), (37, 19, 101, 83), (0, 0, 0, 0), (16, 0, 16, 150)]
    stats = jl.Batch().set_windows(rects).upload(files, fmt).plan_stats()
    assert stats["idct_listed_mcus"] == sum(_cover(r if r != (0, 0, 0, 0) else (0, 0, w, h), sub) for r, (w, h, sub) in zip(rects, FRAMES)), stats
    stats = jl.Batch().upload(files, fmt).plan_stats()
    assert stats["idct_listed_mcus"] == sum(-(-w // MCU[sub][0]) * -(-h // MCU[sub][1]) for (w, h, sub) in FRAMES), stats


def test_the_other_formats_take_the_generic_class_under_a_window():
    for fmt in (jl.FMT_RGBA_U8, jl.FMT_INTERLEAVED_U8, jl.FMT_INTERLEAVED_U8_SCALED):
        for (w, h, sub) in FRAMES[:4]:
            stats = jl.Batch().set_windows([(32, 16, 128, 96)]).upload([_file(w, h, sub, 3)], fmt).plan_stats()
            assert [c for c in range(6) if stats["idct_work"][c]] == [GENERIC] and stats["idct_listed_mcus"] == _cover((32, 16, 128, 96), sub), (fmt, sub, stats)


# ------------------------------------------------------------------------------------------------ 3: both hand-off forms

@pytest.mark.parametrize("dense", ["0", "1"], ids=["split", "dense"])
def test_the_split_handoff_shapes_under_windows(dense, monkeypatch):
    monkeypatch.setenv("JPGPU_DENSE_HANDOFF", dense)
    files = [bytes(jpegsynth.encode(w, h, sub, q, dri, seed=s)) for (w, h, sub, dri) in SMALL for q, s in ((75, 11), (97, 12))]
    shapes = [(w, h) for (w, h, sub, dri) in SMALL for _ in range(2)]
    whole, win = _check(files, jl.FMT_RGB_PLANAR_U8, [(16, 8, w - 32, h - 11) for (w, h) in shapes])  # aligned, free in y and height
    assert (sum(whole.plan_stats()["idct_split_work"]) > 0) == (dense == "0")  # (the unwindowed twin really is handed over split)
    assert sum(win.plan_stats()["idct_split_work"]) == 0 and win.plan_stats()["idct_work"][GENERIC] == 0, win.plan_stats()
    _, win = _check(files, jl.FMT_RGB_PLANAR_U8, [(5, 3, w - 9, h - 7) for (w, h) in shapes])  # unaligned
    assert win.plan_stats()["idct_work"] == [win.plan_stats()["idct_work"][GENERIC], 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 4: other frame kinds

def _two_windows(f):
    info = jl.Batch().upload([f], jl.FMT_INTERLEAVED_U8).image_info(0)
    W, H = (info.width, info.height) if info.status == 0 else (64, 48)  # (a file that fails at upload: any window)
    return [(16, 3, (W - 16) // 16 * 16, H - 7), (5, 3, W - 9, H - 7), (W - 1, H - 1, 1, 1)]


@pytest.mark.parametrize("fmt", [jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_U8, jl.FMT_INTERLEAVED_U8], ids=["planar_u8", "rgb", "ycc"])
def test_progressive_cut_and_multi_scan_files(fmt):
    prog = _progressive_file()
    base = _file(256, 160, "420", 3)
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stress")
    kinds = {
        "progressive": prog,
        # Cut at 60 % of their length.  As they are, Identify() walks into the end of the data and both files fail at upload, with no output
        # in either run; with the EOI kept, as the other suites cut their files, the scans run: the progressive file takes the partial
        # flush, and the baseline file's unreached samples are zero in both runs.
        "progressive cut at 60 %": prog[:len(prog) * 6 // 10],
        "baseline cut at 60 %": base[:len(base) * 6 // 10],
        "progressive cut at 60 %, EOI kept": prog[:len(prog) * 6 // 10] + b"\xff\xd9",
        "baseline cut at 60 %, EOI kept": base[:len(base) * 6 // 10] + b"\xff\xd9",
        "non-interleaved": _file(96, 64, "444", 0, seed=5, noninterleaved=True),
        "non-interleaved, restart intervals": _file(120, 88, "444", 4, seed=9, noninterleaved=True),
        "a later scan of one component": open(os.path.join(golden, "baseline_overlapping_scans_a_later_scan_of_one_component.jpg"), "rb").read(),
        "a later scan cut short": open(os.path.join(golden, "baseline_overlapping_scans_b_later_scan_cut_short.jpg"), "rb").read(),
    }
    files, windows = [], []
    for f in kinds.values():
        for rect in _two_windows(f):
            files.append(f)
            windows.append(rect)
    whole, win = _check(files, fmt, windows)
    statuses = {name: whole.result(i).status for i, name in enumerate(kinds)}
    assert statuses["progressive"] == 0 and all(statuses[k] != 0 for k in kinds if "cut at" in k), statuses
    infos = {name: whole.image_info(i) for i, name in enumerate(kinds)}
    assert all(infos[k].status == 0 and infos[k].out_bytes > 0 for k in kinds if "EOI kept" in k), {k: v.status for k, v in infos.items()}
    assert win.progressive_replays() == whole.progressive_replays() >= 1  # (the partial flush was issued, under windows too)


# ------------------------------------------------------------------------------------------------ 5: a mixed batch

@pytest.mark.parametrize("fmt", [jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_U8, jl.FMT_INTERLEAVED_U8_SCALED], ids=["planar_f16", "rgb", "ycc_scaled"])
def test_windowed_and_whole_images_in_one_upload_in_two_orders(fmt):
    files, windows = [], []
    for k, (w, h, sub) in enumerate(FRAMES):
        f = _file(w, h, sub, 3 * (k & 1))
        for rect in ((0, 0, 0, 0), (32, 19, 128, 83), (37, 19, 101, 83)):
            files.append(f)
            windows.append(rect)
    for order in (range(len(files)), reversed(range(len(files)))):
        order = list(order)
        fs, ws = [files[k] for k in order], [windows[k] for k in order]
        whole, win = _check(fs, fmt, ws)
        if fmt in FAST_FORMATS:
            assert all(n > 0 for n in win.plan_stats()["idct_work"][:5]), win.plan_stats()
        # one image's window leaves its frame: that image alone fails
        ws2 = list(ws)
        ws2[4] = (200, 100, 100, 10)
        bad = _decode(fs, fmt, ws2)
        info = bad.image_info(4)
        assert (info.status, info.detail, info.out_bytes) == (ERR_ARGUMENT, 0, 0)
        assert (bad.result(4).status, bad.result(4).detail) == (ERR_ARGUMENT, 0)
        distinct = list(dict.fromkeys(fs))
        for i in (3, 5):
            _assert_window_of(whole, distinct.index(fs[i]), bad, i, fmt, ws2[i])
    # exactly one of width and height zero fails the image too
    bad = _decode(files[:2], fmt, [(0, 0, 16, 0), (8, 8, 0, 16)])
    assert [bad.image_info(i).status for i in range(2)] == [ERR_ARGUMENT] * 2


# ------------------------------------------------------------------------------------------------ 6: one-shot windows

def test_windows_are_consumed_by_one_upload():
    f = _file(256, 160, "420", 3)
    b = jl.Batch().set_windows([(32, 16, 128, 96)]).upload([f], jl.FMT_RGB_PLANAR_U8).decode().sync()
    assert b.output(0).shape == (3, 96, 128) and b.window(0) == (32, 16, 128, 96)
    small = b.output(0)
    b.upload([f], jl.FMT_RGB_PLANAR_U8).decode().sync()  # no set_windows: a whole frame again
    assert b.window(0) == (0, 0, 256, 160) and b.output(0).shape == (3, 160, 256)
    assert np.array_equal(b.output(0)[:, 16:112, 32:160], small)
    # withdrawn windows, and windows a refused upload consumed
    b.set_windows([(32, 16, 128, 96)]).set_windows(None).upload([f], jl.FMT_RGB_PLANAR_U8)
    assert b.window(0) == (0, 0, 256, 160)
    with pytest.raises(ArgumentException):
        b.set_windows([(32, 16, 128, 96)]).upload([f, f], jl.FMT_RGB_PLANAR_U8)
    assert len(b) == 0
    b.upload([f, f], jl.FMT_RGB_PLANAR_U8)
    assert len(b) == 2 and b.window(1) == (0, 0, 256, 160)


# ------------------------------------------------------------------------------------------------ 7: refusals

def test_refusals_of_the_whole_call():
    f = _file(256, 160, "420", 3)
    b = jl.Batch().upload([f], jl.FMT_RGB_PLANAR_U8)
    assert len(b) == 1
    rect = (_capi.Rect * 1)(_capi.Rect(32, 16, 128, 96))
    assert _capi.lib.jpgpu_batch_set_windows(None, rect, 1) == ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_set_windows(b._h, rect, -1) == ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_set_windows(b._h, None, 1) == ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_set_windows(b._h, None, 0) == 0
    for fmt in (jl.FMT_PLANAR_U8, jl.FMT_PLANAR_I16, jl.FMT_EXTENDED_U16):
        b.upload([f], jl.FMT_RGB_PLANAR_U8)
        with pytest.raises(ArgumentException):
            b.set_windows([(32, 16, 128, 96)]).upload([f], fmt)
        assert len(b) == 0, fmt
    b.upload([f], jl.FMT_RGB_PLANAR_U8)
    with pytest.raises(ArgumentException):  # count mismatch
        b.set_windows([(32, 16, 128, 96)] * 2).upload([f], jl.FMT_RGB_PLANAR_U8)
    assert len(b) == 0
    b.upload([f], jl.FMT_RGB_PLANAR_U8)
    frames = [{"width": 16, "height": 16, "precision": 8, "components": [(1, 1, 1, 0)]}]
    with pytest.raises(ArgumentException):
        b.set_windows([(0, 0, 8, 8)]).upload_frames(frames, np.ones((1, 4, 64), dtype=np.uint16), jl.FMT_INTERLEAVED_U8)
    assert len(b) == 0
    b.upload_frames(frames, np.ones((1, 4, 64), dtype=np.uint16), jl.FMT_INTERLEAVED_U8)  # (and consumed by the refusal)
    assert len(b) == 1 and b.window(0) == (0, 0, 16, 16)


# ------------------------------------------------------------------------------------------------ 8: the torch hand-over

def test_decode_to_tensors_under_windows():
    torch = pytest.importorskip("torch")
    files = [_file(w, h, sub, 3) for (w, h, sub) in FRAMES]
    windows = [(32, 16, 128, 96), (32, 19, 128, 83), (37, 19, 101, 83), (0, 0, 0, 0), (16, 0, 16, 150)]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    whole, _ = jl.decode_to_tensors(files, dtype=torch.float16, mean=mean, std=std)
    tensors, results = jl.decode_to_tensors(files, dtype=torch.float16, mean=mean, std=std, windows=windows)
    for i, (t, rect) in enumerate(zip(tensors, windows)):
        x, y, w, h = rect if rect != (0, 0, 0, 0) else (0, 0, FRAMES[i][0], FRAMES[i][1])
        assert results[i].status == 0 and t.dtype == torch.float16 and tuple(t.shape) == (3, h, w) and t.is_contiguous(), (i, t.shape)
        assert torch.equal(t.view(torch.int16), whole[i][:, y:y + h, x:x + w].contiguous().view(torch.int16)), i
    # data_ptr() == base + out_offset, and files given as device tensors give the same pixels
    dev = [torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda() for f in files]
    b = jl.Batch().set_output_affine(*jl.affine_from_mean_std(mean, std)).set_windows(windows).upload_tensors(dev, jl.FMT_RGB_PLANAR_F16).decode().sync()
    base, _ = b.output_device_ptr()
    for i, t in enumerate(tensors):
        d = b.output_tensor(i)
        assert d.data_ptr() == base + b.image_info(i).out_offset and tuple(d.shape) == tuple(t.shape)
        assert torch.equal(d.view(torch.int16), t.view(torch.int16)), i
