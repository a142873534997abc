"""The window of the lossless transform without a device (include/jpgpu.h section (5), "Window"): the model (tests/crop_model.py) against the
oracle, and the host side (jl.plan_transform(window=...), the C ABI's surface, the Python keyword arguments) against the model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import crop_cases as cc
import crop_model as cm
import jpeglibrary_amd as jl
import transform_model as tm
from golden_util import read_jpeg
from jpeglibrary_amd import _capi
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one orientation per class: none, a mirror in x, both mirrors, a mirror in y, the transposition, the two quarter turns, the anti-transposition
ORIENTATIONS = tuple(range(1, 9))


def _windows(name, o, edge):
    yield cc.interior_window(name, o, edge)
    yield cc.edge_window(name, o, edge)
    W, H, mw, mh = cc.geometry(name, o, edge)
    if W >= 2 * mw and H >= 2 * mh:
        yield cc.off_centre_window(name, o, edge)


def _edge_for(name, o):
    try:
        tm.plan(tm.frame_of(cc.make(name)), o, "refuse")
        return "refuse"
    except tm.Refused:
        return "trim"


# ---------------------------------------------------------------------------------------------- the model against the oracle
@pytest.mark.parametrize("name", cc.ALL)
def test_the_cropped_file_decodes_to_the_slice_of_the_turned_one(name):
    """The contract: decoding F'' gives, sample for sample, the slice of the decode of F'.  The bound is 0 -- the blocks are equal, and the
    reference's decoder works block by block -- and so are the decoded coefficients."""
    f = cc.make(name)
    coefs, _ = po.decode_coefficients(f)
    seen = 0
    for o in ORIENTATIONS:
        edge = _edge_for(name, o)
        try:
            whole = f if o == 1 else tm.write_turned(f, o, edge)
        except tm.Refused:  # (narrower than one MCU on a mirrored axis: nothing to trim to)
            continue
        pixels, _ = po.decode_8bit(whole)
        for x, y, w, h in _windows(name, o, edge):
            g = cm.write_cropped(f, o, edge, (x, y, w, h))
            out, info = po.decode_8bit(g)
            assert (info.width, info.height) == (w, h)
            assert np.array_equal(out, pixels[y:y + h, x:x + w]), (name, o, (x, y, w, h))
            blocks, _ = po.decode_coefficients(g)
            assert np.array_equal(blocks, cm.crop_blocks(coefs, tm.frame_of(f), o, edge, (x, y, w, h))), (name, o)
            seen += 1
    assert seen >= 8


def test_the_whole_frame_as_a_window_is_the_turned_file():
    for name in ("420_48x32", "420_40x27", "grey_20x16"):
        f = cc.make(name)
        fr = tm.frame_of(f)
        for o in (1, 5):
            pl = tm.plan(fr, o)
            assert cm.write_cropped(f, o, "refuse", (0, 0, pl["width"], pl["height"])) == tm.write_turned(f, o)


# ---------------------------------------------------------------------------------------------- planning
@pytest.mark.parametrize("name", cc.ALL)
def test_plan_transform_agrees_with_the_model(name):
    f = cc.make(name)
    fr = tm.frame_of(f)
    for o in ORIENTATIONS:
        edge = _edge_for(name, o)
        try:
            tm.plan(fr, o, edge)
        except tm.Refused:
            continue
        W, H, mw, mh = cc.geometry(name, o, edge)
        windows = list(_windows(name, o, edge)) + [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (min(3, W - 1), min(5, H - 1), 1, 1)]
        for window in windows:
            for origin in ("refuse", "expand"):
                try:
                    pl = cm.plan(fr, o, edge, window, origin)
                except cm.Refused as want:
                    with pytest.raises(jl.NotSupportedException) as e:
                        jl.plan_transform(f, orientations=[o], edge=edge, window=window, origin=origin)
                    coordinate = {"x": window[0], "y": window[1]}[want.axis]
                    size = {"x": mw, "y": mh}[want.axis]
                    assert "window's %s (%d)" % (want.axis, coordinate) in str(e.value) and "(%d pixels)" % size in str(e.value), str(e.value)
                    continue
                got = jl.plan_transform(f, orientations=[o], edge=edge, window=window, origin=origin)
                assert got == jl.TransformPlan(o, pl["width"], pl["height"], pl["trimmed"], pl["factors"], pl["window"]), (name, o, window, origin, got)
                assert got.window == pl["window"] and (got.width, got.height) == pl["window"][2:]


def test_applied_rects_sizes_and_every_refusal():
    f = cc.make("420_48x32")
    six = [(2, 2), (1, 1), (1, 1)]
    assert jl.plan_transform(f, window=(16, 16, 20, 9)) == jl.TransformPlan(1, 20, 9, False, six, (16, 16, 20, 9))
    assert jl.plan_transform(f, window=(20, 9, 20, 9), origin="expand") == jl.TransformPlan(1, 24, 18, False, six, (16, 0, 24, 18))
    assert jl.plan_transform(f, orientations=[6], window=(16, 32, 16, 16)) == jl.TransformPlan(6, 16, 16, False, six, (16, 32, 16, 16))
    f422 = cc.make("422_48x24")  # MCU 16 x 8; turned by 5..8 it is 8 x 16
    assert jl.plan_transform(f422, window=(16, 8, 5, 5)).window == (16, 8, 5, 5)
    assert jl.plan_transform(f422, orientations=[5], window=(8, 16, 5, 5)) == jl.TransformPlan(5, 5, 5, False, [(1, 2), (1, 1), (1, 1)], (8, 16, 5, 5))
    with pytest.raises(jl.NotSupportedException, match=r"window's x \(8\).*MCU width \(16 pixels\)"):
        jl.plan_transform(f422, window=(8, 8, 5, 5))
    with pytest.raises(jl.NotSupportedException, match=r"window's y \(8\).*MCU height \(16 pixels\)"):
        jl.plan_transform(f422, orientations=[5], window=(8, 8, 5, 5))
    assert jl.plan_transform(f422, orientations=[5], window=(9, 8, 5, 5), origin="expand").window == (8, 0, 6, 13)
    # outside the frame of F' (the turned one), a zero side: ArgumentException, whatever the origin policy
    for o, window, word in ((1, (32, 16, 17, 16), "outside"), (1, (0, 0, 48, 33), "outside"), (6, (0, 0, 48, 32), "outside"), (1, (2 ** 32 - 16, 0, 32, 8), "outside"),
                            (1, (48, 32, 1, 1), "outside"), (1, (0, 0, 16, 0), "zero"), (3, (16, 0, 0, 16), "zero"), (1, (5, 5, 0, 7), "zero")):
        for origin in ("refuse", "expand"):
            with pytest.raises(jl.ArgumentException, match=word):
                jl.plan_transform(f, orientations=[o], window=window, origin=origin)
            with pytest.raises(cm.BadWindow, match=word):
                cm.plan(tm.frame_of(f), o, "refuse", window, origin)
    assert jl.plan_transform(f, orientations=[6], window=(0, 0, 32, 48)).window == (0, 0, 32, 48)
    # the mirrored edge is resolved on the whole frame, before the window -- even where the window would leave that edge out
    g = cc.make("420_40x27")
    with pytest.raises(jl.NotSupportedException, match="width"):
        jl.plan_transform(g, orientations=[2], window=(0, 0, 16, 16))
    assert jl.plan_transform(g, orientations=[2], edge="trim", window=(16, 16, 16, 11)) == jl.TransformPlan(2, 16, 11, True, six, (16, 16, 16, 11))
    with pytest.raises(jl.ArgumentException, match="outside"):  # 32 wide behind the trim
        jl.plan_transform(g, orientations=[2], edge="trim", window=(32, 0, 8, 16))
    assert jl.plan_transform(g, window=(32, 16, 8, 11)).window == (32, 16, 8, 11)
    # an image with a window is refused for the reasons a turned one is
    with pytest.raises(jl.NotSupportedException, match="Progressive"):
        jl.plan_transform(read_jpeg("progress.jpg"), window=(0, 0, 8, 8))
    assert jl.plan_transform(read_jpeg("progress.jpg")).orientation == 1


def test_an_unwalkable_file_fails_with_a_window_and_is_left_alone_without_one():
    """plan_transform reports the header error either way; what differs is the upload's rule (tests/test_lossless_crop_gpu.py): without a
    window such a file "is not turned", with one the image fails.  Here: the error is the plan's, and it does not depend on the window."""
    for bad in (b"\xff\xd8\xff\xd9", cc.make("420_48x32")[:40], b"\x00" * 16):
        with pytest.raises(jl.InvalidDataException) as plain:
            jl.plan_transform(bad, orientations=[2])
        with pytest.raises(jl.InvalidDataException) as cut:
            jl.plan_transform(bad, window=(0, 0, 8, 8))
        assert str(plain.value) == str(cut.value)


# ---------------------------------------------------------------------------------------------- surface
def test_the_symbols_and_their_signatures():
    names = {name: (res, args) for name, res, args in _capi.SYMBOLS}
    P, R = C.c_void_p, C.POINTER(_capi.Rect)
    assert names["jpgpu_optimizer_set_origin_policy"] == (C.c_int, [P, C.c_int])
    assert names["jpgpu_optimizer_set_windows"] == (C.c_int, [P, R, C.c_int])
    assert names["jpgpu_optimizer_image_window"] == (C.c_int, [P, C.c_int, R])
    assert names["jpgpu_optimizer_turn_sources"] == (C.c_int, [P, C.POINTER(C.c_int)])
    assert names["jpgpu_transform_plan_window"] == (C.c_int, [P, C.c_size_t, C.c_int, C.c_int, C.c_int, R, C.c_int, C.POINTER(_capi.TransformInfo), R, C.c_char_p,
                                                             C.c_size_t])
    for name in ("jpgpu_optimizer_set_origin_policy", "jpgpu_optimizer_set_windows", "jpgpu_optimizer_image_window", "jpgpu_optimizer_turn_sources",
                 "jpgpu_transform_plan_window"):
        assert hasattr(_capi.lib, name), name
    assert _capi.lib.jpgpu_sizeof_rect() == C.sizeof(_capi.Rect) == 16
    assert _capi.lib.jpgpu_sizeof_transform_info() == C.sizeof(_capi.TransformInfo) == 32  # (unchanged)
    header = open(os.path.join(ROOT, "include", "jpgpu.h")).read()
    for word in ("JPGPU_ORIGIN_REFUSE = 0", "JPGPU_ORIGIN_EXPAND = 1", "jpgpu_origin_policy", "jpgpu_optimizer_set_windows(jpgpu_optimizer *o, const jpgpu_rect *windows, int n)",
                 "jpgpu_optimizer_image_window(const jpgpu_optimizer *o, int i, jpgpu_rect *applied)", "jpgpu_optimizer_turn_sources(const jpgpu_optimizer *o, int *files)",
                 "jpgpu_transform_plan_window(", "jpgpu_optimizer_set_origin_policy(jpgpu_optimizer *o, int origin)"):
        assert word in header, word
    assert "Not covered: cropping" not in header


def _fields(info):
    return (info.orientation, info.trimmed, info.width, info.height, info.num_components, bytes(info.h), bytes(info.v), info.reserved)


def test_a_null_or_zero_window_is_jpgpu_transform_plan():
    lib = _capi.lib
    files = [cc.make("420_40x27"), cc.make("422_48x24", 0, exif=6), read_jpeg("progress.jpg"), b"\xff\xd8\xff\xd9"]
    zero = _capi.Rect(0, 0, 0, 0)
    for f in files:
        buf = np.frombuffer(f, np.uint8)
        for o in (0, 1, 2, 6):
            for policy in (0, 1):
                for edge in (0, 1):
                    a, b, c = _capi.TransformInfo(), _capi.TransformInfo(), _capi.TransformInfo()
                    ma, mb, mc = (C.create_string_buffer(256) for _ in range(3))
                    applied = _capi.Rect(9, 9, 9, 9)
                    ra = lib.jpgpu_transform_plan(buf.ctypes.data, buf.size, o, policy, edge, C.byref(a), ma, 256)
                    rb = lib.jpgpu_transform_plan_window(buf.ctypes.data, buf.size, o, policy, edge, None, 1, C.byref(b), None, mb, 256)
                    rc = lib.jpgpu_transform_plan_window(buf.ctypes.data, buf.size, o, policy, edge, C.byref(zero), 0, C.byref(c), C.byref(applied), mc, 256)
                    assert ra == rb == rc and _fields(a) == _fields(b) == _fields(c) and ma.value == mb.value == mc.value, (len(f), o, policy, edge)
                    if ra == 0:
                        assert (applied.x, applied.y, applied.width, applied.height) == (0, 0, a.width, a.height)
    buf = np.frombuffer(files[0], np.uint8)
    info, msg, w = _capi.TransformInfo(), C.create_string_buffer(256), _capi.Rect(0, 0, 16, 16)
    assert lib.jpgpu_transform_plan_window(buf.ctypes.data, buf.size, 1, 0, 0, C.byref(w), 2, C.byref(info), None, msg, 256) == _capi.ERR_ARGUMENT
    assert lib.jpgpu_transform_plan_window(buf.ctypes.data, buf.size, 1, 0, 0, C.byref(w), 0, None, None, msg, 256) == _capi.ERR_ARGUMENT
    assert lib.jpgpu_transform_plan_window(buf.ctypes.data, buf.size, 1, 0, 0, C.byref(w), 0, C.byref(info), None, None, 0) == 0 and (info.width, info.height) == (16, 16)


def test_the_python_keyword_arguments_are_checked():
    f = cc.make("420_48x32")
    for bad in ((0, 0, 16), (0, 0, 16, -1), (0, 0, 16, 1.5), "abcd", (0, 0, 2 ** 32, 1), 7):
        with pytest.raises(ValueError):
            jl.plan_transform(f, window=bad)
        with pytest.raises(ValueError):  # optimize_batch checks its arguments before it asks for a device
            jl.optimize_batch([f], windows=[bad])
    with pytest.raises(ValueError):
        jl.plan_transform(f, window=(0, 0, 16, 16), origin="shrink")
    with pytest.raises(ValueError):
        jl.optimize_batch([f], windows=[(0, 0, 16, 16)], origin="shrink")
    with pytest.raises(ValueError):
        jl.optimize_batch([f, f], windows=[(0, 0, 16, 16)])
    with pytest.raises(ValueError):
        jl.optimize_batch([f], windows=[])
    with pytest.raises(ValueError):
        jl.optimize_batch([f], windows=[(0, 0, 16, 16)], edge="crop")  # (a window is not an edge policy)
    for method in ("set_windows", "set_origin_policy", "window", "turn_sources"):
        assert callable(getattr(jl.OptimizeBatch, method))
    assert jl.TransformPlan._fields == ("orientation", "width", "height", "trimmed", "factors", "window")
    assert jl.TransformPlan(1, 48, 32, False, []).window == (0, 0, 48, 32)


# ---------------------------------------------------------------------------------------------- the sanitizer harness
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_window_planning_code_is_clean_under_asan_and_ubsan(tmp_path):
    """tools/fuzz/crop_plan_asan.cpp: a stand-alone program over csrc/transform_plan.h (plan_transform with a window, the SOF patch of F'')"""
    exe = str(tmp_path / "crop_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=address,undefined",
                    "-I", os.path.join(ROOT, "jpeglibrary_amd", "csrc"), os.path.join(ROOT, "tools", "fuzz", "crop_plan_asan.cpp"),
                    os.path.join(ROOT, "jpeglibrary_amd", "csrc", "host_parser.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "crop plan ok: 4000 edits" in r.stdout and " 0 failures" in r.stdout
    cut = int(r.stdout.split("edits, ")[1].split()[0])
    assert cut >= 200, r.stdout  # (a harness whose windows are all refused would cover nothing)
