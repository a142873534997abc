"""The lossless transform without a device: the model (tests/transform_model.py) against the oracle, and the host side (jl.plan_transform,
the C ABI's surface, the Python keyword arguments) against the model."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeglibrary_amd as jl
import transform_cases as tc
import transform_model as tm
from jpeglibrary_amd import _capi
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIS = (0, 1, 2, 100)
FILES = [(name, dri) for name in tc.SHAPES for dri in (DRIS if name in ("420_48x32", "422_48x24") else (0,))]
# The largest absolute difference, over FILES and orientations 2..8 (edge "trim" where an axis is partial), between po.decode_8bit(F') and the
# numpy-turned po.decode_8bit(F).  The transform is exact in the coefficients; the reference's float IDCT need not be symmetric under a mirror
# or a transposition, so the bound is measured, not assumed -- and it is measured as 0.  The files and seeds are fixed and the oracle is
# deterministic: no margin.  Produced by
#   python -m pytest tests/test_lossless_transform_cpu.py -k pixel_bound -s        (prints "pixel bound: <name> <dri> <max>" per file)
PIXEL_BOUND = 0


def _turnable(f):
    """(orientation, edge, plan) for every orientation the file can be turned by"""
    fr = tm.frame_of(f)
    for o in range(2, 9):
        for edge in ("refuse", "trim"):
            try:
                yield o, edge, tm.plan(fr, o, edge)
                break
            except tm.Refused:
                continue


@pytest.mark.parametrize("name,dri", FILES)
def test_block_equality(name, dri):
    f = tc.make(name, dri)
    fr = tm.frame_of(f)
    coefs, _ = po.decode_coefficients(f)
    seen = 0
    for o, edge, pl in _turnable(f):
        turned, _ = po.decode_coefficients(tm.write_turned(f, o, edge))
        assert turned.shape[0] == pl["mcus"][0] * pl["mcus"][1] * sum(h * v for h, v in pl["factors"])
        assert np.array_equal(turned, tm.turn_blocks(coefs, fr, o, edge)), (name, dri, o, edge)
        seen += 1
    assert seen >= (3 if name == "420_12x32" else 7)


@pytest.mark.parametrize("name,dri", FILES)
def test_pixel_bound(name, dri):
    f = tc.make(name, dri)
    src, _ = po.decode_8bit(f)
    worst = 0
    for o, edge, pl in _turnable(f):
        g = tm.write_turned(f, o, edge)
        assert Image.open(io.BytesIO(g)).size == (pl["width"], pl["height"])
        out, info = po.decode_8bit(g)
        assert (info.width, info.height) == (pl["width"], pl["height"])
        kw, kh = pl["kept"]
        worst = max(worst, int(np.abs(out.astype(int) - tm.turn_pixels(src[:kh, :kw], o).astype(int)).max()))
    print("pixel bound:", name, dri, worst)
    assert worst <= PIXEL_BOUND


@pytest.mark.parametrize("name", ["grey_8x8", "444_16x24", "420_48x32", "422_48x24", "440_24x48", "411_64x16"])
def test_involutions(name):
    f = tc.make(name)
    fr = tm.frame_of(f)
    coefs, _ = po.decode_coefficients(f)
    for o in range(2, 9):
        there = tm.turn_blocks(coefs, fr, o)
        assert not np.array_equal(there, coefs) or name == "grey_8x8"
        back = tm.turn_blocks(there, tm.frame_of(tm.write_turned(f, o)), tm.INVERSE[o])
        assert np.array_equal(back, coefs), (name, o)
    assert np.array_equal(tm.turn_blocks(coefs, fr, 1), coefs)


# ---------------------------------------------------------------------------------------------- planning
@pytest.mark.parametrize("name", list(tc.SHAPES))
def test_plan_transform_agrees_with_the_model(name):
    f = tc.make(name)
    fr = tm.frame_of(f)
    for o in range(1, 9):
        for edge in ("refuse", "trim"):
            try:
                pl = tm.plan(fr, o, edge)
            except tm.Refused as want:
                with pytest.raises(jl.NotSupportedException) as e:
                    jl.plan_transform(f, orientations=[o], edge=edge)
                assert want.axis in str(e.value), (name, o, edge, str(e.value))
                continue
            got = jl.plan_transform(f, orientations=[o], edge=edge)
            assert got == jl.TransformPlan(o, pl["width"], pl["height"], pl["trimmed"], pl["factors"]), (name, o, edge)


def test_factor_swaps_trims_and_refusals():
    assert jl.plan_transform(tc.make("420_48x32"), orientations=[6]).factors == [(2, 2), (1, 1), (1, 1)]
    assert jl.plan_transform(tc.make("422_48x24"), orientations=[5]) == jl.TransformPlan(5, 24, 48, False, [(1, 2), (1, 1), (1, 1)])
    assert jl.plan_transform(tc.make("440_24x48"), orientations=[8]) == jl.TransformPlan(8, 48, 24, False, [(2, 1), (1, 1), (1, 1)])
    assert jl.plan_transform(tc.make("411_64x16"), orientations=[7]) == jl.TransformPlan(7, 16, 64, False, [(1, 4), (1, 1), (1, 1)])
    assert jl.plan_transform(tc.make("grey_20x16"), orientations=[6]) == jl.TransformPlan(6, 16, 20, False, [(1, 1)])
    f = tc.make("420_40x27")
    assert jl.plan_transform(f, orientations=[5]) == jl.TransformPlan(5, 27, 40, False, [(2, 2), (1, 1), (1, 1)])
    assert jl.plan_transform(f, orientations=[2], edge="trim") == jl.TransformPlan(2, 32, 27, True, [(2, 2), (1, 1), (1, 1)])
    assert jl.plan_transform(f, orientations=[6], edge="trim") == jl.TransformPlan(6, 16, 40, True, [(2, 2), (1, 1), (1, 1)])
    for o, axis in ((2, "width"), (4, "height"), (6, "height"), (8, "width")):
        with pytest.raises(jl.NotSupportedException, match=axis):
            jl.plan_transform(f, orientations=[o])
    with pytest.raises(jl.NotSupportedException, match="width"):  # narrower than one MCU: nothing to trim to
        jl.plan_transform(tc.make("420_12x32"), orientations=[2], edge="trim")
    with pytest.raises(jl.NotSupportedException):
        jl.plan_transform(open(tc.__file__.replace("transform_cases.py", "golden/progress.jpg"), "rb").read(), orientations=[2])
    with pytest.raises(jl.InvalidDataException):
        jl.plan_transform(b"\xff\xd8\xff\xd9", orientations=[2])


def test_the_file_policy_reads_the_exif_rule():
    for o in range(1, 9):
        f = tc.make("420_48x32", 0, exif=o)
        assert jl.identify_orientation(f) == o
        assert jl.plan_transform(f, orientation="file").orientation == o
        assert jl.plan_transform(f).orientation == 1 and jl.plan_transform(f, orientation="stored").orientation == 1
        assert jl.plan_transform(f, orientation="file", orientations=[0]).orientation == o
        assert jl.plan_transform(f, orientation="file", orientations=[4]).orientation == 4
    assert jl.plan_transform(tc.make("420_48x32"), orientation="file").orientation == 1  # no tag
    assert jl.plan_transform(tc.make("420_48x32", 0, exif=7, exif_order="big"), orientation="file") == jl.TransformPlan(7, 32, 48, False, [(2, 2), (1, 1), (1, 1)])
    f = tc.make("420_48x32", 0, exif=6)
    at = f.index(b"Exif\0\0") + 6
    for bad in (f[:at] + b"XX" + f[at + 2:], f[:at + 2] + b"\x00\x00" + f[at + 4:], f[:at + 4] + b"\xff\xff\xff\x7f" + f[at + 8:]):
        assert jl.identify_orientation(bad) == 1
        assert jl.plan_transform(bad, orientation="file") == jl.TransformPlan(1, 48, 32, False, [(2, 2), (1, 1), (1, 1)])  # malformed: 1, never a failure


def test_a_file_with_stray_bytes_between_its_segments_is_planned_as_identify_reads_it():
    """The reference's reader looks for a marker, it does not expect one: bytes no segment owns are stepped over.  plan_transform walks the
    headers with that reader, so it agrees with identify_orientation and with the oracle's Identify() on such a file."""
    for name, o in (("420_48x32", 6), ("422_48x24", 3), ("420_40x27", 5)):
        f = tc.make(name, 0, exif=o)
        for before_soi in (False, True):
            s = tc.with_stray_bytes(f, before_soi)
            assert s != f and po.optimize(s, True) == po.optimize(f, True)  # (the oracle's optimizer takes the file)
            info, _ = po.identify(s)
            assert jl.identify_orientation(s) == o
            for kw in ({"orientation": "file"}, {"orientations": [o]}, {}):
                got, clean = jl.plan_transform(s, **kw), jl.plan_transform(f, **kw)
                assert got == clean and got.orientation == (o if kw else 1), (name, before_soi, kw, got)
                swap = got.orientation >= 5
                assert (got.width, got.height) == ((info.height, info.width) if swap else (info.width, info.height))
                assert got.factors == [((c.v, c.h) if swap else (c.h, c.v)) for c in info.comp[:info.ncomp]]
        s = tc.with_stray_bytes(f)
        assert tm.expected(s, o, from_file=True) == tm.expected(f, o, from_file=True)  # (... and the model, whose F' holds no stray byte)


# ---------------------------------------------------------------------------------------------- surface
def test_the_symbols_and_their_signatures():
    names = {name: (res, args) for name, res, args in _capi.SYMBOLS}
    P = C.c_void_p
    assert names["jpgpu_optimizer_set_orientation_policy"] == (C.c_int, [P, C.c_int])
    assert names["jpgpu_optimizer_set_orientations"] == (C.c_int, [P, C.POINTER(C.c_uint8), C.c_int])
    assert names["jpgpu_optimizer_set_edge_policy"] == (C.c_int, [P, C.c_int])
    assert names["jpgpu_optimizer_image_transform"] == (C.c_int, [P, C.c_int, C.POINTER(_capi.TransformInfo)])
    assert names["jpgpu_transform_plan"] == (C.c_int, [P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(_capi.TransformInfo), C.c_char_p, C.c_size_t])
    for name in names:
        if "transform" in name or "optimizer_set_" in name or "turn_ms" in name:
            assert hasattr(_capi.lib, name), name
    assert _capi.lib.jpgpu_sizeof_transform_info() == C.sizeof(_capi.TransformInfo) == 32
    header = open(tc.__file__.replace("tests/transform_cases.py", "include/jpgpu.h")).read()
    for word in ("JPGPU_EDGE_REFUSE = 0", "JPGPU_EDGE_TRIM = 1", "jpgpu_transform_info", "jpgpu_transform_plan", "jpgpu_optimizer_image_transform"):
        assert word in header, word
    info = _capi.TransformInfo()
    f = tc.make("420_40x27")
    buf = np.frombuffer(f, np.uint8)
    msg = C.create_string_buffer(256)
    assert _capi.lib.jpgpu_transform_plan(buf.ctypes.data, buf.size, 9, 0, 0, C.byref(info), msg, 256) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_transform_plan(buf.ctypes.data, buf.size, 2, 2, 0, C.byref(info), msg, 256) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_transform_plan(buf.ctypes.data, buf.size, 2, 0, 2, C.byref(info), msg, 256) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_transform_plan(buf.ctypes.data, buf.size, 2, 0, 0, None, msg, 256) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_transform_plan(buf.ctypes.data, buf.size, 2, 0, 0, C.byref(info), msg, 256) != 0 and b"width" in msg.value
    assert _capi.lib.jpgpu_transform_plan(buf.ctypes.data, buf.size, 2, 0, 1, C.byref(info), None, 0) == 0 and (info.width, info.height, info.trimmed) == (32, 27, 1)


def test_the_python_keyword_arguments_are_checked():
    f = tc.make("420_48x32")
    with pytest.raises(ValueError):
        jl.plan_transform(f, orientations=[2], edge="crop")
    with pytest.raises(ValueError):
        jl.plan_transform(f, orientations=[9])
    with pytest.raises(ValueError):
        jl.plan_transform(f, orientations=[2, 3])
    with pytest.raises(ValueError):
        jl.plan_transform(f, orientation="exif")
    # optimize_batch checks its arguments before it asks for a device
    with pytest.raises(ValueError):
        jl.optimize_batch([f], orientations=[2], edge="crop")
    with pytest.raises(ValueError):
        jl.optimize_batch([f, f], orientations=[2])
    with pytest.raises(ValueError):
        jl.optimize_batch([f], orientation="exif")
    for method in ("set_orientation_policy", "set_orientations", "set_edge_policy", "transform"):
        assert callable(getattr(jl.OptimizeBatch, method))


# ---------------------------------------------------------------------------------------------- the sanitizer harness
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_planning_code_is_clean_under_asan_and_ubsan(tmp_path):
    """tools/fuzz/transform_plan_asan.cpp: a stand-alone program over csrc/transform_plan.h (plan_transform and the in-place patches of F')"""
    exe = str(tmp_path / "plan_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=address,undefined",
                    "-I", os.path.join(ROOT, "jpeglibrary_amd", "csrc"), os.path.join(ROOT, "tools", "fuzz", "transform_plan_asan.cpp"),
                    os.path.join(ROOT, "jpeglibrary_amd", "csrc", "host_parser.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "plan ok: 4000 edits" in r.stdout and " 0 failures" in r.stdout
