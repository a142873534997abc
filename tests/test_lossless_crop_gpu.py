"""The window of the optimizer's lossless transform on the device (include/jpgpu.h section (5), "Window"; kx_lossless.hip, device_optimize.cpp).

Every output is compared byte for byte with tests/crop_model.py: po.optimize() of the file F'' the model writes from the source's own blocks.
There is no tolerance anywhere.  The shapes are those of tests/transform_cases.py plus two that cross a 256-block work entry of KX
(tests/crop_cases.py); every image is a few MCUs.  Where the MCU count of F'' is a multiple of its restart interval the reference's Scan()
gives up (Optimize() then throws): there the model raises and the library must report the same class with an empty output.  CASES lists every
(file, orientation, window) the byte comparisons use, so that the share of them that ends so can be counted: a suite of refusals would cover
nothing."""
import functools

import numpy as np
import pytest

import crop_cases as cc
import crop_model as cm
import jpeglibrary_amd as jl
import transform_cases as tc
import transform_model as tm
from golden_util import read_jpeg
from jpeglibrary_amd import _capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

# ---- (name, dri, orientation, edge, window)
UPRIGHT = [(n, 0, 1, "refuse", w) for n in cc.ALL for w in (cc.interior_window(n), cc.edge_window(n))] + \
          [("420_40x27", 0, 1, "refuse", (16, 16, 24, 11)), ("grey_20x16", 0, 1, "refuse", (8, 8, 12, 8)), ("411_64x16", 0, 1, "refuse", (32, 8, 32, 8))]
MATRIX = {n: [(n, dri, o, "refuse", cc.off_centre_window(n, o)) for dri in (0, 3) for o in range(2, 9)] for n in ("420_48x32", "422_48x24")}
TRIMMED = [("420_40x27", 0, 2, "trim", (16, 16, 16, 11)), ("420_40x27", 0, 7, "trim", (0, 16, 16, 16))]
RESTART = [("420_48x32", 4, 3, "refuse", (16, 0, 32, 32)), ("420_48x32", 3, 3, "refuse", (16, 0, 32, 32))]
ENTRIES = [("420_160x128", 0, 1, "refuse", (16, 16, 128, 96)), ("420_160x128", 0, 6, "refuse", None), ("420_160x128", 0, 6, "refuse", (16, 32, 96, 128)),
           ("444_136x40", 0, 1, "refuse", (8, 8, 128, 32)), ("444_136x40", 0, 5, "refuse", (0, 8, 32, 128))]
CASES = UPRIGHT + MATRIX["420_48x32"] + MATRIX["422_48x24"] + TRIMMED + RESTART + ENTRIES


@functools.lru_cache(maxsize=None)
def _expected(name, dri, o, edge="refuse", window=None, origin="refuse", strip=True, most_optimal=False):
    """the model's bytes, or the oracle's exception; computed once per case"""
    try:
        return cm.expected(cc.make(name, dri), o, edge, window, origin, strip, most_optimal)
    except po.OracleError as e:
        return e


def _run(files, windows=None, orientations=None, strip=True, most_optimal=False, orientation=None, edge="refuse", origin="refuse"):
    """the batch after run(): per image bytes or the exception, transform(i), window(i), and turn_sources()"""
    b = jl.OptimizeBatch().set_most_optimal_coding(most_optimal).set_orientation_policy(orientation).set_edge_policy(edge).set_origin_policy(origin)
    if orientations is not None:
        b.set_orientations(orientations)
    if windows is not None:
        b.set_windows([w or (0, 0, 0, 0) for w in windows])
    b.upload(files, strip).run()
    out = []
    for i in range(len(b)):
        try:
            out.append(b.output(i))
        except jl.JpegError as e:
            assert b.result(i)[1] == 0, "a failing image has an empty output"
            out.append(e)
    plans, applied, sources = [b.transform(i) for i in range(len(b))], [b.window(i) for i in range(len(b))], b.turn_sources()
    b.close()
    return out, plans, applied, sources


def _same(got, want, what):
    if isinstance(want, po.OracleError):
        assert isinstance(got, getattr(jl, want.kind)), (what, want, got)
    else:
        assert isinstance(got, bytes), (what, got)
        assert got == want, (what, len(got), len(want))


def _check_cases(cases, edge="refuse"):
    files = [cc.make(n, dri) for n, dri, _, _, _ in cases]
    outs, plans, applied, sources = _run(files, windows=[c[4] for c in cases], orientations=[c[2] for c in cases], edge=edge)
    for case, f, got, plan, win in zip(cases, files, outs, plans, applied):
        name, dri, o, e, window = case
        assert e == edge
        _same(got, _expected(*case), case)
        pl = cm.plan(tm.frame_of(f), o, e, window)
        assert (plan.orientation, plan.width, plan.height, plan.trimmed, plan.factors) == (o, pl["width"], pl["height"], pl["trimmed"], pl["factors"]), (case, plan)
        assert win == plan.window == pl["window"], (case, win)
    assert sources == len(set(files))
    return outs


def test_a_window_alone_on_every_sampling():
    outs = _check_cases(UPRIGHT)
    assert all(isinstance(o, bytes) for o in outs)
    assert len(UPRIGHT) == 2 * len(cc.ALL) + 3


@pytest.mark.parametrize("name", ["420_48x32", "422_48x24"])
def test_every_orientation_with_a_window_under_two_restart_intervals(name):
    """The window is off-centre (a wrong origin axis, or a mirror counted from the wrong edge, moves it) and one MCU wide, two tall (a swapped
    width and height show).  Two MCUs under DRI 3: no case ends in the restart rule, and no restart marker is written."""
    outs = _check_cases(MATRIX[name])
    assert all(isinstance(o, bytes) for o in outs)
    assert len(set(outs[:7])) == 7 and len(set(outs[7:])) == 7  # (no two orientations collapse)


def test_trim_then_window():
    _check_cases(TRIMMED, edge="trim")
    f = cc.make("420_40x27")
    outs, _, _, _ = _run([f, f], windows=[(0, 0, 16, 16), (32, 0, 8, 16)], orientations=[2, 2], edge="trim")
    assert isinstance(outs[0], bytes) and isinstance(outs[1], jl.ArgumentException) and "outside" in str(outs[1])  # 32 wide behind the trim
    outs, _, _, _ = _run([f], windows=[(0, 0, 16, 16)], orientations=[2])  # the edge refuses first, though the window leaves it out
    assert isinstance(outs[0], jl.NotSupportedException) and "width" in str(outs[0])


def test_the_restart_rule_is_that_of_the_cropped_file():
    """420_48x32 has six MCUs; the window leaves four.  DRI 4: Scan() of F'' gives up.  DRI 3 divides the SOURCE's count, not the window's:
    the image must pass (uncut, the same file reports InvalidOperation)."""
    assert isinstance(_expected(*RESTART[0]), po.OracleError) and _expected(*RESTART[0]).kind == "InvalidOperationException"
    assert isinstance(_expected(*RESTART[1]), bytes)
    outs = _check_cases(RESTART)
    assert isinstance(outs[0], jl.InvalidOperationException) and isinstance(outs[1], bytes)
    plain, _, _, _ = _run([cc.make("420_48x32", 3)], orientations=[3])
    assert isinstance(plain[0], jl.InvalidOperationException)


def test_refusals_are_a_small_share_of_the_cases():
    ended = sum(isinstance(_expected(*c), po.OracleError) for c in CASES)
    assert ended >= 1 and ended <= 0.15 * len(CASES), (ended, len(CASES))


def test_windows_that_cross_a_work_entry_of_the_turn_kernel():
    """288 blocks: two entries, the second with a tail of 32; 480 blocks of a quarter turn without a window; a transposed window of 288; a
    source whose last MCU column is partial"""
    outs = _check_cases(ENTRIES)
    assert all(isinstance(o, bytes) for o in outs)
    blocks = [cm.plan(tm.frame_of(cc.make(n)), o, e, w)["mcus"] for n, _, o, e, w in ENTRIES]
    assert [c * r * (6 if n.startswith("420") else 3) for (c, r), (n, _, _, _, _) in zip(blocks, ENTRIES)] == [288, 480, 288, 192, 192]


def test_pixel_identity_on_the_device():
    """decode(output) == the decoder's own window of the source (orientation 1), == the slice of decode(the uncropped turned output) (2..8)"""
    cases = [(n, 1, w) for n, _, _, _, w in UPRIGHT if n in ("420_48x32", "422_48x24", "420_40x27", "444_136x40", "411_64x16")] + \
            [("420_160x128", 1, (16, 16, 128, 96))] + [(n, o, cc.off_centre_window(n, o)) for n in ("420_48x32", "422_48x24") for o in range(2, 9)] + \
            [("420_160x128", 6, (16, 32, 96, 128))]
    files = [cc.make(n) for n, _, _ in cases]
    outs, _, _, _ = _run(files, windows=[w for _, _, w in cases], orientations=[o for _, o, _ in cases])
    assert all(isinstance(o, bytes) for o in outs), outs
    got, res = jl.decode_batch(outs, jl.FMT_INTERLEAVED_U8)
    assert all(r.status == 0 for r in res)
    upright = [i for i, c in enumerate(cases) if c[1] == 1]
    want, res = jl.decode_batch([files[i] for i in upright], jl.FMT_INTERLEAVED_U8, windows=[cases[i][2] for i in upright])
    assert all(r.status == 0 for r in res)
    for i, w in zip(upright, want):
        assert np.array_equal(got[i], w), cases[i]
    turned = [i for i, c in enumerate(cases) if c[1] != 1]
    whole = jl.optimize_batch([files[i] for i in turned], orientations=[cases[i][1] for i in turned])
    pixels, res = jl.decode_batch(whole, jl.FMT_INTERLEAVED_U8)
    assert all(r.status == 0 for r in res)
    for i, p in zip(turned, pixels):
        x, y, w, h = cases[i][2]
        assert got[i].shape[:2] == (h, w) and np.array_equal(got[i], p[y:y + h, x:x + w]), cases[i]


def test_the_whole_frame_written_out_takes_the_coefficient_road_and_gives_the_untouched_bytes():
    names = [n for n in cc.ALL if n not in ("440_24x48", "411_64x16")]  # the shapes Pillow wrote
    files = [cc.make(n) for n in names]
    windows = [(0, 0) + cc.geometry(n)[:2] for n in names]
    outs, plans, applied, sources = _run(files, windows=windows)
    assert sources == len(files)  # (every one of them was entropy-decoded for the road)
    assert outs == jl.optimize_batch(files) == [po.optimize(f, True) for f in files]
    assert applied == windows
    none, _, applied, sources = _run(files, windows=[(0, 0, 0, 0)] * len(files))  # {0, 0, 0, 0}: no window, the untouched road
    assert sources == 0 and none == outs and applied == windows


def test_the_origin_policy():
    f, g = cc.make("420_48x32"), cc.make("422_48x24")
    windows = [(16, 16, 16, 16), (20, 16, 12, 16), (16, 9, 16, 7), (16, 4, 9, 9), (32, 0, 16, 16)]
    files = [f, f, f, g, f]
    outs, _, _, _ = _run(files, windows=windows)
    assert isinstance(outs[1], jl.NotSupportedException) and "window's x (20)" in str(outs[1]) and "16 pixels" in str(outs[1])
    assert isinstance(outs[2], jl.NotSupportedException) and "window's y (9)" in str(outs[2]) and "16 pixels" in str(outs[2])
    assert isinstance(outs[3], jl.NotSupportedException) and "window's y (4)" in str(outs[3]) and "8 pixels" in str(outs[3])
    assert outs[0] == _expected("420_48x32", 0, 1, "refuse", windows[0]) and outs[4] == _expected("420_48x32", 0, 1, "refuse", windows[4])  # the neighbours
    outs, plans, applied, _ = _run(files, windows=windows, origin="expand")
    for i, (name, w) in enumerate(zip(("420_48x32",) * 3 + ("422_48x24", "420_48x32"), windows)):
        pl = cm.plan(tm.frame_of(files[i]), 1, "refuse", w, "expand")
        assert applied[i] == pl["window"] and (plans[i].width, plans[i].height) == pl["window"][2:]
        assert outs[i] == _expected(name, 0, 1, "refuse", w, "expand"), i
    assert applied[1] == (16, 16, 16, 16) and applied[2] == (16, 0, 16, 16) and applied[3] == (16, 0, 9, 13) and outs[1] == outs[0]
    # under a transposing orientation the MCU of F' is the source's, turned: 4:2:2 becomes 8 x 16
    outs, _, applied, _ = _run([g, g], windows=[(8, 16, 8, 16), (12, 20, 4, 12)], orientations=[6, 6], origin="expand")
    assert applied == [(8, 16, 8, 16)] * 2 and outs[0] == outs[1] == _expected("422_48x24", 0, 6, "refuse", (8, 16, 8, 16))


def test_a_mixed_batch_keeps_every_image_to_itself():
    f, g = cc.make("420_48x32"), cc.make("422_48x24", 2)
    progressive = read_jpeg("progress.jpg")
    unwalkable = f[:f.index(b"\xff\xc0")]  # no frame header, no scan
    batch = [f, f, g, f, progressive, f, unwalkable, unwalkable, g]
    windows = [None, (32, 16, 16, 16), (0, 32, 8, 16), (40, 0, 16, 16), (0, 0, 8, 8), (16, 0, 16, 0), (0, 0, 8, 8), None, None]
    orients = [1, 1, 8, 1, 1, 4, 1, 1, 5]
    outs, plans, applied, sources = _run(batch, windows=windows, orientations=orients)
    assert sources == 2  # f (cropped) and g (turned and cropped, turned): the refused ones are not decoded, and one file is decoded once
    assert outs[0] == po.optimize(f, True) and applied[0] == (0, 0, 48, 32) and plans[0].orientation == 1
    assert outs[1] == _expected("420_48x32", 0, 1, "refuse", windows[1]) and applied[1] == windows[1] and plans[1][:4] == (1, 16, 16, False)
    assert outs[2] == _expected("422_48x24", 2, 8, "refuse", windows[2]) and applied[2] == windows[2]
    assert plans[2] == jl.TransformPlan(8, 8, 16, False, [(1, 2), (1, 1), (1, 1)], windows[2])
    assert isinstance(outs[3], jl.ArgumentException) and "outside" in str(outs[3]) and "48 x 32" in str(outs[3])
    assert isinstance(outs[5], jl.ArgumentException) and "zero" in str(outs[5])
    plain = jl.OptimizeBatch().upload([progressive, unwalkable], True).run()
    for i, k in ((4, 0), (6, 1), (7, 1)):  # files the optimizer's own walks fail keep that status, with a window or without: never a picture
        with pytest.raises(jl.JpegError) as alone:
            plain.output(k)
        assert type(outs[i]) is type(alone.value) and str(outs[i]) == str(alone.value), (i, outs[i], alone.value)
    plain.close()
    assert outs[8] == tm.expected(g, 5)
    for i in (1, 2, 8):
        w, o = windows[i], orients[i]
        alone, _, _, _ = _run([batch[i]], windows=[w], orientations=[o])
        assert alone[0] == outs[i], i


def test_the_list_is_consumed_and_a_wrong_count_leaves_the_optimizer_usable():
    f, g = cc.make("420_48x32"), cc.make("422_48x24")
    b = jl.OptimizeBatch()
    b.set_windows([(16, 16, 16, 16), (0, 0, 0, 0)]).upload([f, g], True).run()
    first = [b.output(i) for i in range(2)]
    assert first == [_expected("420_48x32", 0, 1, "refuse", (16, 16, 16, 16)), po.optimize(g, True)] and b.turn_sources() == 1
    b.run()
    assert [b.output(i) for i in range(2)] == first  # a second run
    b.upload([f, g], True).run()  # the list was consumed: untouched bytes
    assert [b.output(i) for i in range(2)] == [po.optimize(f, True), po.optimize(g, True)] and b.turn_sources() == 0 and b.window(0) == (0, 0, 48, 32)
    b.set_windows([(16, 16, 16, 16), (0, 0, 0, 0)]).upload([f, g], True).run()  # a second upload
    assert [b.output(i) for i in range(2)] == first
    with pytest.raises(jl.ArgumentException):
        b.set_windows([(0, 0, 16, 16)]).upload([f, g], True)
    with pytest.raises(jl.JpegError):  # empty: nothing to report
        b.result(0)
    b.upload([f], True).run()  # ... and usable; the refused list does not come back
    assert b.output(0) == po.optimize(f, True) and b.window(0) == (0, 0, 48, 32)
    b.set_windows([(16, 16, 16, 16)]).set_windows(None).upload([f], True).run()  # withdrawn
    assert b.output(0) == po.optimize(f, True)
    assert _capi.lib.jpgpu_optimizer_set_origin_policy(b._h, 2) == _capi.ERR_ARGUMENT
    b.close()


def test_tiles_of_one_canvas_are_decoded_once():
    canvas, other = cc.make("420_160x128"), cc.make("444_136x40")
    tiles = [(32 * c, 32 * r, 32, 32) for r in range(4) for c in range(5)]
    outs, _, applied, sources = _run([canvas] * 20, windows=tiles)
    assert sources == 1 and applied == tiles
    want = [_expected("420_160x128", 0, 1, "refuse", t) for t in tiles]
    assert outs == want and len(set(outs)) == 20
    assert [_run([canvas], windows=[t])[0][0] for t in tiles] == outs  # the sharing does not show
    strips = [(8 * k, 8, 8, 24) for k in range(10)]
    mixed, _, _, sources = _run([canvas, other] * 10, windows=[w for pair in zip(tiles[:10], strips) for w in pair])
    assert sources == 2
    assert mixed[0::2] == want[:10] and mixed[1::2] == [_expected("444_136x40", 0, 1, "refuse", s) for s in strips]
    copies, _, _, sources = _run([canvas, bytes(bytearray(canvas))], windows=tiles[:2])  # equal bytes, another object: another file
    assert sources == 2 and copies == want[:2]


def test_most_optimal_coding_strip_and_the_keyword_arguments():
    f = cc.make("420_48x32", 4)
    w = (16, 16, 16, 32)
    (got,), _, _, _ = _run([f], windows=[w], orientations=[7], most_optimal=True)
    assert got == _expected("420_48x32", 4, 7, "refuse", w, most_optimal=True)
    assert jl.optimize_batch([f, f], windows=[w, (0, 0, 0, 0)], orientations=[7, 1]) == [_expected("420_48x32", 4, 7, "refuse", w), po.optimize(f, True)]
    assert jl.optimize_batch([f], windows=[(20, 20, 8, 8)], origin="expand") == [_expected("420_48x32", 4, 1, "refuse", (20, 20, 8, 8), "expand")]
    with pytest.raises(jl.NotSupportedException, match="window's x"):
        jl.optimize_batch([f], windows=[(20, 20, 8, 8)])


def test_strip_false_keeps_the_appn_segments_and_rewrites_the_exif_tag_only_where_the_file_decided():
    f = cc.make("420_48x32", 0, exif=6)
    w = (16, 16, 16, 32)  # in the 32 x 48 frame the tag turns the file into
    (kept,), plans, _, _ = _run([f], windows=[w], strip=False, orientation="file")
    assert plans[0] == jl.TransformPlan(6, 16, 32, False, [(2, 2), (1, 1), (1, 1)], w)
    assert kept == cm.expected(f, 6, "refuse", w, strip=False, from_file=True)
    assert jl.identify_orientation(f) == 6 and jl.identify_orientation(kept) == 1
    (before,), (after,) = tc.app1_of(f), tc.app1_of(kept)
    assert len(before) == len(after) and before != after
    (listed,), _, _, _ = _run([f], windows=[w], orientations=[8], strip=False, orientation="file")  # an explicit value leaves APP1 alone
    assert listed == cm.expected(f, 8, "refuse", w, strip=False) and tc.app1_of(listed) == tc.app1_of(f)
    (upright,), _, _, _ = _run([f], windows=[(16, 16, 32, 16)], orientations=[1], strip=False, orientation="file")  # a window alone: nothing decided
    assert upright == cm.expected(f, 1, "refuse", (16, 16, 32, 16), strip=False) and tc.app1_of(upright) == tc.app1_of(f)
    (stripped,), _, _, _ = _run([f], windows=[w], orientation="file")
    assert stripped == cm.expected(f, 6, "refuse", w, from_file=True) and b"Exif" not in stripped
