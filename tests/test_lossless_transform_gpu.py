"""The optimizer's lossless transform on the device (include/jpgpu.h section (5), "Lossless transform"; kx_lossless.hip, device_optimize.cpp).

Every output is compared byte for byte with tests/transform_model.py: po.optimize() of the file F' the model writes from the source's own
blocks.  The shapes (tests/transform_cases.py) are the smallest at which KX's index arithmetic can still go wrong; the restart intervals are
0, 1, 2 (which does not divide the three MCUs of a row), 4 and one above the MCU count.  The reference's Scan() gives up on a scan whose MCU
count is a multiple of its restart interval (Optimize() then throws): there the model raises and the library must report the same class with an
empty output -- which is what the image reports without being turned, too."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeglibrary_amd as jl
import transform_cases as tc
import transform_model as tm
from golden_util import read_jpeg
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

DRIS = (0, 1, 2, 4, 100)
ALIGNED = ("grey_8x8", "444_16x24", "420_48x32", "422_48x24", "440_24x48", "411_64x16")


def _run(files, strip=True, most_optimal=False, orientation=None, orientations=None, edge="refuse"):
    """the batch after run(): per image bytes or the exception, and transform(i)"""
    b = jl.OptimizeBatch().set_most_optimal_coding(most_optimal).set_orientation_policy(orientation).set_edge_policy(edge)
    if orientations is not None:
        b.set_orientations(orientations)
    b.upload(files, strip).run()
    out = []
    for i in range(len(b)):
        try:
            out.append(b.output(i))
        except jl.JpegError as e:
            assert b.result(i)[1] == 0, "a failing image has an empty output"
            out.append(e)
    plans = [b.transform(i) for i in range(len(b))]
    b.close()
    return out, plans


def _expected(f, o, **kw):
    try:
        return tm.expected(f, o, **kw)
    except po.OracleError as e:
        return e


def _same(got, want, what):
    if isinstance(want, po.OracleError):
        assert isinstance(got, getattr(jl, want.kind)), (what, want, got)
    else:
        assert isinstance(got, bytes), (what, got)
        assert got == want, (what, len(got), len(want))


def _check_plan(plan, f, o, edge="refuse"):
    pl = tm.plan(tm.frame_of(f), o, edge)
    assert (plan.orientation, plan.width, plan.height, plan.trimmed, plan.factors) == (o, pl["width"], pl["height"], pl["trimmed"], pl["factors"]), (plan, pl)


@pytest.mark.parametrize("name", ["420_48x32", "422_48x24"])
def test_every_orientation_under_every_restart_interval(name):
    files, orients = [], []
    for dri in DRIS:
        for o in range(2, 9):
            files.append(tc.make(name, dri))
            orients.append(o)
    outs, plans = _run(files, orientations=orients)
    produced = {dri: 0 for dri in DRIS}
    for f, o, got, plan in zip(files, orients, outs, plans):
        dri = tm.frame_of(f)["dri"]
        _same(got, _expected(f, o), (name, dri, o))
        _check_plan(plan, f, o)
        produced[dri] += isinstance(got, bytes)
    # an interval that divides the MCU count (six, or nine) makes the reference's Scan() give up; every other one gives all seven files
    mcus = {"420_48x32": 6, "422_48x24": 9}[name]
    assert produced == {dri: (0 if dri and mcus % dri == 0 else 7) for dri in DRIS}, produced


def test_the_other_shapes_under_the_orientations_their_geometry_makes_interesting():
    cases = [("grey_8x8", o, "refuse") for o in range(2, 9)] + [("grey_20x16", o, "refuse") for o in (4, 5, 6)] + [("grey_20x16", o, "trim") for o in (2, 3, 8)] + \
            [("444_16x24", o, "refuse") for o in (3, 6, 7)] + [("440_24x48", o, "refuse") for o in (2, 5, 8)] + [("411_64x16", o, "refuse") for o in (6, 8, 3)] + \
            [("420_40x27", 5, "refuse"), ("420_40x27", 2, "trim"), ("420_40x27", 4, "trim"), ("420_40x27", 7, "trim"), ("420_12x32", 4, "refuse"), ("420_12x32", 6, "refuse")]
    for edge in ("refuse", "trim"):
        sel = [c for c in cases if c[2] == edge]
        files = [tc.make(n) for n, _, _ in sel]
        outs, plans = _run(files, orientations=[o for _, o, _ in sel], edge=edge)
        for (n, o, _), f, got, plan in zip(sel, files, outs, plans):
            _same(got, _expected(f, o, edge=edge), (n, o, edge))
            _check_plan(plan, f, o, edge)
            assert isinstance(got, bytes), (n, o, got)
            assert Image.open(io.BytesIO(got)).size == (plan.width, plan.height)
    f = tc.make("420_40x27")
    assert _run([f], orientations=[2], edge="trim")[1][0][1:4] == (32, 27, True)


def test_edges_that_are_refused_name_their_axis_and_leave_the_neighbours_alone():
    f, narrow, ok = tc.make("420_40x27"), tc.make("420_12x32"), tc.make("420_48x32")
    outs, _ = _run([f, ok, f, narrow, f], orientations=[4, 6, 2, 2, 3])
    assert outs[1] == tm.expected(ok, 6)
    for got, axis in ((outs[0], "height"), (outs[2], "width"), (outs[3], "width")):
        assert isinstance(got, jl.NotSupportedException) and axis in str(got), got
    assert isinstance(outs[4], jl.NotSupportedException)
    outs, _ = _run([narrow, ok], orientations=[2, 2], edge="trim")  # narrower than one MCU: nothing would be left
    assert isinstance(outs[0], jl.NotSupportedException) and "width" in str(outs[0]) and outs[1] == tm.expected(ok, 2)


@pytest.mark.parametrize("name", ALIGNED)
def test_an_orientation_and_its_inverse_give_back_the_optimized_source(name):
    f = tc.make(name)
    want = jl.optimize_batch([f])[0]
    assert want == po.optimize(f, True)
    once, _ = _run([f] * 7, orientations=list(range(2, 9)))
    back, _ = _run(once, orientations=[tm.INVERSE[o] for o in range(2, 9)])
    for o, got in zip(range(2, 9), back):
        assert got == want, (name, o)


def test_the_decoded_blocks_of_the_output_are_the_turned_blocks_of_the_source():
    names = ["420_48x32", "422_48x24", "411_64x16", "grey_20x16"]
    # (restart intervals that never restart: the scan Optimize() writes behind a real RSTn is one the reference's own decoder rejects, turned
    # or not -- po.decode_coefficients(po.optimize(f)) fails on these sources as they are -- so there is nothing to decode back)
    files = [tc.make(n, dri) for n, dri in zip(names, (100, 0, 100, 0))]
    orients = [6, 7, 8, 5]
    outs, _ = _run(files, orientations=orients)
    src = jl.Batch().upload(files, jl.FMT_PLANAR_U8)
    src.run_entropy()
    dst = jl.Batch().upload(outs, jl.FMT_PLANAR_U8)
    dst.run_entropy()
    for i, (f, o) in enumerate(zip(files, orients)):
        assert np.array_equal(dst.coefficients(i), tm.turn_blocks(src.coefficients(i), tm.frame_of(f), o)), (names[i], o)


def test_a_mixed_batch_keeps_every_image_to_itself():
    shapes = ["420_48x32", "grey_8x8", "444_16x24", "422_48x24", "440_24x48", "grey_20x16", "420_48x32", "411_64x16"]
    files = [tc.make(n, dri) for n, dri in zip(shapes, (0, 0, 4, 2, 0, 0, 4, 100))]  # orientations 1..8, in order
    orients = list(range(1, 9))
    tagged = [tc.make("420_48x32", 0, exif=6), tc.make("422_48x24", 0, exif=3, exif_order="big"), tc.make("444_16x24", 0, exif=1)]
    truncated = tc.make("420_48x32", 4)[:-40]
    progressive = read_jpeg("progress.jpg")
    batch = files + tagged + [truncated, progressive]
    given = orients + [0, 0, 0, 5, 6]
    outs, plans = _run(batch, orientation="file", orientations=given)
    plain = jl.OptimizeBatch().upload(batch, True).run()
    for i, (f, o) in enumerate(zip(batch, given)):
        applied = plans[i].orientation
        if i < 8:
            assert applied == o
        if 8 <= i < 11:
            assert applied == (6, 3, 1)[i - 8]
        if i >= 11:  # the failing two keep the optimizer's statuses
            with pytest.raises(jl.JpegError) as plain_err:
                plain.output(i)
            assert type(outs[i]) is type(plain_err.value), (i, outs[i], plain_err.value)
            continue
        if applied == 1:
            assert outs[i] == plain.output(i) == po.optimize(f, True)
        else:
            _same(outs[i], _expected(f, applied, from_file=8 <= i < 11), (i, applied))
            alone, _ = _run([f], orientations=[applied])
            assert alone[0] == outs[i], i
    plain.close()


def test_files_with_stray_bytes_between_their_segments():
    """Bytes no segment owns (the reference's reader steps over them): with nothing set the file is optimized as ever; turned, it gives what its
    clean twin gives.  (Bytes in front of SOI: the optimizer's upload goes through the decoder-side parser, which asks for SOI at offset 0 and
    fails such a file whatever is set -- the transform's plan is not what decides it: the outcome is the same with and without a list.)"""
    f = tc.make("420_48x32", 0, exif=6)
    stray, junk = tc.with_stray_bytes(f), tc.with_stray_bytes(f, before_soi=True)
    for strip in (True, False):
        assert jl.optimize_batch([stray, f], strip=strip) == [po.optimize(stray, strip), po.optimize(f, strip)]
        # a list of ones, and a policy that finds nothing to do, leave the road alone as well
        assert jl.optimize_batch([stray], strip=strip, orientations=[1], orientation="stored") == [po.optimize(stray, strip)]
        (untouched, neighbour), _ = _run([junk, stray], strip=strip)
        (listed, turned), _ = _run([junk, stray], strip=strip, orientation="file", orientations=[1, 0])
        assert type(untouched) is type(listed) and str(untouched) == str(listed) and neighbour == po.optimize(stray, strip)
        assert turned == tm.expected(stray, 6, strip=strip, from_file=True)
        (by_file, by_list), plans = _run([stray, stray], strip=strip, orientation="file", orientations=[0, 8])
        assert [p.orientation for p in plans] == [6, 8]
        assert by_file == tm.expected(stray, 6, strip=strip, from_file=True) == tm.expected(f, 6, strip=strip, from_file=True)
        assert by_list == tm.expected(stray, 8, strip=strip)
    assert jl.identify_orientation(by_file) == 1


def test_the_exif_tag_is_rewritten_only_where_the_file_decided():
    for order in ("little", "big"):
        f = tc.make("420_48x32", 0, exif=6, exif_order=order)
        assert jl.identify_orientation(f) == 6
        (kept,), _ = _run([f], strip=False, orientation="file")
        assert kept == tm.expected(f, 6, strip=False, from_file=True)
        assert jl.identify_orientation(kept) == 1
        (before,), (after,) = tc.app1_of(f), tc.app1_of(kept)
        at = tm.exif_value_at(f)[0] - (f.index(b"Exif\0\0"))
        assert len(before) == len(after) and before[:at] == after[:at] and before[at + 2:] == after[at + 2:] and before[at:at + 2] != after[at:at + 2]
        (listed,), _ = _run([f], strip=False, orientation="file", orientations=[8])  # an explicit value leaves APP1 alone
        assert listed == tm.expected(f, 8, strip=False) and tc.app1_of(listed) == tc.app1_of(f) and jl.identify_orientation(listed) == 6
        (stripped,), _ = _run([f], strip=True, orientation="file")
        assert stripped == tm.expected(f, 6, from_file=True)
        # what Optimize(true) keeps of the APPn segments: APP0 alone (JpegOptimizer.cs copies it whatever `strip` says)
        assert not any(m in range(0xE1, 0xF0) for m, _, _, _ in tm.segments(stripped)[0]) and b"Exif" not in stripped


def test_a_second_run_and_a_second_upload_give_the_same_bytes():
    a, b2 = tc.make("420_48x32", 4), tc.make("422_48x24", 0)
    b = jl.OptimizeBatch()
    b.set_orientations([6, 1, 3]).upload([a, b2, a], True).run()
    first = [b.output(i) for i in range(3)]
    b.run()
    assert [b.output(i) for i in range(3)] == first
    assert first[0] == tm.expected(a, 6) and first[1] == po.optimize(b2, True) and first[2] == tm.expected(a, 3)
    b.upload([b2, a], True).run()  # the list was consumed: nothing is turned
    assert [b.transform(i).orientation for i in range(2)] == [1, 1] and b.output(0) == first[1] and b.output(1) == po.optimize(a, True)
    b.set_orientations([8, 2]).upload([b2, a], True).run()
    assert b.output(0) == tm.expected(b2, 8) and b.output(1) == tm.expected(a, 2)
    assert b.turn_ms() > 0
    with pytest.raises(jl.ArgumentException):  # a list of another length: refused, and consumed
        b.set_orientations([2]).upload([a, a], True)
    b.upload([a], True).run()
    assert b.transform(0).orientation == 1 and b.output(0) == po.optimize(a, True)
    b.close()


def test_most_optimal_coding_is_honoured():
    f = tc.make("420_48x32", 4)
    (got,), _ = _run([f], most_optimal=True, orientations=[7])
    assert got == tm.expected(f, 7, most_optimal=True)


def test_the_keyword_arguments_of_optimize_batch():
    f, tagged = tc.make("422_48x24"), tc.make("420_40x27", 0, exif=5)
    assert jl.optimize_batch([f, f], orientations=[6, 1]) == [tm.expected(f, 6), po.optimize(f, True)]
    assert jl.optimize_batch([tagged], strip=True, orientation="file") == [tm.expected(tagged, 5, from_file=True)]
    assert jl.optimize_batch([tc.make("420_40x27")], orientations=[2], edge="trim") == [tm.expected(tc.make("420_40x27"), 2, edge="trim")]
    assert jl.optimize_batch([f]) == [po.optimize(f, True)]
