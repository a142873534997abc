"""The decode policies in combination on the GPU: every row of tests/policy_model.py's covering array against the composed model, bit for bit.

The array's rows that share their upload settings are one upload, so most uploads hold images on several of the planner's roads at once.  Each
upload is driven through Batch's setters, decoded into an output buffer filled with 0xA5, and every image's status, its seven accessors and
its bytes are the model's; the bytes between the slots stay 0xA5; a resize sink's slabs are the model's; a second decode gives the same bytes.
Behind the matrix: every road the planner has under one set of settings in ONE upload, forwards and reversed; the two stage calls against
decode(); and the Exif route to the orientations against the given list.  No tolerance anywhere: floats are compared as bit patterns."""
import numpy as np
import pytest
import torch

import float_sink_model as fm
import jpeglibrary_amd as jl
import orient_model as om
import policy_model as pm
from test_color_gpu import _assert_bits

pytestmark = pytest.mark.gpu

_TORCH = {np.uint8: torch.uint8, np.float16: torch.float16, np.float32: torch.float32}
_outcome = pm.row_outcome  # the model of row k, computed once (shared with test_batch_reuse_gpu.py) and never changed


def _upload(settings, images, files=None, orientation_policy=None, batch=None):
    """settings: a Row whose upload axes count; images: [(file name, orientation, window rectangle or None)] -> the Batch, uploaded, not decoded.
    files: the bytes to upload in place of the named files'; orientation_policy: set it and give no list; batch: a Batch that has been used
    (test_batch_reuse_gpu.py) in place of a fresh one -- what this upload does not set is first put back to what a fresh Batch has"""
    fmt, consts, resize = pm.sink(settings.sink)
    b = jl.Batch() if batch is None else batch
    if batch is not None:
        b.set_resize(None).set_scale_fit(None).set_output_affine(*fm.DEFAULT).set_orientation_policy("stored").set_orientations(None).set_windows(None)
    b.set_arithmetic_policy(settings.arithmetic).set_upsampling_policy(settings.upsampling).set_color_policy(settings.color)
    b.set_channels_policy(settings.mode)
    if settings.scale == "fit":
        b.set_scale_fit(pm.FIT)
    else:
        b.set_scale_policy(settings.scale)
    if consts is not None:
        b.set_output_affine(*consts)
    if resize is not None:
        b.set_resize(resize[:2], _TORCH[resize[2]])
    if orientation_policy is not None:
        b.set_orientation_policy(orientation_policy)
    else:
        b.set_orientations([o for _, o, _ in images])
    if any(w is not None for _, _, w in images):
        b.set_windows([w or (0, 0, 0, 0) for _, _, w in images])
    return b.upload(files if files is not None else [pm.file(n) for n, _, _ in images], fmt)


def _row_images(ks):
    out = []
    for k in ks:
        r = pm.rows()[k]
        plan = pm.frame_plan(pm.file(r.file), r.arithmetic, r.scale, r.color, r.orientation)
        out.append((r.file, r.orientation, pm.window_rect(r.window, plan.width, plan.height)))
    return out


def _poisoned_decode(b):
    """fills the output buffer with 0xA5, decodes -> the buffer's bytes afterwards"""
    base, total = b.output_device_ptr()
    if not total:
        b.decode().sync()
        return np.zeros(0, np.uint8)
    canvas = torch.as_tensor(jl.batch._DeviceView(None, base, (total,)), device="cuda:0")
    canvas.fill_(0xA5)
    torch.cuda.synchronize()
    b.decode().sync()
    return canvas.cpu().numpy()


def _check_image(b, i, want, what):
    info = b.image_info(i)
    assert info.status == want.status, (what, info.status, want.status)
    got = (b.scale(i), b.arithmetic(i), b.upsampling(i), b.channels(i), b.color(i), b.orientation(i))
    assert got == (want.scale, want.arithmetic, want.upsampling, want.channels, want.color, want.orientation), (what, got, want[3:9])
    if want.refused:
        assert info.out_bytes == 0, what
        return
    assert b.result(i).status == 0 and b.window(i) == want.window, (what, b.result(i).status, b.window(i), want.window)
    _assert_bits(b.output(i), want.output, what)


def _check_uploaded(b, settings, ks):
    """b: the rows ks uploaded under settings, not decoded -> decoded over 0xA5 and checked against the model; b is left open"""
    wants = [_outcome(k) for k in ks]
    what = ["row %d %r" % (k, tuple(pm.rows()[k])) for k in ks]
    after = _poisoned_decode(b)
    end = 0
    for i, want in enumerate(wants):
        _check_image(b, i, want, what[i])
        if not want.refused:
            info = b.image_info(i)
            assert info.out_offset >= end and (after[end:info.out_offset] == 0xA5).all(), "the bytes in front of " + what[i]
            end = info.out_offset + info.out_bytes
    assert (after[end:] == 0xA5).all(), "the bytes behind the last slot"
    resized = b.resized() if pm.sink(settings.sink)[2] is not None else None
    if resized is not None:
        for i, want in enumerate(wants):
            if want.refused:
                assert not resized[i].view(np.uint8).any(), what[i]
            else:
                _assert_bits(resized[i], want.resized, "resized " + what[i])
    # a second decode of the same upload: scratch and staging leave no state behind
    first = [None if w.refused else b.output(i).tobytes() for i, w in enumerate(wants)]
    b.decode().sync()
    for i, w in enumerate(wants):
        assert w.refused or b.output(i).tobytes() == first[i], "the second decode of " + what[i]
    if resized is not None:
        assert b.resized().tobytes() == resized.tobytes(), "the second decode's resized buffer"


def _check_upload(settings, ks):
    b = _upload(settings, _row_images(ks))
    _check_uploaded(b, settings, ks)
    b.close()


@pytest.mark.parametrize("scale", pm.SCALES, ids=lambda s: "scale_%s" % s)
@pytest.mark.parametrize("arithmetic", pm.ARITHMETICS)
def test_every_row_of_the_covering_array_equals_the_composed_model(arithmetic, scale):
    mine = [(u, ks) for u, ks in pm.uploads() if (u.arithmetic, u.scale) == (arithmetic, scale)]
    assert mine
    for settings, ks in mine:
        _check_upload(settings, ks)


# ------------------------------------------------------------------------------------------------ every road in one upload

# (file, orientation, window name): under color="file", "fancy", "libjpeg", scale 2 the images of
#   K3R then ycc_to_rgb (upright, no ratio left or none to begin with), K3C (the by-file kinds, upright), K3U direct (a ratio left, upright),
#   K3U staged + K3O (a ratio left, turned), K3O alone (turned, nothing to filter), the float fallback at full size (the odd layout);
#   under mode="gray" all of them but the fallback take K3Y's scratch road
ROADS = [("444", 1, "none"), ("420", 1, "seam"), ("cmyk", 1, "none"), ("adobe_rgb", 1, "interior"), ("422", 1, "none"), ("440", 1, "interior"),
         ("422", 6, "none"), ("440", 7, "seam"), ("420_dri4", 4, "interior"), ("444", 3, "none"), ("cmyk", 5, "last"), ("420", 8, "none"), ("odd", 1, "none"),
         ("odd", 6, "interior"), ("gray", 2, "none"), ("422_three_scans", 1, "none"), ("420_progressive", 5, "seam")]


@pytest.mark.parametrize("mode", pm.MODES)
def test_every_road_in_one_upload_forwards_and_reversed(mode):
    settings = pm.Row(None, None, None, "libjpeg", 2, "fancy", "file", mode, "planar_u8")
    images, wants = [], []
    for name, o, wname in ROADS:
        plan = pm.frame_plan(pm.file(name), "libjpeg", 2, "file", o)
        images.append((name, o, pm.window_rect(wname, plan.width, plan.height)))
        wants.append(pm.expected(pm.file(name), arithmetic="libjpeg", scale=2, upsampling="fancy", color="file", mode=mode, orientation=o, window=images[-1][2],
                                 fmt=jl.FMT_RGB_PLANAR_U8, consts=None, resize=None))
    # the model's view of the roads: every kind of image is there
    assert {(w.arithmetic, w.scale) for w in wants} == {(1, 2), (0, 1)}
    assert {(w.upsampling, w.orientation != 1) for w in wants} == ({(0, False), (0, True)} if mode == "gray" else {(0, False), (0, True), (1, False), (1, True)})
    assert {"gray", "ycbcr", "rgb", "cmyk"} == {w.color for w in wants} and {w.channels for w in wants} == {1 if mode == "gray" else 3}
    solo = []
    for img in images:
        s = _upload(settings, [img]).decode().sync()
        solo.append(s.output(0))
        s.close()
    for order in (list(range(len(images))), list(range(len(images)))[::-1]):
        b = _upload(settings, [images[k] for k in order])
        after = _poisoned_decode(b)
        infos = [b.image_info(i) for i in range(len(order))]
        end = 0
        for i, k in enumerate(order):
            what = "%r at %d of %d" % (ROADS[k], i, len(order))
            _check_image(b, i, wants[k], what)
            _assert_bits(b.output(i), solo[k], "the solo decode of " + what)
            assert (after[end:infos[i].out_offset] == 0xA5).all(), "the bytes in front of " + what
            end = infos[i].out_offset + infos[i].out_bytes
            if i + 1 < len(order):
                assert infos[i + 1].out_offset - infos[i].out_offset >= wants[k].slot_bytes, (what, infos[i + 1].out_offset - infos[i].out_offset, wants[k].slot_bytes)
        assert (after[end:] == 0xA5).all()
        if mode == "gray":
            assert b.luma_work() == (0, len(order))
        b.close()


# ------------------------------------------------------------------------------------------------ the stage calls, the Exif route

def _three_uploads_that_differ_in_road():
    """the largest upload of the matrix under "reference", under "libjpeg" at full size and under "libjpeg" at a reduced size"""
    picks = []
    for arithmetic, scales in (("reference", pm.SCALES), ("libjpeg", (1,)), ("libjpeg", (2, 4))):
        picks.append(max((x for x in pm.uploads() if x[0].arithmetic == arithmetic and x[0].scale in scales), key=lambda x: len(x[1])))
    return picks


def test_run_entropy_and_run_idct_give_the_bytes_of_decode():
    for settings, ks in _three_uploads_that_differ_in_road():
        b = _upload(settings, _row_images(ks)).run_entropy().run_idct().sync()
        for i, k in enumerate(ks):
            _check_image(b, i, _outcome(k), "row %d through the stage calls" % k)
        if pm.sink(settings.sink)[2] is not None:
            for i, k in enumerate(ks):
                if not _outcome(k).refused:
                    _assert_bits(b.resized()[i], _outcome(k).resized, "resized row %d through the stage calls" % k)
        b.close()


def test_exif_tagged_copies_give_the_bytes_of_the_given_list():
    settings, ks = max((x for x in pm.uploads() if x[0].arithmetic == "libjpeg" and x[0].color == "file"), key=lambda x: (len({pm.rows()[k].orientation for k in x[1]}), len(x[1])))
    images = _row_images(ks)
    assert len({o for _, o, _ in images}) >= 3
    tagged = [om.with_orientation(pm.file(n), o, "MM" if i & 1 else "II") for i, (n, o, _) in enumerate(images)]
    assert [jl.identify_orientation(f) for f in tagged] == [o for _, o, _ in images]
    b = _upload(settings, images, files=tagged, orientation_policy="file").decode().sync()
    for i, k in enumerate(ks):
        _check_image(b, i, _outcome(k), "row %d through its Exif block" % k)
    b.close()
