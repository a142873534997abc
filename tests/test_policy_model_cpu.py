"""tests/policy_model.py on the CPU: the covering array covers what it must and is the same on every build, few of its rows are refusals, the
composed model is each single-feature model where only that feature is switched on, and it is Pillow's draft() + transpose + crop + convert
wherever Pillow can do the whole chain."""
import io

import numpy as np
import pytest

import jpeglibrary_amd as jl
import color_model as cm
import float_sink_model as fm
import islow_model as im
import luma_model as lm
import orient_model as om
import policy_model as pm
import resize_model as rm
import scaled_model as sm
import upsample_model as um

DEFAULTS = dict(arithmetic="reference", scale=1, upsampling="replicate", color="ycc", mode="rgb", orientation=1, window=None, fmt=jl.FMT_RGB_PLANAR_U8,
                consts=None, resize=None)


def _expected(name, **kw):
    return pm.expected(pm.file(name), **dict(DEFAULTS, **kw))


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


def _oracle(name):
    from oracle import pyoracle

    return pyoracle.decode_8bit(pm.file(name))[0]


# ------------------------------------------------------------------------------------------------ 1: the array

def test_every_required_pair_and_triple_has_a_row():
    required = pm.required_tuples()
    assert len(required) == len(set(required))
    n_pairs = sum(len(a) * len(b) for k, a in enumerate(pm.VALUES) for b in pm.VALUES[k + 1:])
    assert sum(t[0] == "p" for t in required) == n_pairs and sum(t[0] == "t" for t in required) > 1000
    covered = set()
    for row in pm.rows():
        assert all(row[a] in pm.VALUES[a] for a in range(len(pm.AXES))), row
        covered.update(pm.tuples_of(row))
    missing = [t for t in required if t not in covered]
    assert not missing, missing[:5]


def test_the_array_is_the_same_on_two_builds_and_its_uploads_are_mixed():
    a, b = pm.build(), pm.build()
    assert a == b == pm.rows()
    ups = pm.uploads()
    assert sorted(k for _, ks in ups for k in ks) == list(range(len(a)))
    for settings, ks in ups:  # rows that share their settings, in array order
        assert ks == sorted(ks) and all(a[k][3:] == settings[3:] for k in ks)
    assert len({u[3:] for u, _ in ups}) == len(ups)
    assert sum(len(ks) >= 3 for _, ks in ups) >= len(ups) // 2  # mixed uploads arise by themselves
    assert {(u.arithmetic, u.scale) for u, _ in ups} == {(a_, s) for a_ in pm.ARITHMETICS for s in pm.SCALES}


def test_at_most_a_tenth_of_the_rows_are_refusals():
    rows = pm.rows()
    refused = [r for r in rows if pm.row_expected(r).refused]
    assert [pm.row_refused(r) for r in rows] == [pm.row_expected(r).refused for r in rows]
    assert 0 < len(refused) <= len(rows) // 10, (len(refused), len(rows))
    statuses = {pm.row_expected(r).status for r in refused}
    assert statuses == {pm.NOT_SUPPORTED, pm.ARGUMENT}  # a 4-component file under "ycc", a window outside the oriented reduced frame
    for r in refused:
        o = pm.row_expected(r)
        assert (o.output, o.resized, o.scale, o.arithmetic, o.upsampling, o.channels, o.color, o.orientation) == (None, None, 1, 0, 0, 3, "ycbcr", 1)


def test_the_window_axis_lies_where_it_says_on_every_frame_of_the_array():
    for r in pm.rows():
        plan = pm.frame_plan(pm.file(r.file), r.arithmetic, r.scale, r.color, r.orientation)
        for name in pm.WINDOWS[1:]:
            x, y, w, h = pm.window_rect(name, plan.width, plan.height)
            inside = x + w <= plan.width and y + h <= plan.height
            assert w >= 1 and h >= 1 and inside == (name != "outside"), (r, name)
            if name == "outside" and plan.width != plan.height:
                assert x + w <= plan.height and y + h <= plan.width  # inside the frame turned by a quarter
        assert pm.window_rect("last", plan.width, plan.height) == (plan.width - 1, plan.height - 1, 1, 1)
        assert pm.window_rect("seam", plan.width, plan.height)[::2] == (0, plan.width)


def test_the_fit_size_makes_the_orientation_decide():
    f = pm.file("420")
    assert [pm.frame_plan(f, "libjpeg", "fit", "ycc", o).denom for o in (1, 6)] == [8, 4]
    assert [pm.frame_plan(pm.file("422"), "libjpeg", "fit", "ycc", o).denom for o in (1, 6)] == [2, 1]
    assert pm.frame_plan(f, "reference", "fit", "ycc", 1).denom == 1 and pm.frame_plan(pm.file("odd"), "libjpeg", 4, "ycc", 1)[2:4] == (False, 1)


# ------------------------------------------------------------------------------------------------ 2: one policy at a time

YCC_FILES = [n for n in pm.FILE_NAMES if n not in ("cmyk", "adobe_rgb")]


@pytest.mark.parametrize("name", YCC_FILES)
def test_with_one_policy_set_the_model_is_that_features_model(name):
    f = pm.file(name)
    kind = "gray" if name == "gray" else "ycbcr"
    I = _oracle(name)
    base = cm.as_format(cm.model(kind, I), jl.FMT_RGB_PLANAR_U8)
    o = _expected(name)
    _same(o.output, base, "defaults")
    W, H = im.frame(f)[:2]
    assert (o.status, o.scale, o.arithmetic, o.upsampling, o.channels, o.color, o.orientation, o.window) == (0, 1, 0, 0, 3, kind, 1, (0, 0, W, H))
    # arithmetic, and scale on top of it (a scale under "reference" changes nothing)
    admitted = name != "odd"
    lib = _expected(name, arithmetic="libjpeg")
    assert lib.arithmetic == int(admitted)
    _same(lib.output, cm.as_format(im.decode(f) if admitted else im.rgb(kind, I), jl.FMT_RGB_PLANAR_U8), "libjpeg")
    for denom in sm.DENOMS:
        _same(_expected(name, scale=denom).output, base, "a scale under reference")
        s = _expected(name, arithmetic="libjpeg", scale=denom)
        assert s.scale == (denom if admitted else 1) and s.window == (0, 0) + (sm.out_size(W, H, denom) if admitted else (W, H))
        _same(s.output, cm.as_format(sm.decode(f, denom) if admitted else im.rgb(kind, I), jl.FMT_RGB_PLANAR_U8), "1/%d" % denom)
    # upsampling
    fancy = _expected(name, upsampling="fancy")
    filtered = kind == "ycbcr" and um.qualifies(f)
    assert fancy.upsampling == int(filtered) == int(pm._FILE_SPECS[name][0] in ("filtered", "multiscan"))
    _same(fancy.output, cm.as_format(cm.model(kind, um.filtered(I, *um.ratio(f)) if filtered else I), jl.FMT_RGB_PLANAR_U8), "fancy")
    assert (fancy.output.tobytes() != base.tobytes()) == filtered
    # colour "file" leaves these files alone; grey output
    _same(_expected(name, color="file").output, base, "color=file")
    g = _expected(name, mode="gray", upsampling="fancy")
    assert (g.channels, g.upsampling) == (1, 0)
    _same(g.output, lm.plane(kind, I), "gray")
    assert _expected(name, mode="gray", fmt=jl.FMT_RGB_U8).channels == 3  # (a format without a one-plane form does not read the policy)
    # orientation, windows
    for o_ in om.ORIENTATIONS:
        t = _expected(name, orientation=o_)
        _same(t.output, om.orient_output(o_, base, jl.FMT_RGB_PLANAR_U8), "orientation %d" % o_)
        assert t.orientation == o_ and t.window == (0, 0) + om.oriented_size(o_, H, W)[::-1]
    for wname in pm.WINDOWS[1:4]:
        x, y, w, h = pm.window_rect(wname, W, H)
        _same(_expected(name, window=(x, y, w, h)).output, np.ascontiguousarray(base[:, y:y + h, x:x + w]), wname)
    assert _expected(name, window=pm.window_rect("outside", W, H)).status == pm.ARGUMENT and _expected(name, window=(0, 0, 0, 3)).status == pm.ARGUMENT
    _same(_expected(name, window=(0, 0, 0, 0)).output, base, "{0, 0, 0, 0} is the whole frame")
    # formats, constants, the resize stage
    _same(_expected(name, fmt=jl.FMT_RGB_U8).output, cm.model(kind, I), "RGB_U8")
    _same(_expected(name, fmt=jl.FMT_RGBA_U8).output[..., :3], cm.model(kind, I), "RGBA_U8")
    assert (_expected(name, fmt=jl.FMT_RGBA_U8).output[..., 3] == 255).all()
    for fmt, dt, consts in ((jl.FMT_RGB_PLANAR_F16, np.float16, fm.IMAGENET), (jl.FMT_RGB_PLANAR_F32, np.float32, fm.NEGATIVE)):
        _same(_expected(name, fmt=fmt, consts=consts).output, fm.model(base, consts[0], consts[1], dt), "float sink")
    for dt, consts in ((np.uint8, None), (np.float16, fm.IMAGENET), (np.float32, None)):
        r = _expected(name, consts=consts, resize=pm.RESIZE + (dt,))
        _same(r.output, base, "the per-image output beside a resize")
        _same(r.resized, rm.model(base, 7, 5, dt, *(consts or (None, None))), "resized")
    gr = _expected(name, mode="gray", consts=fm.IMAGENET, resize=pm.RESIZE + (np.float32,))
    _same(gr.resized, rm.model(np.repeat(lm.plane(kind, I), 3, axis=0), 7, 5, np.float32, *fm.IMAGENET)[:1], "resized gray")


@pytest.mark.parametrize("name, kind", [("cmyk", "cmyk"), ("adobe_rgb", "rgb")])
def test_the_by_file_kinds_one_policy_at_a_time(name, kind):
    f = pm.file(name)
    I = _oracle(name)
    assert jl.identify_color(f) == kind == pm.declared_kind(f)
    o = _expected(name, color="file")
    assert o.color == kind and o.slot_bytes == max(3, I.shape[2]) * I.shape[0] * I.shape[1]
    _same(o.output, cm.as_format(cm.model(kind, I), jl.FMT_RGB_PLANAR_U8), "color=file")
    if kind == "cmyk":
        assert _expected(name).status == pm.NOT_SUPPORTED
    else:
        _same(_expected(name).output, cm.as_format(cm.model("ycbcr", I), jl.FMT_RGB_PLANAR_U8), 'three components under "ycc" are YCbCr')
    _same(_expected(name, color="file", mode="gray").output, lm.plane(kind, I), "gray")
    lib = _expected(name, color="file", arithmetic="libjpeg", upsampling="fancy")
    assert (lib.arithmetic, lib.upsampling) == (1, 0)
    _same(lib.output, cm.as_format(im.rgb(kind, im.samples(f)), jl.FMT_RGB_PLANAR_U8), "libjpeg")


def test_the_kind_rule_agrees_with_the_librarys_on_the_colour_tests_files():
    pytest.importorskip("PIL")
    for n in cm.KIND_FILES:
        f, kind = cm.kind_file(n)
        assert pm.declared_kind(f) == kind == jl.identify_color(f), n
    assert pm.declared_kind(cm.subsampled_ycck()) == "ycck"
    assert pm.color_kind(cm.patch_precision(pm.file("420"), 12), "file") == (pm.NOT_SUPPORTED, None)


# ------------------------------------------------------------------------------------------------ 3: Pillow does the whole chain

# what libjpeg filters or does not sub-sample (the three-scan file has its blocks in the order the reference reads them, which is not T.81's)
PILLOW_FILES = ["gray", "444", "420", "420_dri4", "422", "440", "420_progressive"]
_TRANSPOSE = {2: "FLIP_LEFT_RIGHT", 3: "ROTATE_180", 4: "FLIP_TOP_BOTTOM", 5: "TRANSPOSE", 6: "ROTATE_270", 7: "TRANSVERSE", 8: "ROTATE_90"}  # ImageOps.exif_transpose


@pytest.mark.parametrize("name", PILLOW_FILES)
def test_the_model_is_pillows_draft_transpose_crop_convert(name):
    Image = pytest.importorskip("PIL.Image")
    f = pm.file(name)
    W, H = im.frame(f)[:2]
    cells = set()
    for scale in pm.SCALES:
        for o_ in om.ORIENTATIONS:
            for mode, pil_mode in (("rgb", "RGB"), ("gray", "L")):
                img = Image.open(io.BytesIO(f))
                if scale == "fit":
                    ask = (pm.FIT[0], pm.FIT[1]) if o_ >= 5 else (pm.FIT[1], pm.FIT[0])  # (w, h) of the stored frame
                else:
                    ask = (max(1, W // scale), max(1, H // scale))
                img.draft(pil_mode, ask)
                plan = pm.frame_plan(f, "libjpeg", scale, "ycc", o_)
                assert img.size == sm.out_size(W, H, plan.denom) and (scale == "fit" or plan.denom == scale), (scale, o_, img.size)
                img = img.convert(pil_mode)
                if o_ != 1:
                    img = img.transpose(getattr(Image.Transpose, _TRANSPOSE[o_]))
                assert img.size == (plan.width, plan.height)
                for wname in pm.WINDOWS[:4]:
                    rect = pm.window_rect(wname, plan.width, plan.height)
                    x, y, w, h = rect or (0, 0, plan.width, plan.height)
                    want = np.asarray(img.crop((x, y, x + w, y + h)))
                    got = pm.expected(f, arithmetic="libjpeg", scale=scale, upsampling="fancy", color="ycc", mode=mode, orientation=o_, window=rect,
                                      fmt=jl.FMT_RGB_PLANAR_U8, consts=None, resize=None)
                    want = want[None] if mode == "gray" else np.ascontiguousarray(want.transpose(2, 0, 1))
                    _same(got.output, want, "%s: scale %s, orientation %d, window %s, %s" % (name, scale, o_, wname, mode))
                    cells.add((scale, pm.REDUCED[1][1](pm.Row(name, o_, wname, "libjpeg", scale, "fancy", "ycc", mode, "planar_u8")), rect is not None, mode))
    assert len(cells) == len(pm.SCALES) * 3 * 2 * 2
