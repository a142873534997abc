"""The composed model of the decode policies (include/jpgpu.h: "Arithmetic", "Scaled decode", "Chroma upsampling", "Colour", "Grey output",
"Orientation", "Windows", the five RGB formats, the affine constants and the resize stage), and the covering array that walks it.

    expected(file, arithmetic=, scale=, upsampling=, color=, mode=, orientation=, window=, fmt=, consts=, resize=) -> Outcome
        one pure function: the steps in the order the header states them, every stage one of the single-feature models of this directory
        (islow_model, scaled_model, upsample_model, color_model, luma_model, orient_model, float_sink_model, resize_model) over the oracle's
        coefficients and samples.  Nothing here calls the decoder: jpeglibrary_amd is imported for the names of its formats only.
    frame_plan(file, arithmetic, scale, color, orientation) -> Plan
        steps 1 and 2 alone: the colour kind, whether libjpeg's transform is taken, the denominator, the oriented reduced frame
    window_rect(name, ow, oh)   the window axis' symbolic values as rectangles of an oriented, reduced frame of ow x oh pixels
    rows() / uploads()          the covering array (built once, from a fixed seed) and its rows grouped into uploads
    row_outcome(k)              expected() of row k, cached: test_policy_matrix_gpu.py and test_batch_reuse_gpu.py share one computation per row
    required_tuples()           the pairs and triples the array has to cover; tuples_of(row) what one row covers

Rules the model takes from the header, not from the planner:
    colour kind    "ycc": 1 component grey, 3 YCbCr, anything else refused (NOT_SUPPORTED).  "file": libjpeg's rule over JFIF, Adobe and the ids.
    transform      libjpeg's where arithmetic is "libjpeg", the precision is 8, the component count is the kind's, every scan has at most 16 blocks
                   per MCU and replications of 1, 2 or 4, no two sequential scans write one component, no scan names one twice, and no
                   sequential component has several blocks per MCU line or column that are replicated as well.  Else the float transform.
    scale          a denominator above 1 exactly where libjpeg's transform is taken; "fit" is Pillow's draft rule on the oriented frame.
    constants      per upload: under "libjpeg" every YCbCr -> RGB step takes libjpeg's, also in an image that keeps the float transform.
    filter         "fancy", kind YCbCr, 3 components, precision 8, component 0 maximal, chroma ratio (2,1) (2,2) (1,2) in the (reduced)
                   picture, cw > 2 for hs == 2, denominator below 8, and more than one plane asked for.
    refusals       a window outside the oriented reduced frame: ARGUMENT, that image alone; the accessors of a refused image report the
                   defaults the header names for "an image that failed at upload" (scale 1, reference, no filter, 3 channels, YCBCR, orientation 1).
"""
import collections
import itertools
import random
import struct

import numpy as np

import color_model as cm
import float_sink_model as fm
import islow_model as im
import luma_model as lm
import orient_model as om
import resize_model as rm
import scaled_model as sm
import upsample_model as um

OK, NOT_SUPPORTED, ARGUMENT = 0, 3, 4  # jpgpu_status
FIT = (8, 16)  # (h, w): the least size of the "fit" axis value -- 130 x 67 takes 1/8 upright and 1/4 turned, 33 x 17 takes 1/2 and 1/1
RESIZE = (7, 5)  # (oh, ow)

Plan = collections.namedtuple("Plan", "status kind islow denom width height")  # width x height: the oriented (reduced) frame
Outcome = collections.namedtuple("Outcome", "status output resized scale arithmetic upsampling channels color orientation window slot_bytes")
Outcome.refused = property(lambda self: self.status != OK)


# ------------------------------------------------------------------------------------------------ steps 1 and 2: kind, transform, size

def declared_kind(f):
    """libjpeg's rule over the markers between SOI and the first SOS (include/jpgpu.h, "Colour"); None where it refuses the frame"""
    W, H, precision, hv = um.sof_sampling(f)
    ids = [c[0] for c in im.frame(f)[3]]
    jfif, adobe = False, None
    for m, a, b in cm.segments(f):
        p = f[a + 4:b]
        if m == 0xE0 and len(p) >= 14 and p[:5] == b"JFIF\0":
            jfif = True
        if m == 0xEE and len(p) >= 12 and p[:5] == b"Adobe":
            adobe = p[11]
    if precision != 8:
        return None
    if len(hv) == 1:
        return "gray"
    if len(hv) == 3:
        if jfif:
            return "ycbcr"
        if adobe is not None:
            return "rgb" if adobe == 0 else "ycbcr"
        return "rgb" if ids == [ord("R"), ord("G"), ord("B")] else "ycbcr"
    if len(hv) == 4:
        return "ycck" if adobe not in (None, 0) else "cmyk"
    return None


def color_kind(f, color):
    """-> (status, kind)"""
    W, H, precision, hv = um.sof_sampling(f)
    kind = {1: "gray", 3: "ycbcr"}.get(len(hv)) if color == "ycc" else declared_kind(f)
    if kind is None or precision != 8:
        return NOT_SUPPORTED, None
    return OK, kind


def admits_islow(f, kind):
    """does libjpeg's transform apply to the image (the header's rule; every file here is 8-bit and no progressive one is of the kind whose
    Dispose() the reference runs slot by slot)"""
    W, H, progressive, comps = im.frame(f)
    if um.sof_sampling(f)[2] != 8 or len(comps) != {"gray": 1, "ycbcr": 3, "rgb": 3, "cmyk": 4, "ycck": 4}[kind]:
        return False
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    written = set()
    for sc in im.scans(f):
        if len(set(sc)) != len(sc) or sum(comps[c][1] * comps[c][2] for c in sc) > 16:
            return False
        for c in sc:
            h, v = comps[c][1], comps[c][2]
            if hmax % h or vmax % v or hmax // h not in (1, 2, 4) or vmax // v not in (1, 2, 4):
                return False
            if not progressive and ((h > 1 and hmax // h > 1) or (v > 1 and vmax // v > 1)):
                return False
        if not progressive:
            if written & set(sc):
                return False
            written |= set(sc)
    return True


def fit_denominator(w, h, fit):
    """Pillow's draft() rule on the oriented frame w x h; fit = (min_h, min_w)"""
    k = min(w // fit[1], h // fit[0])
    return 8 if k >= 8 else 4 if k >= 4 else 2 if k >= 2 else 1


def frame_plan(f, arithmetic, scale, color, orientation):
    status, kind = color_kind(f, color)
    W, H = im.frame(f)[:2]
    turned = orientation >= 5
    if status != OK:
        return Plan(status, None, False, 1, H if turned else W, W if turned else H)
    islow = arithmetic == "libjpeg" and admits_islow(f, kind)
    denom = 1
    if islow:
        denom = fit_denominator(H if turned else W, W if turned else H, FIT) if scale == "fit" else scale
    Wr, Hr = sm.out_size(W, H, denom)
    return Plan(OK, kind, islow, denom, Hr if turned else Wr, Wr if turned else Hr)


# ------------------------------------------------------------------------------------------------ steps 3 and 4: samples, cached

_STAGE = {}


def _filter_ratio(f, kind, denom, upsampling):
    """(hs, vs) where the header's rule filters the (reduced) picture, else None"""
    W, H, precision, hv = um.sof_sampling(f)
    if upsampling != "fancy" or kind != "ycbcr" or len(hv) != 3 or precision != 8 or denom >= 8:
        return None
    r = um.ratio(f) if denom == 1 else sm.residual_ratio(f, denom)
    if r is None or not um.ratio_filtered(r[0], r[1], sm.out_size(W, H, denom)[0]):
        return None
    return r


def stored_samples(f, islow, denom, ratio):
    """uint8[H', W', C]: the stored samples of step 3, filtered (step 4) where ratio is given; cached, read-only"""
    key = (f, islow, denom, ratio)
    if key not in _STAGE:
        base = (f, islow, denom, None)
        if base not in _STAGE:
            if not islow:
                from oracle import pyoracle

                s = pyoracle.decode_8bit(f)[0]
            else:
                s = im.samples(f) if denom == 1 else sm.samples(f, denom)
            s = np.ascontiguousarray(s)
            s.setflags(write=False)
            _STAGE[base] = s
        if ratio is not None:
            s = um.filtered(_STAGE[base], *ratio)
            s.setflags(write=False)
            _STAGE[key] = s
    return _STAGE[key]


# ------------------------------------------------------------------------------------------------ the composed model

def _planar(fmt):
    import jpeglibrary_amd as jl

    return fmt in (jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_PLANAR_F32)


def _np_dtype(fmt):
    import jpeglibrary_amd as jl

    return {jl.FMT_RGB_PLANAR_F16: np.float16, jl.FMT_RGB_PLANAR_F32: np.float32}.get(fmt, np.uint8)


def _refusal(status):
    return Outcome(status, None, None, 1, 0, 0, 3, "ycbcr", 1, None, 0)


def expected(f, *, arithmetic, scale, upsampling, color, mode, orientation, window, fmt, consts, resize):
    """window: (x, y, w, h) in pixels of the oriented, reduced frame, or None; fmt: one of the five RGB formats; consts: (scale[3], bias[3]) or
    None; resize: (oh, ow, numpy dtype) or None (fmt is then RGB_PLANAR_U8)."""
    import jpeglibrary_amd as jl

    # 1, 2: the colour kind, the transform and its size
    plan = frame_plan(f, arithmetic, scale, color, orientation)
    if plan.status != OK:
        return _refusal(plan.status)
    if window is not None and tuple(window) != (0, 0, 0, 0):
        x, y, w, h = window
        if w == 0 or h == 0 or x + w > plan.width or y + h > plan.height:
            return _refusal(ARGUMENT)
    else:
        x, y, w, h = 0, 0, plan.width, plan.height
    one_plane = mode == "gray" and _planar(fmt)
    # 3, 4: the stored samples, filtered where the rule holds
    ratio = None if one_plane else _filter_ratio(f, plan.kind, plan.denom, upsampling)
    s = stored_samples(f, plan.islow, plan.denom, ratio)
    # 5: RGB or grey; the constants are the upload's
    to_rgb = im.rgb if arithmetic == "libjpeg" else cm.model
    if one_plane:
        px = lm.gray(plan.kind, s) if plan.kind in ("gray", "ycbcr") else lm.L(to_rgb(plan.kind, s))
    else:
        px = to_rgb(plan.kind, s)
    # 6: turn, crop, lay out
    px = np.ascontiguousarray(om.orient(orientation, px)[y:y + h, x:x + w])
    scale3, bias3 = consts if consts is not None else fm.DEFAULT
    if one_plane:
        u8 = px[None]
        out = lm.as_dtype(u8, _np_dtype(fmt), scale3[0], bias3[0])
    else:
        u8 = np.ascontiguousarray(px.transpose(2, 0, 1))
        out = cm.as_format(px, fmt, consts)
    # 7: the resize stage reads the u8 planes
    resized = None
    if resize is not None:
        assert fmt == jl.FMT_RGB_PLANAR_U8
        oh, ow, dt = resize
        planes = np.repeat(u8, 3, axis=0) if one_plane else u8  # (resize_model takes three planes: the same function per plane, constants [0])
        resized = rm.model(planes, oh, ow, dt, scale3, bias3)[:1 if one_plane else 3]
    # the least room the image's slot must have in the output buffer (its samples pass through a scratch slot at the same offset)
    need = out.nbytes
    if plan.kind in ("cmyk", "ycck"):
        need = max(need, 4 * w * h)
    if ratio is not None:
        sx, sy, sw, sh = _stored_window(orientation, (x, y, w, h), s.shape[1], s.shape[0])
        fx, fy, fw, fh = um.fetch_rect(sx, sy, sw, sh, s.shape[1], s.shape[0], *ratio)
        need = max(need, fw * fh * 3 + (3 * w * h if orientation != 1 else 0))
    return Outcome(OK, out, resized, plan.denom, int(plan.islow), int(ratio is not None), 1 if one_plane else 3, plan.kind, orientation,
                   (x, y, w, h), need)


def _stored_window(o, win, W, H):
    """the rectangle of the stored W x H frame that the window of the oriented frame shows"""
    x, y, w, h = win
    ys, xs = om.source_index(o, H, W)
    ys, xs = ys[y:y + h, x:x + w], xs[y:y + h, x:x + w]
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


# ------------------------------------------------------------------------------------------------ the axes

def _four_components(w, h, ids, factors, transform, seed):
    """a 4- or 3-component file from the project's own encoder model, an Adobe APP14 spliced in behind SOI"""
    import encoder_arrangements as ea
    import encoder_model as em

    std = em.standard_tables()
    comps = [em.Component(k, t, t, t, hv, hv, ea.LUM75 if t == 0 else ea.CHR75) for k, (t, hv) in enumerate(factors)]
    arr = em.Arrangement(comps, [(0, ea.LUM75), (1, ea.CHR75)], [(0, 0, std[0]), (1, 0, std[1]), (0, 1, std[2]), (1, 1, std[3])], 0, False)
    f = bytes(em.encode(cm.picture(w, h, len(factors), seed=seed), arr)[0])
    return cm.insert_after_soi(cm.patch_component_ids(f, ids), cm.app14(transform))


def _synth(w, h, sampling, dri, seed, **kw):
    from tools import jpegsynth

    if sampling == "gray":
        return bytes(jpegsynth.encode(w, h, "gray", 75, dri, seed=seed, **kw))
    return bytes(jpegsynth.encode(w, h, "444", 75, dri, seed=seed, sampling=sampling, **kw))


S444, S420, S422, S440, S411, SODD = ((1, 1),) * 3, ((2, 2), (1, 1), (1, 1)), ((2, 1), (1, 1), (1, 1)), ((1, 2), (1, 1), (1, 1)), ((4, 1), (1, 1), (1, 1)), ((2, 1), (4, 1), (1, 1))
# name -> (class of the triples, builder).  130 x 67 is the one size with more than one K3U / K3O tile.
_FILE_SPECS = collections.OrderedDict([
    ("gray", ("gray", lambda: _synth(33, 17, "gray", 0, 1))),
    ("444", ("444", lambda: _synth(35, 19, S444, 0, 2))),
    ("420", ("filtered", lambda: _synth(130, 67, S420, 0, 3))),
    ("420_dri4", ("filtered", lambda: _synth(47, 31, S420, 4, 4))),
    ("422", ("filtered", lambda: _synth(33, 17, S422, 4, 5))),
    ("440", ("filtered", lambda: _synth(34, 50, S440, 0, 6))),
    ("411", ("unfiltered", lambda: _synth(70, 33, S411, 0, 7))),
    ("420_progressive", ("multiscan", lambda: _synth(33, 17, S420, 0, 8, progressive=True))),
    ("422_three_scans", ("multiscan", lambda: _synth(45, 23, S422, 4, 9, noninterleaved=True))),
    ("odd", ("unfiltered", lambda: _synth(70, 33, SODD, 3, 10))),
    ("cmyk", ("byfile", lambda: _four_components(45, 37, (ord("C"), ord("M"), ord("Y"), ord("K")), [(0, 1)] * 4, 0, 11))),
    ("adobe_rgb", ("byfile", lambda: _four_components(37, 21, (ord("R"), ord("G"), ord("B")), [(0, 1)] * 3, 0, 12))),
])
FILE_NAMES = tuple(_FILE_SPECS)
_FILES = {}


def file(name):
    if name not in _FILES:
        _FILES[name] = _FILE_SPECS[name][1]()
    return _FILES[name]


ORIENTATIONS = (1, 2, 3, 4, 5, 6, 7, 8)
WINDOWS = ("none", "interior", "last", "seam", "outside")
ARITHMETICS = ("reference", "libjpeg")
SCALES = (1, 2, 4, 8, "fit")
UPSAMPLINGS = ("replicate", "fancy")
COLORS = ("ycc", "file")
MODES = ("rgb", "gray")
SINKS = ("rgb_u8", "rgba_u8", "planar_u8", "planar_f16_imagenet", "planar_f32_negative", "resize_u8", "resize_f16_imagenet", "resize_f32")
SINK_CLASS = {"rgb_u8": "pixels", "rgba_u8": "pixels", "planar_u8": "planar", "planar_f16_imagenet": "float", "planar_f32_negative": "float",
              "resize_u8": "resized", "resize_f16_imagenet": "resized", "resize_f32": "resized"}


def sink(name):
    """-> (fmt, consts, resize) as expected() takes them"""
    import jpeglibrary_amd as jl

    return {"rgb_u8": (jl.FMT_RGB_U8, None, None), "rgba_u8": (jl.FMT_RGBA_U8, None, None), "planar_u8": (jl.FMT_RGB_PLANAR_U8, None, None),
            "planar_f16_imagenet": (jl.FMT_RGB_PLANAR_F16, fm.IMAGENET, None), "planar_f32_negative": (jl.FMT_RGB_PLANAR_F32, fm.NEGATIVE, None),
            "resize_u8": (jl.FMT_RGB_PLANAR_U8, None, RESIZE + (np.uint8,)), "resize_f16_imagenet": (jl.FMT_RGB_PLANAR_U8, fm.IMAGENET, RESIZE + (np.float16,)),
            "resize_f32": (jl.FMT_RGB_PLANAR_U8, None, RESIZE + (np.float32,))}[name]


def window_rect(name, ow, oh):
    """the window axis on an oriented, reduced frame of ow x oh pixels"""
    if name == "none":
        return None
    if name == "interior":  # odd origin, odd sizes where the frame has the room
        def span(n):
            at = 1 if n >= 3 else 0
            size = max(1, n - 1 - at)
            return at, size - (1 if size > 1 and size % 2 == 0 else 0)
        (x, w), (y, h) = span(ow), span(oh)
        return (x, y, w, h)
    if name == "last":
        return (ow - 1, oh - 1, 1, 1)
    if name == "seam":  # every column of the rows around the first MCU seam that 16 stored lines (8 of a short frame) leave in the frame
        s = min(oh - 1, max(1, oh // 2 if oh < 16 else 16 if oh > 17 else 8))
        return (0, s - 1, ow, min(3, oh - s + 1))
    if name == "outside":  # inside the frame turned by a quarter, outside this one; beside a square frame
        return (oh - 1, 0, 1, 1) if ow < oh else (0, ow - 1, 1, 1) if oh < ow else (ow, 0, 1, 1)
    raise ValueError(name)


AXES = ("file", "orientation", "window", "arithmetic", "scale", "upsampling", "color", "mode", "sink")
VALUES = (FILE_NAMES, ORIENTATIONS, WINDOWS, ARITHMETICS, SCALES, UPSAMPLINGS, COLORS, MODES, SINKS)
UPLOAD_AXES = (3, 4, 5, 6, 7, 8)
Row = collections.namedtuple("Row", AXES)


def row_expected(row):
    f = file(row.file)
    plan = frame_plan(f, row.arithmetic, row.scale, row.color, row.orientation)
    fmt, consts, resize = sink(row.sink)
    return expected(f, arithmetic=row.arithmetic, scale=row.scale, upsampling=row.upsampling, color=row.color, mode=row.mode, orientation=row.orientation,
                    window=window_rect(row.window, plan.width, plan.height), fmt=fmt, consts=consts, resize=resize)


_OUTCOME = {}


def row_outcome(k):
    """row_expected of row k of rows(), computed once for every suite that walks the array and never changed"""
    if k not in _OUTCOME:
        _OUTCOME[k] = row_expected(rows()[k])
    return _OUTCOME[k]


def row_refused(row):
    """cheap: is the row's outcome a refusal (no samples are computed)"""
    f = file(row.file)
    plan = frame_plan(f, row.arithmetic, row.scale, row.color, row.orientation)
    return plan.status != OK or row.window == "outside"


# ------------------------------------------------------------------------------------------------ the covering array

# the road-choosing axes, reduced: (name, function of a row)
REDUCED = (
    ("file", lambda r: _FILE_SPECS[r.file][0]),
    ("orientation", lambda r: "upright" if r.orientation == 1 else "mirrored" if r.orientation < 5 else "transposed"),
    ("window", lambda r: r.window != "none"),
    ("arithmetic_scale", lambda r: "reference" if r.arithmetic == "reference" else "full" if r.scale == 1 else "eighth" if r.scale == 8 else "reduced"),
    ("upsampling", lambda r: r.upsampling),
    ("mode", lambda r: r.mode),
    ("sink", lambda r: SINK_CLASS[r.sink]),
)
REDUCED_VALUES = (("gray", "444", "filtered", "unfiltered", "multiscan", "byfile"), ("upright", "mirrored", "transposed"), (False, True),
                  ("reference", "full", "reduced", "eighth"), UPSAMPLINGS, MODES, ("pixels", "planar", "float", "resized"))
_REDUCED_UPLOAD = (3, 4, 5, 6)  # the reduced axes an upload's settings decide


def tuples_of(row):
    """what a row covers: ("p", a, va, b, vb) for every pair of axes, ("t", a, va, b, vb, c, vc) for every triple of reduced axes"""
    out = [("p", a, row[a], b, row[b]) for a, b in itertools.combinations(range(len(AXES)), 2)]
    red = [fn(row) for _, fn in REDUCED]
    out += [("t", a, red[a], b, red[b], c, red[c]) for a, b, c in itertools.combinations(range(len(REDUCED)), 3)]
    return out


def required_tuples():
    """every pair of values over all axes, every triple over the reduced axes -- enumerated from the value lists, not from rows"""
    out = []
    for a, b in itertools.combinations(range(len(AXES)), 2):
        out += [("p", a, va, b, vb) for va in VALUES[a] for vb in VALUES[b]]
    for a, b, c in itertools.combinations(range(len(REDUCED)), 3):
        out += [("t", a, va, b, vb, c, vc) for va in REDUCED_VALUES[a] for vb in REDUCED_VALUES[b] for vc in REDUCED_VALUES[c]]
    return out


def _fixed_by(t):
    """the axis values a tuple pins: {axis: allowed values}"""
    if t[0] == "p":
        return {t[1]: (t[2],), t[3]: (t[4],)}
    fixed = {}
    for a, v in ((t[1], t[2]), (t[3], t[4]), (t[5], t[6])):
        name = REDUCED[a][0]
        if name == "arithmetic_scale":
            fixed[3] = ("reference",) if v == "reference" else ("libjpeg",)
            fixed[4] = SCALES if v == "reference" else {"full": (1,), "eighth": (8,), "reduced": (2, 4, "fit")}[v]
        elif name == "file":
            fixed[0] = tuple(n for n in FILE_NAMES if _FILE_SPECS[n][0] == v)
        elif name == "orientation":
            fixed[1] = {"upright": (1,), "mirrored": (2, 3, 4), "transposed": (5, 6, 7, 8)}[v]
        elif name == "window":
            fixed[2] = WINDOWS[1:] if v else ("none",)
        elif name == "sink":
            fixed[8] = tuple(s for s in SINKS if SINK_CLASS[s] == v)
        else:
            fixed[AXES.index(name)] = (v,)
    return fixed


def build(seed=20240229, tries=24):
    """A greedy builder from a fixed seed, in two passes.  First the uploads: settings tuples until every pair and reduced triple among the
    upload axes has one.  Then the rows: for the first tuple (in enumeration order) that no row covers yet, `tries` random rows that pin its
    values and sit in one of the uploads that allow it; the one that covers most new tuples is taken -- a row that would be refused only where
    the tuple asks for it.  Rows come out grouped by upload, uploads in the order of the first pass."""
    rng = random.Random(seed)
    required = required_tuples()
    # pass 1: the uploads
    def upload_tuples(u):
        probe = Row(FILE_NAMES[0], 1, "none", *u)
        red = [fn(probe) for _, fn in REDUCED]
        out = [("p", a, probe[a], b, probe[b]) for a, b in itertools.combinations(UPLOAD_AXES, 2)]
        return out + [("t", a, red[a], b, red[b], c, red[c]) for a, b, c in itertools.combinations(_REDUCED_UPLOAD, 3)]

    def upload_level(t):
        return all(a in UPLOAD_AXES for a in t[1::2]) if t[0] == "p" else all(a in _REDUCED_UPLOAD for a in t[1::2])

    todo = [t for t in required if upload_level(t)]
    left = set(todo)
    uploads = []
    while left:
        first = next(t for t in todo if t in left)
        fixed = _fixed_by(first)
        best, best_gain = None, 0
        for _ in range(tries):
            u = tuple(rng.choice(fixed.get(a, VALUES[a])) for a in UPLOAD_AXES)
            gain = sum(1 for t in upload_tuples(u) if t in left)  # (at least 1: the tuple itself, so a settings tuple is never taken twice)
            if gain > best_gain:
                best, best_gain = u, gain
        uploads.append(best)
        left -= set(upload_tuples(best))
    # pass 2: the rows
    per_upload = [[] for _ in uploads]
    left = set(required)
    for t in required:
        if t not in left:
            continue
        fixed = _fixed_by(t)
        fits = [k for k, u in enumerate(uploads) if all(u[a - 3] in fixed[a] for a in fixed if a in UPLOAD_AXES)]
        assert fits, t
        wants_refusal = fixed.get(2) == ("outside",) or (fixed.get(0) == ("cmyk",) and fixed.get(6) == ("ycc",))
        best, best_score = None, None
        for _ in range(tries):
            k = rng.choice(fits)
            row = Row(*(tuple(rng.choice(fixed.get(a, VALUES[a])) for a in (0, 1, 2)) + uploads[k]))
            gain = sum(1 for x in tuples_of(row) if x in left)
            score = (wants_refusal or not row_refused(row), gain - 2 * len(per_upload[k]))  # (and a slight pull towards the shorter uploads)
            if best_score is None or score > best_score:
                best, best_score = (k, row), score
        per_upload[best[0]].append(best[1])
        left -= set(tuples_of(best[1]))
        assert t not in left
    return [row for rows in per_upload for row in rows]


_ROWS = []


def rows():
    if not _ROWS:
        _ROWS.extend(build())
    return list(_ROWS)


def uploads():
    """[(settings Row with the image axes None, [row index])]: rows that share their upload settings, in array order"""
    groups = collections.OrderedDict()
    for k, r in enumerate(rows()):
        groups.setdefault(r[3:], []).append(k)
    return [(Row(None, None, None, *u), ks) for u, ks in groups.items()]
