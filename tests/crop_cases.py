"""The files the lossless-window tests share: the shapes of tests/transform_cases.py, and two more made the same way (seeded noise over a
gradient, Pillow, quality 90, the asymmetric tables) that are large enough to cross a 256-block work entry of KX:

    420_160x128   10 x 8 MCUs of six blocks: a (16, 16, 128, 96) window is 288 blocks, the whole frame 480
    444_136x40    17 x 5 MCUs, the last column partial in the source

and the windows the tests use, derived from the model's geometry so that they hold for every sampling."""
import functools
import io

from PIL import Image

import crop_model as cm
import transform_cases as tc
import transform_model as tm

EXTRA = {
    "420_160x128": ("RGB", 160, 128, 2, 101),
    "444_136x40": ("RGB", 136, 40, 0, 102),
}
ALL = list(tc.SHAPES) + list(EXTRA)


@functools.lru_cache(maxsize=None)
def make(name, dri=0, exif=None):
    if name in tc.SHAPES:
        return tc.make(name, dri, exif)
    mode, width, height, sub, seed = EXTRA[name]
    kw = {"quality": 90, "qtables": [tc.QT_LUMA, tc.QT_CHROMA], "subsampling": sub}
    if exif is not None:
        kw["exif"] = tc.exif_block(exif)
    buf = io.BytesIO()
    Image.fromarray(tc._pixels(mode, width, height, seed), mode).save(buf, "JPEG", **kw)
    return tc._with_dri(buf.getvalue(), dri)


def geometry(name, o=1, edge="refuse"):
    """(W', H', mw, mh) of the turned frame of shape `name`"""
    pl = cm.plan(tm.frame_of(make(name)), o, edge)
    return pl["frame"] + pl["mcu"]


def interior_window(name, o=1, edge="refuse"):
    """one MCU, as far from the frame's origin as an interior MCU can be (the second column / row where there is one)"""
    W, H, mw, mh = geometry(name, o, edge)
    x, y = mw if W >= 2 * mw else 0, mh if H >= 2 * mh else 0
    return (x, y, min(mw, W - x), min(mh, H - y))


def edge_window(name, o=1, edge="refuse"):
    """from the last MCU column and row that start inside the frame, to the frame's right and bottom edge: a partial last MCU where the
    frame has one (the padding blocks of F' come along)"""
    W, H, mw, mh = geometry(name, o, edge)
    x, y = (W - 1) // mw * mw, (H - 1) // mh * mh
    return (x, y, W - x, H - y)


def off_centre_window(name, o, edge="refuse"):
    """one MCU wide and two tall, in the last whole MCU column, from the second MCU row on where the frame has three -- one column to the left
    where that would put it at the same MCU index along both axes: a wrong origin axis, a mirror counted from the wrong edge or a swapped width
    and height all move it or change its size"""
    W, H, mw, mh = geometry(name, o, edge)
    assert W >= 2 * mw and H >= 2 * mh, (name, o)
    ox, oy = W // mw - 1, 1 if H >= 3 * mh else 0
    if ox == oy:
        ox -= 1
    return (ox * mw, oy * mh, mw, 2 * mh)
