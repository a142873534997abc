"""The window of the optimizer's lossless transform (include/jpgpu.h section (5), "Window"), in numpy, on top of tests/transform_model.py.

    plan(frame, o, edge, window, origin)      the geometry: the turned frame F', the applied window, the MCUs it keeps
    write_cropped(file, o, edge, window, ...)  the file F'': the MCUs of F' the window keeps, coded with the Annex K tables under the source's DRI
    expected(file, ...)                        po.optimize(write_cropped(...), strip): what the library must write

A window is a slice of the MCU grid of F' and a size in the SOF; nothing else is new.  Nothing here imports the library under test."""
import transform_model as tm
from oracle import pyoracle as po

Refused = tm.Refused


class BadWindow(Exception):
    """The window fails the image (JPGPU_ERR_ARGUMENT); .word is "outside" or "zero"."""

    def __init__(self, word):
        super().__init__(word)
        self.word = word


def plan(frame, o, edge="refuse", window=None, origin="refuse"):
    """tm.plan() of the whole frame first (the orientation and the edge policy do not see the window), then the window in the frame of F'.
    Adds "frame" (W', H'), "mcu" (mw, mh), "window" (as applied), "origin_mcu" (ox, oy); "width", "height" and "mcus" become the window's."""
    pl = dict(tm.plan(frame, o, edge))
    mw, mh = 8 * max(h for h, _ in pl["factors"]), 8 * max(v for _, v in pl["factors"])
    pl["frame"], pl["mcu"] = (pl["width"], pl["height"]), (mw, mh)
    if window is None or tuple(window) == (0, 0, 0, 0):
        pl["window"], pl["origin_mcu"] = (0, 0, pl["width"], pl["height"]), (0, 0)
        return pl
    x, y, w, h = window
    if w == 0 or h == 0:
        raise BadWindow("zero")
    if x + w > pl["width"] or y + h > pl["height"]:
        raise BadWindow("outside")
    if x % mw or y % mh:
        if origin != "expand":
            raise Refused("origin", "x" if x % mw else "y")
        x, w, y, h = x - x % mw, w + x % mw, y - y % mh, h + y % mh
    pl["window"], pl["origin_mcu"] = (x, y, w, h), (x // mw, y // mh)
    pl["width"], pl["height"], pl["mcus"] = w, h, (-(-w // mw), -(-h // mh))
    return pl


def crop_blocks(coefs, frame, o, edge="refuse", window=None, origin="refuse"):
    """coefs[nblocks, 64] of F -> the blocks of F'' (zig-zag, MCU order of the window's grid)"""
    pl = plan(frame, o, edge, window, origin)
    whole = tm.plan(frame, o, edge)
    turned = tm.turn_blocks(coefs, frame, o, edge)
    (ox, oy), (cols, rows) = pl["origin_mcu"], pl["mcus"]
    grids = [g[oy * v:(oy + rows) * v, ox * h:(ox + cols) * h] for g, (h, v) in zip(tm._grids(turned, whole["factors"], *whole["mcus"]), whole["factors"])]
    return tm._scan_order(grids, pl["factors"], cols, rows)


def write_cropped(file, o=1, edge="refuse", window=None, origin="refuse", from_file=False):
    """F'' (see the module's head).  from_file: the orientation is the file's own (policy "file"): its Exif tag is rewritten to 1."""
    fr = tm.frame_of(file)
    pl = plan(fr, o, edge, window, origin)
    coefs, _ = po.decode_coefficients(bytes(file))
    return tm.assemble(file, pl["width"], pl["height"], pl["factors"], crop_blocks(coefs, fr, o, edge, window, origin), o >= 5, from_file)


def expected(file, o=1, edge="refuse", window=None, origin="refuse", strip=True, most_optimal=False, from_file=False):
    return po.optimize(write_cropped(file, o, edge, window, origin, from_file), strip, most_optimal)
