"""The numpy model of the orientation feature (include/jpgpu.h, "Orientation") that the orientation tests share, and the Exif blocks they build their
inputs with.

Model.  With H x W the stored frame and (Y, X) a pixel of the output, the source pixel (y, x) is
    1 (Y, X)   2 (Y, W-1-X)   3 (H-1-Y, W-1-X)   4 (H-1-Y, X)   5 (X, Y)   6 (H-1-X, Y)   7 (H-1-X, W-1-Y)   8 (X, W-1-Y)
orient(o, a) applies it to an array whose two pixel axes are given; source_index(o, H, W) gives the table itself, as index arrays."""
import struct

import numpy as np

import color_model as cm

ORIENTATIONS = (1, 2, 3, 4, 5, 6, 7, 8)


def oriented_size(o, h, w):
    """(H', W') of the output"""
    return (w, h) if o >= 5 else (h, w)


def source_index(o, h, w):
    """(y, x): two int arrays of the output's shape, the source pixel of every output pixel -- the table, literally"""
    oh, ow = oriented_size(o, h, w)
    Y, X = np.mgrid[0:oh, 0:ow]
    return {1: (Y, X), 2: (Y, w - 1 - X), 3: (h - 1 - Y, w - 1 - X), 4: (h - 1 - Y, X),
            5: (X, Y), 6: (h - 1 - X, Y), 7: (h - 1 - X, w - 1 - Y), 8: (X, w - 1 - Y)}[o]


def orient(o, a, axes=(0, 1)):
    """a: an array whose axes[0] is y and axes[1] is x (uint8[H, W, C]: (0, 1); [3, H, W] planes: (1, 2)) -> the oriented array, contiguous"""
    ay, ax = axes
    a = np.moveaxis(np.asarray(a), (ay, ax), (0, 1))
    y, x = source_index(o, a.shape[0], a.shape[1])
    return np.ascontiguousarray(np.moveaxis(a[y, x], (0, 1), (ay, ax)))


def orient_output(o, out, fmt):
    """Batch.output(i) under orientation 1 -> what it is under orientation o: [H, W, C] pixels (RGB_U8, RGBA_U8) or [3, H, W] planes"""
    import jpeglibrary_amd as jl

    return orient(o, out, (0, 1) if fmt in (jl.FMT_RGB_U8, jl.FMT_RGBA_U8) else (1, 2))


# ------------------------------------------------------------------------------------------------ Exif blocks

def tiff(o=None, order="MM", entries=None, magic=42, ifd_offset=8, count=None, typ=3, n=1, pad=b"", ifd_at=None):
    """The bytes behind "Exif\\0\\0": a TIFF header and IFD0.  entries: [(tag, type, count, value bytes (4))]; by default two harmless tags
    around the orientation o (None: no orientation entry).  count: the entry count written (default: the real one).  ifd_offset: the offset
    written; ifd_at: where IFD0 really lies (default: there)."""
    e = ">" if order == "MM" else "<"

    def short_value(v):
        return struct.pack(e + "HH", v, 0)

    if entries is None:
        entries = [(0x010F, 2, 4, b"abc\0")]
        if o is not None:
            entries.append((0x0112, typ, n, short_value(o) if typ == 3 else struct.pack(e + "I", o)))
        entries.append((0x0131, 2, 4, b"xyz\0"))
    ifd = struct.pack(e + "H", len(entries) if count is None else count)
    for tag, t, c, v in entries:
        ifd += struct.pack(e + "HHI", tag, t, c) + v
    ifd += struct.pack(e + "I", 0)
    head = order.encode() + struct.pack(e + "HI", magic, ifd_offset)
    return head + b"\0" * max(0, (ifd_offset if ifd_at is None else ifd_at) - 8) + ifd + pad


def exif_segment(o, order="MM", **kw):
    """an APP1 "Exif" segment whose IFD0 holds orientation o (see tiff() for the ways to break it)"""
    return cm.segment(0xE1, b"Exif\0\0" + tiff(o, order, **kw))


def with_orientation(f, o, order="MM", **kw):
    """file f with such a segment behind SOI"""
    return cm.insert_after_soi(f, exif_segment(o, order, **kw))


XMP = cm.segment(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta/>")
