"""The files the lossless-transform tests share: seeded noise over a gradient, written by Pillow at quality 90 with an asymmetric pair of
quantisation tables (a DQT left untransposed is seen), in the smallest shapes at which the index arithmetic can still go wrong.  Pillow writes
4:4:4, 4:2:2 and 4:2:0; 4:4:0 and 4:1:1 are made from a 4:4:4 file's own blocks (transform_model.assemble).  Nothing is turned here."""
import functools
import io

import numpy as np
from PIL import Image

import transform_model as tm
from oracle import pyoracle as po

# asymmetric under transposition: rows and columns of the natural-order table differ everywhere off the diagonal
QT_LUMA = [2 + 3 * (k // 8) + (k % 8) for k in range(64)]
QT_CHROMA = [3 + (k // 8) + 4 * (k % 8) for k in range(64)]

# name -> (mode, width, height, Pillow subsampling or the factors made from 4:4:4)
SHAPES = {
    "grey_8x8": ("L", 8, 8, None),
    "grey_20x16": ("L", 20, 16, None),
    "444_16x24": ("RGB", 16, 24, 0),
    "420_48x32": ("RGB", 48, 32, 2),
    "422_48x24": ("RGB", 48, 24, 1),
    "440_24x48": ("RGB", 24, 48, [(1, 2), (1, 1), (1, 1)]),
    "411_64x16": ("RGB", 64, 16, [(4, 1), (1, 1), (1, 1)]),
    "420_40x27": ("RGB", 40, 27, 2),
    "420_12x32": ("RGB", 12, 32, 2),
}


def _pixels(mode, width, height, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    chans = 1 if mode == "L" else 3
    base = np.stack([(3 * x + 5 * y + 40 * c) % 256 for c in range(chans)], axis=-1).astype(np.int64)
    img = np.clip(base + rng.integers(-48, 49, base.shape), 0, 255).astype(np.uint8)
    return img[..., 0] if mode == "L" else img


def _with_dri(file, dri):
    """the same blocks under a restart interval (Pillow writes none): the model's own writer around the source's blocks"""
    if not dri:
        return file
    d = bytes(file)
    at = d.index(b"\xff\xda")
    d = d[:at] + b"\xff\xdd\x00\x04" + dri.to_bytes(2, "big") + d[at:]
    fr = tm.frame_of(d)
    coefs, _ = po.decode_coefficients(bytes(file))
    return tm.assemble(d, fr["width"], fr["height"], [(c[1], c[2]) for c in fr["components"]], coefs)


@functools.lru_cache(maxsize=None)
def make(name, dri=0, exif=None, exif_order="little", seed=None):
    """The file of shape `name`; exif: an Orientation value Pillow writes into an Exif block (exif_order "big": the block rewritten as MM)"""
    mode, width, height, sub = SHAPES[name]
    seed = sorted(SHAPES).index(name) + 1 if seed is None else seed
    im = Image.fromarray(_pixels(mode, width, height, seed), mode)
    kw = {"quality": 90, "qtables": [QT_LUMA] if mode == "L" else [QT_LUMA, QT_CHROMA]}
    if mode != "L":
        kw["subsampling"] = sub if isinstance(sub, int) else 0
    if exif is not None:
        kw["exif"] = exif_block(exif, exif_order)
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    file = buf.getvalue()
    if isinstance(sub, list):  # 4:4:0, 4:1:1: the luma blocks as they are, every hs-th / vs-th chroma block
        fr = tm.frame_of(file)
        coefs, _ = po.decode_coefficients(file)
        cols, rows = -(-width // 8), -(-height // 8)
        grids = tm._grids(coefs, [(1, 1)] * 3, cols, rows)
        hmax, vmax = sub[0]
        mcols, mrows = -(-cols // hmax), -(-rows // vmax)
        luma = np.zeros((mrows * vmax, mcols * hmax, 8, 8), np.int16)
        luma[:rows, :cols] = grids[0]
        chroma = [g[::vmax, ::hmax][:mrows, :mcols] for g in grids[1:]]
        file = tm.assemble(file, width, height, sub, tm._scan_order([luma] + chroma, sub, mcols, mrows))
    return _with_dri(file, dri)


def exif_block(orientation, order="little"):
    """"Exif\\0\\0" + a TIFF header + IFD0 with the Orientation tag alone"""
    o = order
    tiff = (b"II" if o == "little" else b"MM") + (42).to_bytes(2, o) + (8).to_bytes(4, o)
    entry = (0x0112).to_bytes(2, o) + (3).to_bytes(2, o) + (1).to_bytes(4, o) + orientation.to_bytes(2, o) + b"\0\0"
    return b"Exif\0\0" + tiff + (1).to_bytes(2, o) + entry + (0).to_bytes(4, o)


def with_stray_bytes(file, before_soi=False):
    """the same file with bytes no segment owns: one between the last DQT and what follows it, three in front of SOS, and (before_soi) two in
    front of SOI.  The reference's reader steps over them (JpegReader.cs: a marker is looked for, not expected), so the optimizer takes the
    file either way; the decoder's Decode() asks for SOI at offset 0, so only the optimizer's untouched road takes the before_soi form."""
    d = bytes(file)
    segs, _ = tm.segments(d)
    after_dqt = max(at + n for m, _, at, n in segs if m == 0xDB)
    sos = [ff for m, ff, _, _ in segs if m == 0xDA][0]
    return (b"\x00\x11" if before_soi else b"") + d[:after_dqt] + b"\x00" + d[after_dqt:sos] + b"\x01\x02\x03" + d[sos:]


def app1_of(file):
    """the payloads of the file's APP1 segments"""
    d = bytes(file)
    return [d[at:at + n] for m, _, at, n in tm.segments(d)[0] if m == 0xE1]
