"""The lossless transform of the optimizer (include/jpgpu.h section (5), "Lossless transform"), in numpy and plain Python.

    turn_blocks(coefs, frame, orientation, edge)   the blocks of F' from the blocks of F
    write_turned(file, orientation, edge)          the file F': the source's segments with the SOF / DQT / Exif patches, the turned blocks
                                                   coded with the Annex K tables under the source's DRI
    expected(file, ...)                            po.optimize(write_turned(...), strip): what the library must write

Everything follows from ONE table, source_pixel(): the source-pixel table of the header's orientation section.  Blocks are relocated by it in
units of blocks, and a block's coefficients are what the 2-D DCT makes of a mirrored or transposed 8 x 8 tile: a mirror along an axis negates the
odd frequencies of that axis, a transposition swaps the two frequencies.  Nothing here imports the library under test."""
import numpy as np

import encoder_model
from oracle import pyoracle as po
from scan_writer import BitWriter, block_symbols

INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}


class Refused(Exception):
    """The image is refused (JPGPU_ERR_NOT_SUPPORTED); .axis is "width" or "height" for an edge refusal."""

    def __init__(self, message, axis=None):
        super().__init__(message)
        self.axis = axis


def source_pixel(o, Y, X, H, W):
    """(y, x) of the stored H x W frame that output pixel (Y, X) shows under orientation o: the table of include/jpgpu.h"""
    return {1: (Y, X), 2: (Y, W - 1 - X), 3: (H - 1 - Y, W - 1 - X), 4: (H - 1 - Y, X),
            5: (X, Y), 6: (H - 1 - X, Y), 7: (H - 1 - X, W - 1 - Y), 8: (X, W - 1 - Y)}[o]


def mirrors(o):
    """(source x is mirrored, source y is mirrored, the axes are swapped), read off the table on a 2 x 3 frame"""
    y0, x0 = source_pixel(o, 0, 0, 2, 3)
    return x0 != 0, y0 != 0, o >= 5


def turn_pixels(a, o):
    """a[H, W, ...] under orientation o, pixel by pixel from the table (numpy indexing)"""
    H, W = a.shape[:2]
    oh, ow = (W, H) if o >= 5 else (H, W)
    Y, X = np.mgrid[0:oh, 0:ow]
    y, x = source_pixel(o, Y, X, H, W)
    return a[y, x]


# ---------------------------------------------------------------------------------------------- segments
ZIGZAG = []  # zig-zag position -> (v, u)
for _s in range(15):
    for _t in range(_s + 1):
        _v = _t if _s & 1 else _s - _t
        if _v < 8 and _s - _v < 8:
            ZIGZAG.append((_v, _s - _v))
ZZ_OF = {vu: k for k, vu in enumerate(ZIGZAG)}


def segments(file):
    """[(marker, offset of the FF, payload offset, payload length)] of the segments up to and including SOS.  Markers are found the way the
    reference's reader finds them: bytes in front of one are stepped over, and so are fill bytes, SOI and RSTn."""
    d, p, out = bytes(file), 0, []
    while True:
        p = d.index(b"\xff", p)
        if d[p + 1] in (0xFF, 0x00):
            p += 1 if d[p + 1] == 0xFF else 2
            continue
        if d[p + 1] == 0xD8 or 0xD0 <= d[p + 1] <= 0xD7:
            p += 2
            continue
        m, n = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        out.append((m, p, p + 4, n - 2))
        p += 2 + n
        if m == 0xDA:
            return out, p


def frame_of(file):
    """{"width", "height", "components": [(id, h, v, tq)], "dri", "tables": [(class, id)] in the DHT's order}"""
    d = bytes(file)
    segs, scan_at = segments(d)
    fr = {"dri": 0, "tables": [], "scan_at": scan_at}
    for m, _, at, n in segs:
        if m in (0xC0, 0xC1):
            fr["height"], fr["width"] = (d[at + 1] << 8) | d[at + 2], (d[at + 3] << 8) | d[at + 4]
            fr["components"] = [(d[at + 6 + 3 * c], d[at + 7 + 3 * c] >> 4, d[at + 7 + 3 * c] & 15, d[at + 8 + 3 * c]) for c in range(d[at + 5])]
        elif m == 0xC2:
            raise Refused("progressive")
        elif m == 0xDD:
            fr["dri"] = (d[at] << 8) | d[at + 1]
        elif m == 0xC4:
            q = at
            while q < at + n:
                fr["tables"].append((d[q] >> 4, d[q] & 15))
                q += 17 + sum(d[q + 1:q + 17])
        elif m == 0xDA:
            fr["scan"] = [(d[at + 1 + 2 * c], d[at + 2 + 2 * c] >> 4, d[at + 2 + 2 * c] & 15) for c in range(d[at])]
    return fr


def plan(frame, o, edge="refuse"):
    """The geometry of the turned image: what is kept of the source, the output's size and factors"""
    comps = frame["components"]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mw, mh = 8 * hmax, 8 * vmax
    kw, kh, trimmed = frame["width"], frame["height"], False
    mx, my, swap = mirrors(o)
    if mx and kw % mw:
        if edge != "trim" or kw < mw:
            raise Refused("width", "width")
        kw, trimmed = kw - kw % mw, True
    if my and kh % mh:
        if edge != "trim" or kh < mh:
            raise Refused("height", "height")
        kh, trimmed = kh - kh % mh, True
    cols, rows = -(-kw // mw), -(-kh // mh)
    return {"orientation": o, "trimmed": trimmed, "kept": (kw, kh), "kept_mcus": (cols, rows), "src_mcus": (-(-frame["width"] // mw), -(-frame["height"] // mh)),
            "width": kh if swap else kw, "height": kw if swap else kh, "mcus": (rows, cols) if swap else (cols, rows),
            "factors": [(c[2], c[1]) if swap else (c[1], c[2]) for c in comps]}


# ---------------------------------------------------------------------------------------------- blocks
def _grids(coefs, factors, cols, rows):
    """scan-order zig-zag blocks -> per component [rows * v, cols * h, 8, 8] arrays c[by, bx, v, u]"""
    bpm = sum(h * v for h, v in factors)
    coefs = np.asarray(coefs).reshape(rows, cols, bpm, 64)
    nat = np.zeros((rows, cols, bpm, 8, 8), coefs.dtype)
    for k, (v, u) in enumerate(ZIGZAG):
        nat[..., v, u] = coefs[..., k]
    out, b = [], 0
    for h, v in factors:
        g = nat[:, :, b:b + h * v].reshape(rows, cols, v, h, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(rows * v, cols * h, 8, 8)
        out.append(g)
        b += h * v
    return out


def _scan_order(grids, factors, cols, rows):
    parts = [g.reshape(rows, v, cols, h, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(rows, cols, h * v, 8, 8) for g, (h, v) in zip(grids, factors)]
    nat = np.concatenate(parts, axis=2)
    out = np.zeros(nat.shape[:3] + (64,), nat.dtype)
    for k, (v, u) in enumerate(ZIGZAG):
        out[..., k] = nat[..., v, u]
    return out.reshape(-1, 64)


def turn_blocks(coefs, frame, o, edge="refuse"):
    """coefs[nblocks, 64] of F (po.decode_coefficients: zig-zag, scan order) -> the blocks of F', same form"""
    pl = plan(frame, o, edge)
    src_factors = [(c[1], c[2]) for c in frame["components"]]
    (scols, srows), (kcols, krows), (cols, rows) = pl["src_mcus"], pl["kept_mcus"], pl["mcus"]
    mx, my, swap = mirrors(o)
    sign_u = np.where(np.arange(8) % 2 == 1, -1, 1).astype(np.int16)
    out = []
    for g, (h, v) in zip(_grids(coefs, src_factors, scols, srows), src_factors):
        g = g[:krows * v, :kcols * h]  # (a trimmed edge: the last MCU column or row of the mirrored axis goes)
        H, W = g.shape[:2]
        oh, ow = (W, H) if swap else (H, W)
        Y, X = np.mgrid[0:oh, 0:ow]
        y, x = source_pixel(o, Y, X, H, W)  # block (Y, X) of the output is block (y, x) of the source
        t = g[y, x].copy()
        if mx:
            t = (t * sign_u[None, None, None, :]).astype(np.int16)   # odd u
        if my:
            t = (t * sign_u[None, None, :, None]).astype(np.int16)   # odd v
        if swap:
            t = t.transpose(0, 1, 3, 2)
        out.append(t)
    return _scan_order(out, pl["factors"], cols, rows)


# ---------------------------------------------------------------------------------------------- the file F'
def _std_table(cls, ident):
    """Annex K: luminance tables for identifier 0, chrominance for the others"""
    std = encoder_model.standard_tables()
    return std[(2 if ident else 0) + cls]


def _dht_payload(cls, ident):
    codes = _std_table(cls, ident)
    bits = [sum(1 for _, _, n in codes if n == ln) for ln in range(1, 17)]
    return bytes([(cls << 4) | ident]) + bytes(bits) + bytes(s for s, _, _ in codes)


def exif_value_at(file):
    """(offset of the two value bytes of the Orientation tag the identify rule reads, little-endian?) or None"""
    d = bytes(file)
    for m, _, at, n in segments(d)[0]:
        if m == 0xE1 and d[at:at + 6] == b"Exif\0\0":
            t = d[at + 6:at + n]
            if len(t) < 8 or t[:2] not in (b"II", b"MM"):
                return None
            order = "little" if t[:2] == b"II" else "big"
            u = lambda a, k: int.from_bytes(t[a:a + k], order)
            if u(2, 2) != 42:
                return None
            ifd = u(4, 4)
            if ifd + 2 > len(t):
                return None
            for k in range(u(ifd, 2)):
                e = ifd + 2 + 12 * k
                if e + 12 > len(t):
                    return None
                if u(e, 2) == 0x0112:
                    if u(e + 2, 2) != 3 or u(e + 4, 4) != 1 or not 1 <= u(e + 8, 2) <= 8:
                        return None
                    return at + 6 + e + 8, order == "little"
            return None
    return None


def assemble(file, width, height, factors, blocks, swap_dqt=False, from_file=False):
    """The source's segments around other blocks: SOF size and factors as given, every DQT transposed (swap_dqt), every DHT table replaced by the
    Annex K table of its class and identifier, the Exif tag rewritten to 1 (from_file), then `blocks` (zig-zag, MCU order of `factors`) coded
    with those tables under the source's DRI, then whatever follows the source's scan."""
    d = bytearray(file)
    fr = frame_of(d)
    assert [s[0] for s in fr["scan"]] == [c[0] for c in fr["components"]], "one scan with every component"
    segs, scan_at = segments(d)
    if from_file:
        at, little = exif_value_at(d)
        d[at:at + 2] = (1).to_bytes(2, "little" if little else "big")
    out = bytearray(b"\xff\xd8")
    for m, ff, at, n in segs:
        body = bytearray(d[at:at + n])
        if m in (0xC0, 0xC1):
            body[1:3] = height.to_bytes(2, "big")
            body[3:5] = width.to_bytes(2, "big")
            for c, (h, v) in enumerate(factors):
                body[7 + 3 * c] = (h << 4) | v
        elif m == 0xDB and swap_dqt:
            q = 0
            while q < n:
                size = 2 if body[q] >> 4 else 1
                old = bytes(body[q + 1:q + 1 + 64 * size])
                for k, (v, u) in enumerate(ZIGZAG):
                    j = ZZ_OF[(u, v)]
                    body[q + 1 + k * size:q + 1 + (k + 1) * size] = old[j * size:(j + 1) * size]
                q += 1 + 64 * size
        elif m == 0xC4:
            q, new = 0, bytearray()
            while q < n:
                new += _dht_payload(body[q] >> 4, body[q] & 15)
                q += 17 + sum(body[q + 1:q + 17])
            body = new
        out += bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + body
    sel = {s[0]: (s[1], s[2]) for s in fr["scan"]}
    comp_of_block = []
    for c, (h, v) in enumerate(factors):
        comp_of_block += [c] * (h * v)
    bpm = len(comp_of_block)
    codes = {}
    for c, comp in enumerate(fr["components"]):
        td, ta = sel[comp[0]]
        codes[c] = ({s: (code, ln) for s, code, ln in _std_table(0, td)}, {s: (code, ln) for s, code, ln in _std_table(1, ta)})
    w, dri, rst = BitWriter(), fr["dri"], 0
    pred = [0] * len(fr["components"])
    for i, blk in enumerate(blocks):
        mcu, b = divmod(i, bpm)
        if b == 0 and dri and mcu and mcu % dri == 0:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + (rst & 7)])
            rst += 1
            pred = [0] * len(pred)
        c = comp_of_block[b]
        (dcat, dbits), ac = block_symbols(blk, pred[c])
        pred[c] = int(blk[0])
        code, ln = codes[c][0][dcat]
        w.put(code, ln)
        if dcat:
            w.put(dbits, dcat)
        for sym, m, s in ac:
            code, ln = codes[c][1][sym]
            w.put(code, ln)
            if s:
                w.put(m, s)
    w.flush()
    q = scan_at
    while not (d[q] == 0xFF and d[q + 1] != 0 and not 0xD0 <= d[q + 1] <= 0xD7):
        q += 1
    return bytes(out) + bytes(w.out) + bytes(d[q:])


def write_turned(file, o, edge="refuse", from_file=False):
    """F' (see the module's head).  from_file: the orientation is the file's own (policy "file"): its Exif tag is rewritten to 1."""
    fr = frame_of(file)
    pl = plan(fr, o, edge)
    coefs, _ = po.decode_coefficients(bytes(file))
    return assemble(file, pl["width"], pl["height"], pl["factors"], turn_blocks(coefs, fr, o, edge), o >= 5, from_file)


def expected(file, o, edge="refuse", strip=True, most_optimal=False, from_file=False):
    return po.optimize(write_turned(file, o, edge, from_file), strip, most_optimal)
