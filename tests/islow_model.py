"""The numpy model of the arithmetic policy "libjpeg" (include/jpgpu.h, "Arithmetic") that the libjpeg tests share: jpeg_idct_islow in integers
that wrap like int32, the assembly of an image's samples from its coefficient blocks, and libjpeg's colour constants.

    islow(coefs, quant)              int16[n, 64] zig-zag coefficients, uint16[64] or [n, 64] zig-zag quantisers -> uint8[n, 8, 8] samples: the
                                     transform in int64, wrapped to int32 in front of each descale, clamp(v + 128, 0, 255)
    asserts_in_range(coefs, quant)   the same samples, asserting on the way that every dequantised coefficient and workspace value fits int16
                                     and every pass sum int32: where libjpeg's C code, its SIMD code and the wrapped model are one function
    tables(f), frame(f), scans(f)    what the assembly needs of a file's headers
    samples(f)                       the image as INTERLEAVED_U8 holds it, uint8[H, W, C], every block through islow(): a baseline file from
                                     pyoracle.decode_coefficients (MCU order, scan by scan), a progressive one from decode_progressive_store;
                                     sub-sampled components are replicated like the reference replicates them
    samples_from_blocks(f, blocks)   the same from a caller's int16[n, 64] in the order of Batch.coefficients (baseline files)
    ycc_rgb(s) / rgb(kind, s)        libjpeg's constants {91881, -46802, 116130, -22554} over uint8[H, W, 3], and color_model's kinds with them
    decode(f, upsampling, kind)      samples -> upsample_model.filtered where the policy filters -> rgb: uint8[H, W, 3], what
                                     decode_to_tensors(arithmetic="libjpeg") delivers (as color_model.as_format turns it)
    pillow_rgb(f) / pillow_l(f)      Pillow's decode of the file, or None without Pillow

Only numpy, Pillow and the sibling models are imported at module level."""
import io
import struct

import numpy as np

import upsample_model as um

CONST_BITS, PASS1_BITS = 13, 2
FACTORS = (91881, -46802, 116130, -22554)  # cr_r, cr_g, cb_b, cb_g
# natural position of zig-zag index k
NAT_OF_ZIG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def wrap32(x):
    """int64 -> the int32 with the same low 32 bits, as int64"""
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _pass(d, shift, check):
    """the 1-D pass along axis 1 of int64[n, 8, m]: d[:, k] is input k -> the eight descaled outputs, same shape"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[:, k] for k in range(8))
    z1 = (d2 + d6) * 4433
    e2 = z1 - d6 * 15137
    e3 = z1 + d2 * 6270
    e0 = (d0 + d4) << CONST_BITS
    e1 = (d0 - d4) << CONST_BITS
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    t0, t1, t2, t3 = d7, d5, d3, d1
    z1 = t0 + t3
    z2 = t1 + t2
    z3 = t0 + t2
    z4 = t1 + t3
    z5 = (z3 + z4) * 9633
    t0 = t0 * 2446
    t1 = t1 * 16819
    t2 = t2 * 25172
    t3 = t3 * 12299
    z1 = z1 * -7373
    z2 = z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    t0 = t0 + z1 + z3
    t1 = t1 + z2 + z4
    t2 = t2 + z2 + z3
    t3 = t3 + z1 + z4
    sums = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    if check:
        for v in sums + [z5, e2, e3, t0, t1, t2, t3]:
            assert np.abs(v).max(initial=0) + (1 << (shift - 1)) < (1 << 31), "a pass sum leaves int32"
    return np.stack([wrap32(wrap32(s) + (1 << (shift - 1))) >> shift for s in sums], axis=1)


def _islow(coefs, quant, check):
    coefs = np.asarray(coefs, dtype=np.int16).reshape(-1, 64).astype(np.int64)
    quant = np.broadcast_to(np.asarray(quant).astype(np.int64).reshape(-1, 64), coefs.shape)
    d = np.zeros(coefs.shape, np.int64)
    d[:, NAT_OF_ZIG] = coefs * quant  # int16 x uint16: inside int32
    if check:
        assert np.abs(d).max(initial=0) < (1 << 15), "a dequantised coefficient leaves int16"
    d = d.reshape(-1, 8, 8)                                    # [n, row, column]
    ws = _pass(d, CONST_BITS - PASS1_BITS, check)              # columns: the pass runs along the rows' axis
    if check:
        assert np.abs(ws).max(initial=0) < (1 << 15), "a workspace value leaves int16"
    out = _pass(ws.transpose(0, 2, 1), CONST_BITS + PASS1_BITS + 3, check).transpose(0, 2, 1)  # rows
    return np.clip(wrap32(out + 128), 0, 255).astype(np.uint8)


def islow(coefs, quant):
    return _islow(coefs, quant, False)


def asserts_in_range(coefs, quant):
    return _islow(coefs, quant, True)


# ------------------------------------------------------------------------------------------------ headers

def _segments(f):
    """(marker, payload offset, payload length) of every segment up to and including the first SOS, and of every later DQT / SOS"""
    pos, out = 2, []
    while pos + 4 <= len(f):
        if f[pos] != 0xFF:
            pos += 1
            continue
        m = f[pos + 1]
        if m == 0xFF or m == 0x00 or 0xD0 <= m <= 0xD7 or m == 0x01:
            pos += 1 if m == 0xFF else 2
            continue
        if m == 0xD9:
            break
        n = struct.unpack(">H", f[pos + 2:pos + 4])[0]
        out.append((m, pos + 4, n - 2))
        pos += 2 + n
    return out


def tables(f):
    """{identifier: uint16[64] zig-zag} of the DQT segments in front of the first SOS"""
    q = {}
    for m, at, n in _segments(f):
        if m == 0xDA:
            break
        if m != 0xDB:
            continue
        p = at
        while p < at + n:
            pq, tq = f[p] >> 4, f[p] & 15
            if pq:
                q[tq] = np.array(struct.unpack(">64H", f[p + 1:p + 129]), np.uint16)
                p += 129
            else:
                q[tq] = np.frombuffer(f[p + 1:p + 65], np.uint8).astype(np.uint16)
                p += 65
    return q


def frame(f):
    """(W, H, progressive, [(id, h, v, tq)])"""
    a = um.sof(f)
    H, W, n = struct.unpack(">H", f[a + 5:a + 7])[0], struct.unpack(">H", f[a + 7:a + 9])[0], f[a + 9]
    comps = [(f[a + 10 + 3 * c], f[a + 11 + 3 * c] >> 4, f[a + 11 + 3 * c] & 15, f[a + 12 + 3 * c]) for c in range(n)]
    return W, H, f[a + 1] == 0xC2, comps


def scans(f):
    """the frame component indices of every SOS, in file order"""
    ids = [c[0] for c in frame(f)[3]]
    return [[ids.index(f[at + 1 + 2 * k]) for k in range(f[at])] for m, at, n in _segments(f) if m == 0xDA]


def _canvas(f):
    W, H, progressive, comps = frame(f)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return W, H, comps, hmax, vmax, mx, my, np.zeros((my * vmax * 8 + 32, mx * hmax * 8 + 32, len(comps)), np.uint8)


def _place(canvas, c, x, y, block, hs, vs):
    rep = np.repeat(np.repeat(block, vs, axis=0), hs, axis=1)
    canvas[y:y + 8 * vs, x:x + 8 * hs, c] = rep[:canvas.shape[0] - y, :canvas.shape[1] - x]


def samples_from_blocks(f, blocks, transform=islow):
    """a baseline file: the blocks of its scans back to back, each scan over the frame's MCU grid with h x v blocks per scan component"""
    W, H, comps, hmax, vmax, mx, my, canvas = _canvas(f)
    q = tables(f)
    blocks = np.asarray(blocks).reshape(-1, 64)
    order = []  # (component, x, y) of every block
    for sc in scans(f):
        for m in range(mx * my):
            for c in sc:
                _, h, v, _ = comps[c]
                order += [(c, ((m % mx) * hmax + bx) * 8, ((m // mx) * vmax + by) * 8) for by in range(v) for bx in range(h)]
    assert len(order) == len(blocks), (len(order), len(blocks))
    px = transform(blocks, np.stack([q[comps[c][3]] for c, _, _ in order]))
    for (c, x, y), b in zip(order, px):
        _place(canvas, c, x, y, b, hmax // comps[c][1], vmax // comps[c][2])
    return np.ascontiguousarray(canvas[:H, :W])


def samples(f, transform=islow):
    from oracle import pyoracle

    W, H, progressive, comps = frame(f)
    if not progressive:
        return samples_from_blocks(f, pyoracle.decode_coefficients(f)[0], transform)
    _, _, _, hmax, vmax, _, _, canvas = _canvas(f)
    _, store, quant = pyoracle.decode_progressive_store(f)
    for c, blocks in store.items():
        hs, vs = hmax // comps[c][1], vmax // comps[c][2]
        keys = [k for k in blocks if k[0] * hs * 8 < canvas.shape[1] - 32 and k[1] * vs * 8 < canvas.shape[0] - 32]
        px = transform(np.stack([blocks[k] for k in keys]), quant[c])
        for (bx, by), b in zip(keys, px):
            _place(canvas, c, bx * hs * 8, by * vs * 8, b, hs, vs)  # (JpegBlockAllocator.Flush's placement)
    return np.ascontiguousarray(canvas[:H, :W])


# ------------------------------------------------------------------------------------------------ colour

def ycc_rgb(s):
    s = np.asarray(s).astype(np.int64)
    y, cb, cr = s[..., 0], s[..., 1] - 128, s[..., 2] - 128
    cr_r, cr_g, cb_b, cb_g = FACTORS
    r = y + ((cr_r * cr + 32768) >> 16)
    g = y + ((cb_g * cb + 32768 + cr_g * cr) >> 16)
    b = y + ((cb_b * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def rgb(kind, s):
    """color_model.model with libjpeg's constants in its YCbCr steps"""
    import color_model as cm

    s = np.ascontiguousarray(s, dtype=np.uint8)
    if kind == "gray":
        return np.repeat(s.reshape(s.shape[0], s.shape[1], 1), 3, axis=2)
    if kind == "ycbcr":
        return ycc_rgb(s)
    if kind == "ycck":
        return cm.d((255 - ycc_rgb(s[..., :3]).astype(np.uint32)) * s[..., 3:4].astype(np.uint32)).astype(np.uint8)
    return cm.model(kind, s)  # (rgb, cmyk: no YCbCr step)


def ratio(f):
    return um.ratio(f) if len(frame(f)[3]) == 3 else None


def decode(f, upsampling="replicate", kind=None, transform=islow):
    s = samples(f, transform)
    if kind is None:
        kind = "gray" if s.shape[2] == 1 else "ycbcr"
    if upsampling == "fancy" and kind == "ycbcr" and um.qualifies(f):
        s = um.filtered(s, *um.ratio(f))
    return rgb(kind, s)


def pillow_rgb(f, mode="RGB"):
    try:
        from PIL import Image
    except ImportError:
        return None
    return np.asarray(Image.open(io.BytesIO(f)).convert(mode))


def pillow_l(f):
    return pillow_rgb(f, "L")
