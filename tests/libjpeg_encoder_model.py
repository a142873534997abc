"""TEST INFRASTRUCTURE ONLY: a numpy restatement of what libjpeg's baseline compressor computes for the encoder's arithmetic policy
"libjpeg" (include/jpgpu.h, section 4d) -- the slow obvious version, written from the contract's seven steps:

  1. quality -> quantisation tables      quant_tables
  2. R,G,B -> Y,Cb,Cr                     rgb_to_ycc
  3. edges and downsampling               component_plane
  4. dummy blocks of an interleaved MCU   quantised_blocks
  5. jpeg_fdct_islow                      fdct_islow (every intermediate an int32; fdct_islow(..., np.int64) is the wide control)
  6. quantisation                         quantise / quantise_mulhi (the device's division-free form)
  7. Annex K Huffman coding and header    encode

encode() returns the whole file, SOI to EOI; quantised_blocks() the zig-zag int16 blocks in encoding order."""
import numpy as np

# Annex K, natural (row-major) order
STD_LUMINANCE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
STD_CHROMINANCE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# zig-zag position -> natural index
NATURAL = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

DC_LUM = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHR = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUM = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHR = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), bytes.fromhex(
    "0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4"
    "c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa".replace(" ", "")))
STD_HUFFMAN = (DC_LUM, AC_LUM, DC_CHR, AC_CHR)  # DC0, AC0, DC1, AC1


def quant_tables(quality):
    """Step 1: (luminance, chrominance), 64 elements each in zig-zag order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    out = []
    for std in (STD_LUMINANCE, STD_CHROMINANCE):
        t = [min(max((v * s + 50) // 100, 1), 255) for v in std]
        out.append(np.array([t[NATURAL[k]] for k in range(64)], np.uint16))
    return out


def rgb_to_ycc(rgb):
    """Step 2, on an (H, W, 3) array: three (H, W) int32 planes."""
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return [y, cb, cr]


def component_plane(plane, h, v, max_h, max_v):
    """Step 3: the component's samples, wb * 8 columns by hb * 8 rows, from its full-size plane."""
    height, width = plane.shape
    wb = -(-(-(-width * h // max_h)) // 8)
    hb = -(-(-(-height * v // max_v)) // 8)
    hs, vs = max_h // h, max_v // v
    p = plane.astype(np.int32)
    p = np.pad(p, ((0, 0), (0, wb * 8 * hs - width)), mode="edge")
    p = np.pad(p, ((0, -height % max_v), (0, 0)), mode="edge")
    cols = np.arange(wb * 8, dtype=np.int32)
    if (hs, vs) == (2, 2):
        bias = 1 + (cols & 1)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias[None, :]) >> 2
    elif (hs, vs) == (2, 1):
        bias = cols & 1
        p = (p[:, 0::2] + p[:, 1::2] + bias[None, :]) >> 1
    elif (hs, vs) != (1, 1):
        raise ValueError("sampling %d x %d" % (hs, vs))
    p = p[:hb * 8]
    return np.pad(p, ((0, hb * 8 - p.shape[0]), (0, 0)), mode="edge"), wb, hb


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


_reached = [0]


def fdct_multiplicand_bound(samples):
    """The largest magnitude a constant of the transform is multiplied with, over both passes of these (..., 8, 8) samples."""
    _reached[0] = 0
    fdct_islow(samples, np.int64)
    return _reached[0]


def _fdct_pass(d, first, dtype):
    """One pass of jpeg_fdct_islow over the LAST axis of d (..., 8)."""
    def c(k):
        return dtype(k)

    def mul(a, k):  # (the device multiplies with 24-bit operands: fdct_multiplicand_bound says what `a` reaches)
        _reached[0] = max(_reached[0], int(np.abs(a).max()))
        return a * c(k)

    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t7 = d0 + d7, d0 - d7
    t1, t6 = d1 + d6, d1 - d6
    t2, t5 = d2 + d5, d2 - d5
    t3, t4 = d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = mul(t12 + t13, 4433)
    o2 = descale(z1 + mul(t13, 6270), n)
    o6 = descale(z1 - mul(t12, 15137), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = mul(z3 + z4, 9633)
    t4, t5, t6, t7 = mul(t4, 2446), mul(t5, 16819), mul(t6, 25172), mul(t7, 12299)
    z1, z2 = mul(z1, -7373), mul(z2, -20995)
    z3, z4 = mul(z3, -16069) + z5, mul(z4, -3196) + z5
    o7 = descale(t4 + z1 + z3, n)
    o5 = descale(t5 + z2 + z4, n)
    o3 = descale(t6 + z2 + z3, n)
    o1 = descale(t7 + z1 + z4, n)
    out = np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=-1)
    assert out.dtype == dtype
    return out


def fdct_islow(samples, dtype=np.int32):
    """Step 5 on (..., 8, 8) samples 0..255: 8 x the DCT, natural order.  Every intermediate has `dtype`."""
    with np.errstate(over="raise"):
        d = samples.astype(dtype) - dtype(128)
        rows = _fdct_pass(d, True, dtype)
        cols = _fdct_pass(np.swapaxes(rows, -1, -2), False, dtype)
        return np.swapaxes(cols, -1, -2)


def quantise(coef, q):
    """Step 6: coef (..., 64) natural order values of the transform, q the 64 divisors in the same order."""
    d = q.astype(np.int64) << 3
    m = (np.abs(coef.astype(np.int64)) + (d >> 1)) // d
    return np.where(coef < 0, -m, m).astype(np.int32)


def mulhi_factor(q):
    """The device's per-divisor constant: floor(2^32 / d) + 1 for d = q << 3."""
    return (1 << 32) // (np.asarray(q, np.uint64) << np.uint64(3)) + np.uint64(1)


def quantise_mulhi(coef, q):
    """Step 6 as the kernel computes it: one multiply-high of |c| + d / 2 by mulhi_factor."""
    d = np.asarray(q, np.uint64) << np.uint64(3)
    n = np.abs(coef.astype(np.int64)).astype(np.uint64) + (d >> np.uint64(1))
    m = ((n * mulhi_factor(q)) >> np.uint64(32)).astype(np.int64)
    return np.where(coef < 0, -m, m).astype(np.int32)


def geometry(width, height, components, luma):
    """(H, V) as planned, MCUs per line and per column, blocks per MCU.  One component: a non-interleaved scan of 1 x 1."""
    max_h, max_v = luma if components == 3 else (1, 1)
    mpl, mpc = -(-width // (8 * max_h)), -(-height // (8 * max_v))
    return max_h, max_v, mpl, mpc, max_h * max_v + (2 if components == 3 else 0)


def quantised_blocks(pixels, luma=(2, 2), quality=75, rgb=True, tables=None):
    """Steps 1 to 6: int16 [total blocks, 64], zig-zag, encoding order.  pixels: (H, W, 3), (H, W, 4) with rgb (alpha stepped over), (H, W)."""
    a = np.asarray(pixels, np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    height, width, c = a.shape
    components = 1 if c == 1 else 3
    qt = quant_tables(quality) if tables is None else [np.asarray(t, np.uint16).reshape(64) for t in tables]
    planes = [a[..., 0].astype(np.int32)] if components == 1 else (rgb_to_ycc(a[..., :3]) if rgb else [a[..., k].astype(np.int32) for k in range(3)])
    max_h, max_v, mpl, mpc, bpm = geometry(width, height, components, luma)
    zig = np.array(NATURAL)
    out = np.zeros((mpl * mpc, bpm, 64), np.int16)
    b0 = 0
    for ci, plane in enumerate(planes):
        h, v = (max_h, max_v) if ci == 0 else (1, 1)
        smp, wb, hb = component_plane(plane, h, v, max_h, max_v)
        q_nat = np.empty(64, np.uint16)
        q_nat[zig] = qt[0 if ci == 0 else 1]
        blocks = smp.reshape(hb, 8, wb, 8).swapaxes(1, 2)
        coef = quantise(fdct_islow(blocks).reshape(hb, wb, 64), q_nat)[..., zig]
        assert np.abs(coef).max() < 32768
        for by in range(mpc * v):
            for bx in range(mpl * h):
                mcu, b = (by // v) * mpl + bx // h, b0 + (by % v) * h + bx % h
                if bx < wb and by < hb:
                    out[mcu, b] = coef[by, bx]
        b0 += h * v
    # step 4: a dummy block (luma only) takes the DC of the block emitted just before it in its MCU
    wb0, hb0 = -(-width // 8), -(-height // 8)
    for mcu in range(mpl * mpc):
        for b in range(1, max_h * max_v if components == 3 else 1):
            bx, by = (mcu % mpl) * max_h + b % max_h, (mcu // mpl) * max_v + b // max_h
            if bx >= wb0 or by >= hb0:
                out[mcu, b] = 0
                out[mcu, b, 0] = out[mcu, b - 1, 0]
    return out.reshape(-1, 64)


# ---------------------------------------------------------------------------------------------- step 7
def huffman_codes(bits, values):
    """{symbol: (code, length)} of a DHT's lists (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[values[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _Bits:
    def __init__(self):
        self.out, self.reg, self.n = bytearray(), 0, 0

    def put(self, value, length):
        self.reg = (self.reg << length) | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.reg >> (self.n - 8)) & 0xFF
            self.n -= 8
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.reg &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(v):
    a = abs(v)
    n = a.bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def _segment(marker, body):
    return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def header(width, height, components, luma, tables, restart_interval=0):
    """SOI .. SOS as libjpeg writes them."""
    max_h, max_v = luma if components == 3 else (1, 1)
    h = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if components == 3 else 1):
        h += _segment(0xDB, bytes([t]) + bytes(int(x) for x in tables[t]))
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([components])
    for c in range(components):
        sof += bytes([c + 1, (max_h << 4 | max_v) if c == 0 else 0x11, 0 if c == 0 else 1])
    h += _segment(0xC0, sof)
    for t in range(4 if components == 3 else 2):
        bits, values = STD_HUFFMAN[t]
        h += _segment(0xC4, bytes([((t & 1) << 4) | (t >> 1)]) + bytes(bits) + bytes(values))
    if restart_interval:
        h += _segment(0xDD, restart_interval.to_bytes(2, "big"))
    sos = bytes([components])
    for c in range(components):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return h + _segment(0xDA, sos + b"\x00\x3f\x00")


def encode(pixels, luma=(2, 2), quality=75, rgb=True, restart_interval=0, tables=None):
    """The whole file."""
    a = np.asarray(pixels, np.uint8)
    height, width = a.shape[:2]
    components = 1 if a.ndim == 2 or a.shape[2] == 1 else 3
    qt = quant_tables(quality) if tables is None else [np.asarray(t, np.uint16).reshape(64) for t in tables]
    blocks = quantised_blocks(a, luma, quality, rgb, qt)
    max_h, max_v, mpl, mpc, bpm = geometry(width, height, components, luma)
    codes = [huffman_codes(*t) for t in STD_HUFFMAN]
    w = _Bits()
    out = bytearray(header(width, height, components, luma, qt, restart_interval))
    pred = [0, 0, 0]
    ny = bpm - (2 if components == 3 else 0)
    for mcu in range(mpl * mpc):
        if restart_interval and mcu and mcu % restart_interval == 0:
            w.flush()
            out += w.out + bytes((0xFF, 0xD0 + (mcu // restart_interval - 1) % 8))
            w = _Bits()
            pred = [0, 0, 0]
        for b in range(bpm):
            comp = 0 if b < ny else b - ny + 1
            dc, ac = codes[0 if comp == 0 else 2], codes[1 if comp == 0 else 3]
            blk = [int(x) for x in blocks[mcu * bpm + b]]
            n, extra = _magnitude(blk[0] - pred[comp])
            pred[comp] = blk[0]
            w.put(*dc[n])
            w.put(extra, n)
            run = 0
            for k in range(1, 64):
                if blk[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    w.put(*ac[0xF0])
                    run -= 16
                n, extra = _magnitude(blk[k])
                w.put(*ac[(run << 4) | n])
                w.put(extra, n)
                run = 0
            if run:
                w.put(*ac[0x00])
    w.flush()
    return bytes(out + w.out + b"\xff\xd9")
