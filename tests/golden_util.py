"""Reading the reference's golden PNG pairs.

Restates tests/JpegLibrary.Tests/Utils/ImageHelper.cs:12-91 of the reference:
u16[y][x][n] = (HIGH[y][x][n] << 8) | (HIGH[y][x][n] XOR LOWDIFF[y][x][n]) for n < numberOfComponents, 4 ushorts
per pixel (unused channels stay 0).  The PNG pairs under tests/golden/ are data files copied from the reference's
tests/Assets (they are bit-exact dumps of the reference decoder's output made by apps/JpegDebugDump).
"""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name)


def read_jpeg(name) -> bytes:
    with open(golden_path(name), "rb") as f:
        return f.read()


def load_reference_buffer(name, width, height, ncomp) -> np.ndarray:
    """Returns uint16 [H, W, 4] exactly as ImageHelper.LoadBuffer builds it."""
    from PIL import Image

    high = np.asarray(Image.open(golden_path(name + ".high.png")).convert("RGBA"), dtype=np.uint16)
    low = np.asarray(Image.open(golden_path(name + ".low-diff.png")).convert("RGBA"), dtype=np.uint16)
    assert high.shape == (height, width, 4) and low.shape == (height, width, 4), (high.shape, low.shape)
    buf = np.zeros((height, width, 4), dtype=np.uint16)
    buf[..., :ncomp] = (high[..., :ncomp] << 8) | (high[..., :ncomp] ^ low[..., :ncomp])
    return buf


def middle_scan_swallow_files():
    """Multi-scan baseline files (three single-component scans, 96 x 72 4:4:4, with and without restart intervals) with 1-3 bytes
    of fill in front of the second SOS, the third SOS or EOI; a DHT of its own in front of the third scan behind one byte; and
    one byte in front of both middle scans.  One whole byte behind a MIDDLE scan makes the reference's reader resume one byte
    into the marker behind it (JpegHuffmanBaselineScanDecoder.cs:167-176), so which scans exist depends on the decode: the
    batch plans such a file again (DeviceBatch::redo_swallowed).  Returns (files, tags); tag = (dri, fill bytes, where)."""
    from tools import jpegsynth

    files, tags = [], []
    for dri in (0, 4):
        good = bytes(jpegsynth.encode(96, 72, "444", 80, dri, seed=31 + dri, noninterleaved=True))
        sos = [i for i in range(len(good) - 1) if good[i] == 0xFF and good[i + 1] == 0xDA]
        eoi = len(good) - 2
        assert len(sos) == 3
        for k in (1, 2, 3):
            for where, at in (("second_sos", sos[1]), ("third_sos", sos[2]), ("eoi", eoi)):
                files.append(good[:at] + bytes([0x5A] * k) + good[at:])
                tags.append((dri, k, where))
        # a DHT of its own in front of the third scan: the swallowed marker is then the DHT's, the third SOS is found, and the scan
        # decodes with the tables in force before (the same ones here)
        dht = good[good.index(b"\xff\xc4"):]
        dht = dht[:2 + int.from_bytes(dht[2:4], "big")]
        files.append(good[:sos[2]] + b"\x5a" + dht + good[sos[2]:])
        tags.append((dri, 1, "dht_before_third_sos"))
        # both middle scans at once: the re-plan is re-planned
        files.append(good[:sos[1]] + b"\x5a" + good[sos[1]:sos[2]] + b"\x5a" + good[sos[2]:])
        tags.append((dri, 1, "second_and_third_sos"))
    return files, tags


# ---- a tiny baseline entropy coder (Annex C code assignment, F.1.2 symbols, byte stuffing): the tests write files with it

def canonical_codes(lengths):
    """{symbol: length} -> ({symbol: (code, length)}, BITS[16], HUFFVAL) the way Annex C assigns codes"""
    order = sorted(lengths.items(), key=lambda kv: (kv[1], kv[0]))
    bits, codes, code, prev = [0] * 16, {}, 0, order[0][1]
    for sym, ln in order:
        code <<= ln - prev
        prev = ln
        codes[sym] = (code, ln)
        assert code < (1 << ln) - (1 if ln == 16 else 0), "code space exhausted"
        code += 1
        bits[ln - 1] += 1
    return codes, bits, [s for s, _ in order]


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, ln):
        self.acc = (self.acc << ln) | (code & ((1 << ln) - 1))
        self.n += ln
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def block_symbols(block, pred):
    """(DC category, DC bits), [(AC symbol, magnitude bits, size)] of one zig-zag block"""
    def mag(v):
        s = int(abs(v)).bit_length()
        return s, (v if v >= 0 else v + (1 << s) - 1) & ((1 << s) - 1)

    d = int(block[0]) - pred
    out, run = [], 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((0xF0, 0, 0))
            run -= 16
        s, m = mag(v)
        out.append(((run << 4) | s, m, s))
        run = 0
    if run:
        out.append((0x00, 0, 0))
    return mag(d), out
