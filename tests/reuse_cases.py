"""The inputs of the reuse suites (test_batch_reuse_gpu.py, test_decoder_reuse_cpu.py): what one upload leaves in a Batch's buffers, and
what the next one must not show of it.  Made at test time from fixed seeds; test_batch_reuse_inputs_cpu.py proves on the oracle alone that
each is what its name says.  Plain Python over Pillow, tools/jpegsynth, progscript and policy_model: nothing here calls the decoder.

LOUD files are what an earlier upload leaves behind: every output sample is at least 16 and every block has a nonzero coefficient in its
last zig-zag position, so stale bytes and stale coefficients are never zero.  The pictures are written in the components' own space
(Pillow's "YCbCr" and "L" modes pass the samples through) at quality 100, whose tables are all ones: 150 + noise of +-12 + the (7, 7)
basis function at amplitude 12 with a random sign per block, which alone puts +-48 into coefficient 63.  Sub-sampled chroma is built at
its own size and repeated, so libjpeg's 2 x 2 average gives it back.  The sizes are whole MCUs (a padded block repeats the picture's last
column: its coefficient 63 is zero) and their output bytes are multiples of 256, so the slots of a loud upload lie back to back.

QUIET files leave a part of their slot unwritten, and are no larger than the loud file whose slot they land in:
    truncated(dri)        a baseline 4:2:0 file cut in the middle of its scan, EOI kept
    missing_last_scan()   three scans, one per component; the last one is not there
    band_1_5()            progressive: the DC scans and the AC band 1..5 only;  band_1_5_cut(): the same, cut inside its second scan
    black_gray()          every block is its DC difference and an end of block
"""
import functools
import io

import numpy as np

import policy_model as pm
import progscript as ps

K2S_MIN_BYTES = 512  # device_batch_layout.cpp, plan_entropy_work: a DRI = 0 scan with fewer bytes from its first entropy byte to the end of the file is one K2 interval
LOUD_FLOOR = 16

_BASIS77 = np.outer(np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16), np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16))


def _loud_plane(rng, h, w):
    assert h % 8 == 0 and w % 8 == 0
    sign = rng.choice([-1.0, 1.0], (h // 8, w // 8))
    p = 150.0 + rng.integers(-12, 13, (h, w)) + 12.0 * np.kron(sign, _BASIS77)
    return np.rint(p).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def loud(w, h, kind, dri=0, seed=0, progressive=False):
    """kind: "420", "444" or "gray"; w x h whole MCUs"""
    from PIL import Image

    rng = np.random.default_rng(seed)
    if kind == "gray":
        img = Image.fromarray(_loud_plane(rng, h, w), "L")
        kw = {}
    else:
        s = 2 if kind == "420" else 1
        assert w % (8 * s) == 0 and h % (8 * s) == 0
        chroma = [np.repeat(np.repeat(_loud_plane(rng, h // s, w // s), s, axis=0), s, axis=1) for _ in range(2)]
        img = Image.fromarray(np.stack([_loud_plane(rng, h, w)] + chroma, axis=2), "YCbCr")
        kw = {"subsampling": 2 if kind == "420" else 0}
    if dri:
        kw["restart_marker_blocks"] = dri
    buf = io.BytesIO()
    img.save(buf, format="JPEG", quality=100, progressive=progressive, **kw)
    return buf.getvalue()


# 21 x 17 MCUs of 4:2:0, 90 restart intervals each: five files from one encoder are ten chunks of 64 intervals, a K2 pool (two chunks make
# one), and single-scan DRI != 0 files are what the split hand-off takes.  336 * 272 * 3 = 1071 * 256 bytes.
def loud_k2(k):
    return loud(336, 272, "420", dri=4, seed=100 + k)


def loud_gray():
    return loud(336, 272, "gray", dri=4, seed=110)  # 357 * 256 bytes, 357 restart intervals: a pool of its own


def loud_k2_upload():
    return [loud_k2(k) for k in range(5)] + [loud_gray()]


# 4:4:4, DRI = 0.  At some fifty bytes a block the smallest loud file above K2S_MIN_BYTES is 16 x 16 (test_batch_reuse_inputs_cpu.py finds
# it); this one is sized for the quiet file that follows it: 324 * 256 bytes, just above the 81 600 of truncated(0).
def loud_k2s(k):
    return loud(192, 144, "444", dri=0, seed=120 + k)


def loud_progressive(k):
    return loud(64, 48, "420", seed=130 + k, progressive=True)  # 36 * 256 bytes


def entropy_start(data):
    """offset of the first entropy-coded byte of the first scan"""
    p = 2
    while True:
        assert data[p] == 0xFF, p
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        if m == 0xDA:
            return p + 2 + n
        p += 2 + n


def _cut(data, fraction, first=None, end=None):
    """the file up to `fraction` of the way through data[first:end] (default: the first scan's entropy bytes), EOI behind it"""
    first = entropy_start(data) if first is None else first
    end = len(data) - 2 if end is None else end
    at = first + int((end - first) * fraction)
    if data[at - 1] == 0xFF:  # (not between an FF and what follows it)
        at += 1
    return bytes(data[:at]) + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def truncated(dri):
    from tools import jpegsynth

    return _cut(bytes(jpegsynth.encode(200, 136, "420", 75, dri, seed=140 + dri)), 0.5)


def _sos_offsets(data):
    out, p = [], 2
    while p < len(data) - 1:
        if data[p] == 0xFF and data[p + 1] == 0xDA:
            out.append(p)
            p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
        elif data[p] == 0xFF and data[p + 1] not in (0, 0xFF) and not 0xD0 <= data[p + 1] <= 0xD9 and not out:
            p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
        else:
            p += 1
    return out


@functools.lru_cache(maxsize=None)
def missing_last_scan():
    from tools import jpegsynth

    # (DRI 4 over 45 MCUs: an interval that divides a scan's MCU count makes the reference expect a marker behind the scan's last MCU)
    data = bytes(jpegsynth.encode(72, 40, "444", 75, 4, seed=160, noninterleaved=True))
    sos = _sos_offsets(data)
    assert len(sos) == 3
    return data[:sos[2]] + b"\xff\xd9"


# (component 0's band last: the reference's Dispose() transforms the components its slots name, and a single-component scan takes slot 0)
BAND_SCRIPT = [ps.S([0, 1, 2], 0, 0, 0, 0), ps.S([1], 1, 5, 0, 0), ps.S([2], 1, 5, 0, 0), ps.S([0], 1, 5, 0, 0)]
assert ps.slots_map_one_to_one(BAND_SCRIPT, 3)
BAND_SIZE = (56, 40)


@functools.lru_cache(maxsize=None)
def _band():
    w, h = BAND_SIZE
    rng = np.random.default_rng(170)
    coefs = ps.recipe_dense(rng, w, h, ps.YCC420, amp=6, dc_amp=300)  # (63 nonzero AC coefficients in every block: 6..63 are there to be left out)
    qtabs = {0: np.full(64, 2, np.uint16), 1: np.full(64, 3, np.uint16)}
    return ps.write(w, h, ps.YCC420, qtabs, coefs, BAND_SCRIPT), coefs


def band_1_5():
    return _band()[0]


@functools.lru_cache(maxsize=None)
def band_store():
    """what the decoder's store holds behind band_1_5(), from the coefficients the file was written from (through no decoder): int16
    [blocks, 64] in the batch's order, coefficients 6..63 zero everywhere"""
    w, h = BAND_SIZE
    out = ps.store_in_mcu_order(ps.expected_store(_band()[1], ps.YCC420, w, h, BAND_SCRIPT), ps.YCC420, w, h)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def band_1_5_cut():
    data = band_1_5()
    sos = _sos_offsets(data)
    assert len(sos) == 4
    first = sos[1] + 2 + int.from_bytes(data[sos[1] + 2:sos[1] + 4], "big")
    end = data.index(b"\xff\xc4", first)  # (the next scan's DHT: "optimal" tables, one in front of every scan)
    return _cut(data, 0.5, first, end)


@functools.lru_cache(maxsize=None)
def black_gray():
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.zeros((48, 72), np.uint8), "L").save(buf, format="JPEG", quality=75)
    return buf.getvalue()


def quiet_upload():
    return [truncated(4), missing_last_scan(), black_gray()]


def band_upload():
    return [band_1_5(), band_1_5_cut()]


def road_files():
    """a file of each road of test_policy_matrix_gpu.ROADS that the files above do not take"""
    return [pm.file(n) for n in ("422", "440", "411", "odd", "cmyk", "adobe_rgb", "422_three_scans", "420_progressive")]


# ------------------------------------------------------------------------------------------------ the JpegDecoder mirror's files

def header_segments(data):
    """[(marker, start, end)] of the segments between SOI and the first SOS"""
    out, p = [], 2
    while data[p + 1] != 0xDA:
        n = int.from_bytes(data[p + 2:p + 4], "big")
        out.append((data[p + 1], p, p + 2 + n))
        p += 2 + n
    return out


def table_payloads(data):
    """the DQT and DHT payloads of the header, in file order"""
    return [bytes(data[a + 4:b]) for m, a, b in header_segments(data) if m in (0xDB, 0xC4)]


def without_tables(data):
    """the abbreviated form of the file: its DQT and DHT segments removed"""
    out, at = bytearray(data[:2]), 2
    for m, a, b in header_segments(data):
        if m not in (0xDB, 0xC4):
            out += data[a:b]
        at = b
    return bytes(out) + bytes(data[at:])


def mirror_a():
    from tools import jpegsynth

    return bytes(jpegsynth.encode(112, 80, "420", 75, 4, seed=180))


def mirror_b():
    """written with mirror_a's tables: the same encoder at the same quality, its standard Huffman tables"""
    from tools import jpegsynth

    return bytes(jpegsynth.encode(72, 56, "420", 75, 4, seed=181))


# ------------------------------------------------------------------------------------------------ what the oracle says of a file

@functools.lru_cache(maxsize=None)
def reference(data):
    """(kind, samples or None, coefficients or None): the oracle's exception class ("OK" for none), its writer's buffer -- None where
    Identify fails --, and its coefficients where a baseline file decodes cleanly; cached, read-only"""
    from oracle import pyoracle as po

    try:
        px, info, err = po.decode_8bit_partial(data)
    except po.OracleError as e:
        return e.kind, None, None
    px.setflags(write=False)
    coefs = None
    if err is None and not is_progressive(data):
        coefs = po.decode_coefficients(data)[0]
        coefs.setflags(write=False)
    return ("OK" if err is None else err.kind), px, coefs


def is_progressive(data):
    import islow_model as im

    return bool(im.frame(data)[2])


@functools.lru_cache(maxsize=None)
def progressive_store(data):
    """int16[blocks, 64] in the batch's order (MCU raster, component order, block raster in the MCU): the oracle's coefficient store of a
    progressive file right before its Dispose(); for frames of whole MCUs, where every block of the MCU grid is a block of the picture"""
    from oracle import pyoracle as po
    import islow_model as im

    W, H, _, comps = im.frame(data)
    _, _, _, _, grids = ps.geometry(W, H, comps)
    assert W % (8 * max(c[1] for c in comps)) == 0 and H % (8 * max(c[2] for c in comps)) == 0
    _, blocks, _ = po.decode_progressive_store(data)
    exp = []
    for ci, (hb, vb) in enumerate(grids):
        assert sorted(blocks[ci]) == sorted((x, y) for y in range(vb) for x in range(hb)), ci
        a = np.zeros((vb, hb, 64), np.int16)
        for (bx, by), v in blocks[ci].items():
            a[by, bx] = v
        exp.append(a)
    out = ps.store_in_mcu_order(exp, comps, W, H)
    out.setflags(write=False)
    return out


def blocks_before_the_error(data):
    """(blocks the oracle's entropy decoder delivered before it threw, the error or None)"""
    from oracle import pyoracle as po

    n = [0]

    def tap(z, ci, bi):
        n[0] += 1

    try:
        po.decode_with_callbacks(data, None, tap)
    except po.OracleError as e:
        return n[0], e
    return n[0], None


def scan_blocks(data):
    """blocks of a single-scan file's MCU grid"""
    import islow_model as im

    W, H, _, comps = im.frame(data)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    return -(-W // (8 * hmax)) * -(-H // (8 * vmax)) * sum(c[1] * c[2] for c in comps)


def output_bytes(data):
    """INTERLEAVED_U8: height * width * components"""
    import islow_model as im

    W, H, _, comps = im.frame(data)
    return W * H * len(comps)
