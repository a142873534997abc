"""The K2 -> K3 coefficient hand-off as half-line planes (a lo plane and a hi plane of 64-byte slots, one flag word per
(chunk of 64 restart intervals, MCU in the interval, block in the MCU); JPGPU_DENSE_HANDOFF=1 keeps every scan dense, =0 splits every scan K3 can read split).

Every case runs both ways and is compared bit for bit with the oracle: the samples, and the coefficients every reader outside K3
still gets as dense int16[blocks][64].  The shapes are the small ones at which the layout can go wrong: an odd count of intervals
and a short last one (padding), a restart interval that does not divide K3's tile (a pair of intervals cut by a tile edge), more
than 64 intervals (several flag words and chunks), more blocks than one tile holds; blocks that end at zig-zag 31, 32 and 63 on
either side of a line; a Batch used again for other content; split and dense scans side by side under every sink; failing scans;
coefficients the caller uploads; the device pointer."""
import ctypes as C

import numpy as np
import pytest

import jpeglibrary_amd as jl
from golden_util import BitWriter, block_symbols, canonical_codes
from jpeglibrary_amd import _capi
from oracle import pyoracle as po
from tools import jpegsynth

pytestmark = pytest.mark.gpu
NAMES = {0: "OK", 1: "InvalidDataException", 2: "InvalidOperationException", 3: "NotSupportedException", 4: "ArgumentException"}


@pytest.fixture(params=["split", "auto", "dense"])
def handoff(request, monkeypatch):
    """dense: the switch; auto: no switch -- the planner splits the scans whose entropy data is at most eight bytes per block, which
    leaves out the Q97 / Q100 / hand-made content here; split: JPGPU_DENSE_HANDOFF=0, every scan K3 has the split form for"""
    if request.param == "auto":
        monkeypatch.delenv("JPGPU_DENSE_HANDOFF", raising=False)
    else:
        monkeypatch.setenv("JPGPU_DENSE_HANDOFF", "1" if request.param == "dense" else "0")
    return request.param


_REF = {}


def _ref(f):
    """(samples, coefficients) of the oracle, computed once per file"""
    if f not in _REF:
        _REF[f] = (po.decode_8bit(f)[0], po.decode_coefficients(f)[0])
    return _REF[f]


def _store_blocks(b):
    total = C.c_uint64()
    assert _capi.lib.jpgpu_batch_coefficients_device(b._h, C.byref(total))
    return total.value


def _padded_blocks(info):
    """the blocks of a split scan's region: an even count of whole restart intervals"""
    per_interval = info.restart_interval * info.blocks_per_mcu
    intervals = -(-info.total_blocks // per_interval)
    return -(-intervals // 2) * 2 * per_interval


def _assert_handed_over(b, handoff, split=None):
    """Pins which layout the batch really has: the coefficient store counts the padding of the split scans (`split`: the images the
    split leg splits, default all) and nothing else.  Where a scan is a whole even count of intervals the two counts are equal; every
    test here has an image whose counts differ.  (The auto leg follows the planner's content rule and is not pinned.)"""
    infos = [b.image_info(i) for i in range(len(b))]
    if handoff == "dense":
        assert _store_blocks(b) == sum(inf.total_blocks for inf in infos)
    elif handoff == "split":
        want = sum(_padded_blocks(inf) if split is None or i in split else inf.total_blocks for i, inf in enumerate(infos))
        assert want > sum(inf.total_blocks for inf in infos)  # (the test's shapes do tell the layouts apart)
        assert _store_blocks(b) == want


# (width, height, subsampling, DRI): MCUs -> intervals.  (Widths are whole MCUs: the bytewise generic output layout of other widths
# keeps its scans dense.)
SMALL = [
    (48, 32, "420", 1),     # 6 MCUs, 6 intervals: three whole lines per block step
    (64, 48, "422", 2),     # 24 MCUs, 12 intervals
    (72, 40, "444", 3),     # 45 MCUs, 15 intervals: an odd count (the last line has one half)
    (80, 56, "gray", 4),    # 70 MCUs, 18 intervals, the last one short (2 MCUs)
    (112, 72, "420", 5),    # 35 MCUs, 7 intervals: odd
    (128, 96, "420", 7),    # 48 MCUs, 7 intervals: odd, the last (even-numbered, no partner) short
    (208, 120, "444", 1),   # 390 intervals: seven flag chunks; 1 170 blocks: five tiles in one workgroup's run
    (208, 120, "gray", 2),  # 195 intervals: odd, four chunks, the last of three intervals
    (208, 120, "420", 5),   # 104 MCUs in tiles of 40 / 42: a pair of intervals cut by a tile edge
    (208, 120, "420", 7),   # ... and with the other DRI that divides no tile; 15 intervals, the last short
    (208, 120, "422", 4),   # 13 x 15 = 195 MCUs, 49 intervals (odd), last short; DRI = 4 as the headline has it
]


@pytest.mark.parametrize("w,h,sub,dri", SMALL, ids=lambda v: str(v))
def test_small_images_pixels_and_coefficients(w, h, sub, dri, handoff):
    files = [bytes(jpegsynth.encode(w, h, sub, q, dri, seed=s)) for q, s in ((75, 11), (97, 12))]
    b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8).decode().sync()
    if (w, h, sub, dri) not in ((48, 32, "420", 1), (64, 48, "422", 2), (208, 120, "444", 1)):  # (a whole even count of intervals: no padding to tell by)
        _assert_handed_over(b, handoff)
    for i, f in enumerate(files):
        px, coefs = _ref(f)
        assert (b.result(i).status, b.result(i).detail) == (0, 0), i
        assert np.array_equal(b.output(i), px), (i, int((b.output(i) != px).sum()))
        assert np.array_equal(b.coefficients(i), coefs), i
    b.close()


# ---- hand-made blocks: where the flag bit turns

def _write_gray(w, h, dri, blocks):
    """a baseline gray file (quantisation table of ones) whose blocks, in scan order, are `blocks` (int16[n][64], zig-zag)"""
    n = ((w + 7) // 8) * ((h + 7) // 8)
    assert len(blocks) == n
    freq, syms, pred = [{}, {}], [], 0
    for i, blk in enumerate(blocks):
        if dri and i % dri == 0:
            pred = 0
        (dcat, dbits), ac = block_symbols(blk, pred)
        pred = int(blk[0])
        freq[0][dcat] = 1
        for sym, _, _ in ac:
            freq[1][sym] = 1
        syms.append((dcat, dbits, ac))
    tabs = [canonical_codes({s: (4 if t == 0 else 8) for s in sorted(freq[t])}) for t in range(2)]
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xdb\x00\x43\x00" + bytes([1] * 64)
    out += b"\xff\xc0\x00\x0b\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + b"\x01\x01\x11\x00"
    for t, tab in enumerate(tabs):
        payload = bytes([t << 4]) + bytes(tab[1]) + bytes(tab[2])
        out += b"\xff\xc4" + (len(payload) + 2).to_bytes(2, "big") + payload
    if dri:
        out += b"\xff\xdd\x00\x04" + dri.to_bytes(2, "big")
    out += b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    bw = BitWriter()
    for i, (dcat, dbits, ac) in enumerate(syms):
        if dri and i and i % dri == 0:
            bw.flush()
            bw.out += bytes([0xFF, 0xD0 + ((i // dri - 1) & 7)])
        bw.put(*tabs[0][0][dcat])
        if dcat:
            bw.put(dbits, dcat)
        for sym, m, s in ac:
            bw.put(*tabs[1][0][sym])
            if s:
                bw.put(m, s)
    bw.flush()
    return bytes(out) + bytes(bw.out) + b"\xff\xd9"


def _block_ending_at(last, rng):
    """a block whose last non-zero coefficient sits at zig-zag `last` (0: the DC alone)"""
    blk = np.zeros(64, np.int16)
    blk[0] = rng.integers(-60, 60)
    for k in rng.choice(np.arange(1, max(last, 2)), size=min(5, max(last - 1, 1)), replace=False):
        if k < last:
            blk[k] = rng.integers(1, 6) * rng.choice([-1, 1])
    if last:
        blk[last] = rng.choice([-2, -1, 1, 3])
    return blk


def _boundary_file(kinds, w=96, h=64, dri=2):
    """kinds[k % len(kinds)] = the zig-zag index block k ends at"""
    rng = np.random.default_rng(5)
    n = (w // 8) * (h // 8)
    blocks = np.stack([_block_ending_at(kinds[k % len(kinds)], rng) for k in range(n)])
    return _write_gray(w, h, dri, blocks), blocks


def _flagged_pairs(blocks, dri):
    """{(flag of the even interval's block, flag of the odd interval's block)} over the lines of the hi plane"""
    seen = set()
    n_int = (len(blocks) + dri - 1) // dri
    flag = lambda i, m: bool(blocks[i * dri + m][32:].any()) if i < n_int and i * dri + m < len(blocks) else False
    for i in range(0, n_int, 2):
        for m in range(dri):
            seen.add((flag(i, m), flag(i + 1, m)))
    return seen


@pytest.mark.parametrize("name,kinds,pairs", [
    # DRI = 2: block k is MCU k & 1 of interval k >> 1, and shares its line with block k +- 2
    ("ends_31_32_63", [31, 32, 63, 0, 32, 31, 63, 31, 31, 32], {(True, False), (False, True), (True, True), (False, False)}),
    ("flagged_then_unflagged", [63, 32, 31, 0], {(True, False)}),
    ("unflagged_then_flagged", [31, 0, 32, 63], {(False, True)}),
    ("all_unflagged", [31, 0, 17], {(False, False)}),
    ("all_flagged", [32, 63, 40], {(True, True)}),
])
def test_flag_boundary_hand_made_blocks(name, kinds, pairs, handoff):
    f, blocks = _boundary_file(kinds)
    assert _flagged_pairs(blocks, 2) == pairs  # (the file holds the pairs it is named for)
    px, coefs = _ref(f)
    assert np.array_equal(coefs, blocks)  # (the oracle reads what the writer above meant)
    b = jl.Batch().upload([f], jl.FMT_INTERLEAVED_U8).decode().sync()
    assert (b.result(0).status, b.result(0).detail) == (0, 0)
    assert np.array_equal(b.output(0), px), int((b.output(0) != px).sum())
    assert np.array_equal(b.coefficients(0), blocks)
    b.close()


def test_flat_and_q100_noise_images(handoff):
    """no block of the flat image is flagged, (nearly) every block of the noise at Q100 is"""
    flat = _write_gray(96, 64, 3, np.tile(np.eye(1, 64, 0, dtype=np.int16) * 40, (96, 1)))
    noise = bytes(jpegsynth.encode(96, 64, "420", 100, 3, seed=21))
    assert (po.decode_coefficients(noise)[0][:, 32:] != 0).any(axis=1).mean() > 0.9
    b = jl.Batch().upload([flat, noise], jl.FMT_INTERLEAVED_U8).decode().sync()
    for i, f in enumerate((flat, noise)):
        px, coefs = _ref(f)
        assert b.result(i).status == 0
        assert np.array_equal(b.output(i), px), i
        assert np.array_equal(b.coefficients(i), coefs), i
    b.close()


def test_no_hi_data_or_flags_of_an_earlier_upload_leak(handoff):
    """one Batch: a flagged image, then an unflagged one of the same shape in the same buffers, decoded twice in a row"""
    flagged, _ = _boundary_file([63, 32, 40])
    unflagged, _ = _boundary_file([31, 0, 9])
    b = jl.Batch()
    for f in (flagged, unflagged):
        b.upload([f], jl.FMT_INTERLEAVED_U8).decode().sync()
        px, coefs = _ref(f)
        assert np.array_equal(b.output(0), px)
        assert np.array_equal(b.coefficients(0), coefs)
    px, coefs = _ref(unflagged)
    b.decode()
    b.decode().sync()
    assert b.result(0).status == 0
    assert np.array_equal(b.output(0), px)
    assert np.array_equal(b.coefficients(0), coefs)
    # ... and the flagged one again behind it: hi lines that were skipped a moment ago are written and read
    b.upload([flagged], jl.FMT_INTERLEAVED_U8).decode().decode().sync()
    assert np.array_equal(b.output(0), _ref(flagged)[0])
    assert np.array_equal(b.coefficients(0), _ref(flagged)[1])
    b.close()


# ---- every sink over split and dense scans side by side

def _header(f):
    """({component index: quantisation table (zig-zag)}, [(h, v)], width, height) of a file's DQT / SOF segments"""
    p, qt, comps = 2, {}, None
    while f[p + 1] != 0xDA:
        n = (f[p + 2] << 8) | f[p + 3]
        seg = f[p + 4:p + 2 + n]
        if f[p + 1] == 0xDB:
            k = 0
            while k < len(seg):
                wide, tq = seg[k] >> 4, seg[k] & 15
                qt[tq] = np.frombuffer(seg[k + 1:k + 1 + 64 * (1 + wide)], dtype=">u2" if wide else np.uint8).astype(np.uint16)
                k += 1 + 64 * (1 + wide)
        elif f[p + 1] in (0xC0, 0xC1, 0xC2):
            height, width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [(seg[6 + 3 * c + 1] >> 4, seg[6 + 3 * c + 1] & 15, seg[6 + 3 * c + 2]) for c in range(seg[5])]
        p += 2 + n
    return {c: qt[tq] for c, (_, _, tq) in enumerate(comps)}, [(h, v) for h, v, _ in comps], width, height


def _ref_planes(f, kind):
    """int16 planes at each component's own resolution, padded to whole MCUs, from the oracle's coefficients and its transform"""
    qt, samp, w, h = _header(f)
    max_h, max_v = max(s[0] for s in samp), max(s[1] for s in samp)
    mpl, mpc = -(-w // (8 * max_h)), -(-h // (8 * max_v))
    planes = [np.zeros((mpc * v * 8, mpl * hh * 8), np.int16) for hh, v in samp]
    put = lambda c, by, bx, z: planes[c].__setitem__((slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8)),
                                                     po.block_dequant_idct_shift(z, qt[c], 128).reshape(8, 8))
    if kind == "progressive":
        _, blocks, _ = po.decode_progressive_store(f)
        for c, grid in blocks.items():
            for (bx, by), z in grid.items():
                if by * 8 < planes[c].shape[0] and bx * 8 < planes[c].shape[1]:
                    put(c, by, bx, z)
        return planes
    coefs, comp = po.decode_coefficients(f)
    if kind == "noninterleaved":  # 4:4:4, a scan per component: its blocks line by line
        k = 0
        for c in range(len(samp)):
            for by in range(-(-h // 8)):
                for bx in range(-(-w // 8)):
                    assert comp[k] == c
                    put(c, by, bx, coefs[k])
                    k += 1
        assert k == len(coefs)
        return planes
    k = 0
    for my in range(mpc):
        for mx in range(mpl):
            for c, (hh, v) in enumerate(samp):
                for y in range(v):
                    for x in range(hh):
                        assert comp[k] == c
                        put(c, my * v + y, mx * hh + x, coefs[k])
                        k += 1
    assert k == len(coefs)
    return planes


@pytest.fixture(scope="module")
def mixed():
    files = [(bytes(jpegsynth.encode(112, 80, "420", 85, 4, seed=31)), "baseline"),             # split
             (bytes(jpegsynth.encode(96, 64, "420", 80, 0, seed=32)), "baseline"),              # DRI = 0: dense
             (bytes(jpegsynth.encode(96, 64, "420", 80, 0, seed=33, progressive=True)), "progressive"),
             (bytes(jpegsynth.encode(80, 48, "444", 90, 7, seed=34, noninterleaved=True)), "noninterleaved"),  # three scans: dense
             (bytes(jpegsynth.encode(112, 56, "422", 92, 2, seed=35)), "baseline"),            # split, another layout class
             (bytes(jpegsynth.encode(72, 40, "444", 88, 3, seed=36)), "baseline"),              # split: the 4:4:4 class (15 intervals)
             (bytes(jpegsynth.encode(80, 56, "gray", 88, 4, seed=37)), "baseline")]             # split: the gray class (last interval short)
    return [(f, po.decode_8bit(f)[0], _ref_planes(f, kind)) for f, kind in files]


# the images of `mixed` K3 has a split form for, by sink (kernels.h: idct_split_supported): 0 is 4:2:0, 4 is 4:2:2, 5 is 4:4:4, 6 is gray
MIXED_SPLIT = {"INTERLEAVED_U8": {0, 4, 5, 6}, "PLANAR_U8": {0, 4, 5, 6}, "PLANAR_I16": {0, 4, 5, 6}, "RGB_U8": {5, 6}, "RGBA_U8": {4, 5, 6},
               "INTERLEAVED_U8_SCALED": {0, 4, 5}}


@pytest.mark.parametrize("fmt", ["INTERLEAVED_U8", "PLANAR_U8", "PLANAR_I16", "RGB_U8", "RGBA_U8", "INTERLEAVED_U8_SCALED"])
def test_mixed_batch_under_every_sink(fmt, mixed, handoff):
    b = jl.Batch().upload([f for f, _, _ in mixed], getattr(jl, "FMT_" + fmt)).decode().sync()
    _assert_handed_over(b, handoff, MIXED_SPLIT[fmt])
    for i, (f, px, planes) in enumerate(mixed):
        assert b.result(i).status == 0, (i, b.result(i).status, b.result(i).detail)
        got = b.output(i)
        if fmt in ("INTERLEAVED_U8", "INTERLEAVED_U8_SCALED"):  # (8-bit frames: the scaled sink's byte is the sample's clamp)
            assert np.array_equal(got, px), (i, int((got != px).sum()))
        elif fmt in ("RGB_U8", "RGBA_U8"):
            assert np.array_equal(got, po.ycbcr8_to_rgb(px, rgba=fmt == "RGBA_U8", gray=px.shape[2] == 1)), i
        else:
            for c, want in enumerate(planes):
                want = want if fmt == "PLANAR_I16" else np.clip(want, 0, 255).astype(np.uint8)
                assert got[c].shape[0] <= want.shape[0] and got[c].shape[1] <= want.shape[1], (i, c, got[c].shape, want.shape)
                assert np.array_equal(got[c], want[:got[c].shape[0], :got[c].shape[1]]), (i, c)
    b.close()


# ---- failing scans

def _truncated(f):
    return f[:len(f) * 11 // 20] + b"\xff\xd9"


def _missing_restart(f):
    """the restart marker in the middle of the scan taken out: the reference's restart check throws there"""
    marks = [k for k in range(len(f) - 1) if f[k] == 0xFF and 0xD0 <= f[k + 1] <= 0xD7]
    k = marks[len(marks) // 2]
    return f[:k] + f[k + 2:]


@pytest.mark.parametrize("w,h,sub,dri", [(208, 104, "420", 4), (120, 88, "444", 5)], ids=lambda v: str(v))  # 23 and 33 intervals
def test_failing_scans_and_the_scan_behind_them(w, h, sub, dri, handoff):
    """Against the reference: the exception's kind (the oracle reports a kind and a message, no detail code) and what the writer holds, as
    the existing corruption tests compare them (test_failing_writer_gpu.py).  Detail and failing interval are compared between the two
    layouts in the test below; the dense layout's are what those existing tests tie to the reference."""
    good = bytes(jpegsynth.encode(w, h, sub, 85, dri, seed=41))
    files = [_truncated(good), _missing_restart(good), good]
    b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8).decode().sync()
    _assert_handed_over(b, handoff)
    for i, f in enumerate(files):
        px, _, err = po.decode_8bit_partial(f)
        assert (err is not None) == (i < 2), i  # (the two damaged files do fail in the reference)
        res = b.result(i)
        assert NAMES.get(res.status) == ("OK" if err is None else err.kind), (i, res.status, res.detail)
        got = b.output(i)
        assert np.array_equal(got, px), (i, int((got != px).sum()))
    assert np.array_equal(b.coefficients(2), _ref(good)[1])
    b.close()


def test_failing_scans_report_the_same_either_way(monkeypatch):
    good = bytes(jpegsynth.encode(208, 120, "420", 85, 4, seed=41))
    files = [_truncated(good), _missing_restart(good), good]
    seen = []
    for dense in ("0", "1"):
        monkeypatch.setenv("JPGPU_DENSE_HANDOFF", dense)
        b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8).decode().sync()
        seen.append([(b.result(i).status, b.result(i).detail, b.result(i).error_interval) for i in range(3)])
        b.close()
    assert seen[0] == seen[1]


# ---- the other readers and writers of the coefficient buffer

def test_coefficients_the_caller_uploads_are_what_run_idct_decodes(handoff):
    fa, fb = (bytes(jpegsynth.encode(128, 96, "420", 80, 5, seed=s)) for s in (51, 52))  # same tables, same shape
    b = jl.Batch().upload([fb, fb], jl.FMT_INTERLEAVED_U8).decode().sync()
    _assert_handed_over(b, handoff)
    assert np.array_equal(b.output(0), _ref(fb)[0])
    b.set_coefficients(0, _ref(fa)[1])  # image 1 keeps what the decode left, in whatever form it was handed over
    b.run_idct().sync()
    assert np.array_equal(b.output(0), _ref(fa)[0])
    assert np.array_equal(b.output(1), _ref(fb)[0])
    assert np.array_equal(b.coefficients(0), _ref(fa)[1])
    assert np.array_equal(b.coefficients(1), _ref(fb)[1])
    b.run_entropy().run_idct().sync()  # the stages on their own agree on the layout, whatever it is by now
    assert np.array_equal(b.output(0), _ref(fb)[0])
    assert np.array_equal(b.coefficients(0), _ref(fb)[1])
    b.upload([fa], jl.FMT_INTERLEAVED_U8).run_entropy().run_idct().sync()  # a new upload: planned afresh
    assert np.array_equal(b.output(0), _ref(fa)[0])
    assert np.array_equal(b.coefficients(0), _ref(fa)[1])
    b.close()


def test_upload_before_any_decode(handoff):
    fa, fb = (bytes(jpegsynth.encode(112, 72, "420", 80, 5, seed=s)) for s in (53, 54))
    b = jl.Batch().upload([fb], jl.FMT_INTERLEAVED_U8)
    b.set_coefficients(0, _ref(fa)[1])
    b.run_idct().sync()
    assert np.array_equal(b.output(0), _ref(fa)[0])
    b.close()


def _hip_memcpy_to_host(ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    for name in (None, "libamdhip64.so.7", "libamdhip64.so"):
        try:
            fn = C.CDLL(name).hipMemcpy
            break
        except (OSError, AttributeError):
            continue
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert fn(out.ctypes.data, ptr, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def test_the_device_pointer_holds_dense_blocks(handoff):
    files = [bytes(jpegsynth.encode(112, 72, "420", 50, 5, seed=61)), bytes(jpegsynth.encode(72, 40, "444", 50, 3, seed=62))]
    b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8).decode().sync()
    total = C.c_uint64()
    ptr = _capi.lib.jpgpu_batch_coefficients_device(b._h, C.byref(total))
    assert ptr
    infos = [b.image_info(i) for i in range(2)]
    # 7 and 15 restart intervals: padded to an even count of whole ones where the scans are split, back to back where they are dense
    padded = sum(-(-(-(-inf.total_blocks // (dri * bpm))) // 2) * 2 * dri * bpm for inf, dri, bpm in zip(infos, (5, 3), (6, 3)))
    assert total.value == (sum(inf.total_blocks for inf in infos) if handoff == "dense" else padded)  # (Q50: under eight bytes a block, split without the switch too)
    for i, f in enumerate(files):
        raw = _hip_memcpy_to_host(ptr + infos[i].coef_offset * 128, infos[i].total_blocks * 128)
        assert np.array_equal(raw.view(np.int16).reshape(-1, 64), _ref(f)[1]), i
    b.close()
