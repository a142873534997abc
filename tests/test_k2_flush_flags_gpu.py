"""K2's split flush: the step's flag word is one ballot over "my own staged block has a non-zero coefficient in 32..63", and a
pass of sixteen blocks whose bits are all clear neither reads, re-zeroes nor stores its hi side.

Every case runs split (JPGPU_DENSE_HANDOFF=0) and dense (=1) and is compared bit for bit with the oracle: the samples and the
coefficients; on the split leg also the flag words K2 left in the store, against words computed here from the oracle's coefficients
(word ((i >> 6) * DRI + m) * bpm + b, bit i & 63, for block b of MCU m of restart interval i).  Each case first asserts on the CPU that
the oracle's coefficients have their flagged blocks where the case says.

The files are hand-made (quantisation table of ones, as at Q100) so that a case decides block by block what is flagged; a lane of a
K2 wave is a restart interval, a pass of the flush is sixteen lanes.  A single image of at most 64 intervals is one chunk and takes
huffman_decode_kernel; two or more chunks with the same tables are pooled (huffman_pool_kernel): device_batch_layout.cpp."""
import ctypes as C

import numpy as np
import pytest

import jpeglibrary_amd as jl
from golden_util import BitWriter, block_symbols, canonical_codes
from jpeglibrary_amd import _capi
from oracle import pyoracle as po
from tools import jpegsynth

pytestmark = pytest.mark.gpu

_DEBUG = C.CDLL(_capi.LIB_PATH)  # (accessors for tests, not part of the C ABI of include/jpgpu.h)
_FLAGS = _DEBUG.jpgpu_debug_batch_split_flags
_FLAGS.restype = C.c_longlong
_FLAGS.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]


@pytest.fixture(params=["split", "dense"])
def handoff(request, monkeypatch):
    monkeypatch.setenv("JPGPU_DENSE_HANDOFF", "1" if request.param == "dense" else "0")
    return request.param


# ---- the writer: gray or 4:2:0, every restart interval coded on its own

# tables that hold every symbol a block can need, so that files of any content stage the same tables (one pool)
_FULL_DC = {s: 4 for s in range(12)}
_FULL_AC = {(r << 4) | s: 8 for r in range(16) for s in range(1, 11)}
_FULL_AC.update({0x00: 8, 0xF0: 8})
_COMPS = {"gray": [0], "420": [0, 0, 0, 0, 1, 2]}


def _interval_symbols(blocks, comps):
    """[(DC category, DC bits, AC symbols)] of the blocks of one restart interval (the predictors start at zero)"""
    pred, out = [0, 0, 0], []
    for k, blk in enumerate(blocks):
        c = comps[k % len(comps)]
        (dcat, dbits), ac = block_symbols(blk, pred[c])
        pred[c] = int(blk[0])
        out.append((dcat, dbits, ac))
    return out


def _interval_bytes(syms, tabs):
    bw = BitWriter()
    for dcat, dbits, ac in syms:
        bw.put(*tabs[0][0][dcat])
        if dcat:
            bw.put(dbits, dcat)
        for sym, m, s in ac:
            bw.put(*tabs[1][0][sym])
            if s:
                bw.put(m, s)
    bw.flush()
    return bytes(bw.out)


def _write(w, h, sub, dri, intervals, order=None, full_tables=False):
    """A baseline file whose restart intervals are `intervals` (each int16[dri * bpm][64], zig-zag; the last may be short), or
    intervals[order[i]] for interval i.  Tables: the symbols the file uses (4-bit DC, 8-bit AC codes), or the full sets."""
    comps = _COMPS[sub]
    mcu = 8 if sub == "gray" else 16
    n_mcus = -(-w // mcu) * -(-h // mcu)
    order = list(range(len(intervals))) if order is None else order
    assert sum(len(intervals[o]) for o in order) == n_mcus * len(comps) and all(len(intervals[o]) == dri * len(comps) for o in order[:-1])
    syms = [_interval_symbols(iv, comps) for iv in intervals]
    if full_tables:
        tabs = [canonical_codes(_FULL_DC), canonical_codes(_FULL_AC)]
    else:
        used = [{d for sy in syms for d, _, _ in sy}, {a for sy in syms for _, _, ac in sy for a, _, _ in ac} | {0}]
        tabs = [canonical_codes({s: (4 if t == 0 else 8) for s in sorted(used[t])}) for t in range(2)]
    coded = [_interval_bytes(sy, tabs) for sy in syms]
    nc = 1 if sub == "gray" else 3
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xdb\x00\x43\x00" + bytes([1] * 64)
    out += b"\xff\xc0" + (8 + 3 * nc).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc])
    out += b"\x01\x11\x00" if nc == 1 else b"\x01\x22\x00\x02\x11\x00\x03\x11\x00"
    for t, tab in enumerate(tabs):
        payload = bytes([t << 4]) + bytes(tab[1]) + bytes(tab[2])
        out += b"\xff\xc4" + (len(payload) + 2).to_bytes(2, "big") + payload
    out += b"\xff\xdd\x00\x04" + dri.to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * nc).to_bytes(2, "big") + bytes([nc]) + b"".join(bytes([c + 1, 0]) for c in range(nc)) + b"\x00\x3f\x00"
    parts = []
    for i, o in enumerate(order):
        if i:
            parts.append(bytes([0xFF, 0xD0 + ((i - 1) & 7)]))
        parts.append(coded[o])
    return bytes(out) + b"".join(parts) + b"\xff\xd9"


def _clean(rng, last=31):
    """an unflagged block: a few coefficients, the last non-zero one at zig-zag `last` (0: the DC alone), then EOB"""
    blk = np.zeros(64, np.int16)
    blk[0] = rng.integers(-60, 60)
    if last:
        for k in rng.choice(np.arange(1, last + 1), size=min(4, last), replace=False):
            blk[k] = rng.integers(1, 6) * rng.choice([-1, 1])
        blk[last] = rng.choice([-2, -1, 1, 3])
    return blk


def _only(at, dc=7):
    blk = np.zeros(64, np.int16)
    blk[0], blk[at] = dc, -3
    return blk


def _file(w, h, sub, dri, special, seed=1, last=31):
    """every block unflagged (its last non-zero coefficient at `last`) except special = {block index in scan order: block}"""
    rng = np.random.default_rng(seed)
    bpm = len(_COMPS[sub])
    mcu = 8 if sub == "gray" else 16
    n = -(-w // mcu) * -(-h // mcu) * bpm
    blocks = np.stack([special[k] if k in special else _clean(rng, last) for k in range(n)])
    per = dri * bpm
    return _write(w, h, sub, dri, [blocks[a:a + per] for a in range(0, n, per)]), blocks


# ---- the checks

def _expected_words(coefs, dri, bpm):
    n_int = -(-(len(coefs) // bpm) // dri)
    words = np.zeros(-(-n_int // 64) * dri * bpm, np.uint64)
    k = np.flatnonzero((coefs[:, 32:] != 0).any(axis=1))
    i, m = np.divmod(k // bpm, dri)
    np.bitwise_or.at(words, ((i >> 6) * dri + m) * bpm + k % bpm, np.uint64(1) << (i & 63).astype(np.uint64))
    return words


def _flag_words(b, i, n):
    got = np.zeros(n, np.uint64)
    assert _FLAGS(b._h, i, got.ctypes.data, n) == n
    return got


_REF = {}


def _ref(f):
    if f not in _REF:
        _REF[f] = (po.decode_8bit(f)[0], po.decode_coefficients(f)[0])
    return _REF[f]


def _check(files, handoff, dri, bpm, flagged=None):
    """flagged: per file, the set of block indices the case means to be flagged (None: not pinned)"""
    for k, f in enumerate(files):
        if flagged is not None and flagged[k] is not None:
            assert set(np.flatnonzero((_ref(f)[1][:, 32:] != 0).any(axis=1)).tolist()) == set(flagged[k]), k
    b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8).decode().sync()
    for i, f in enumerate(files):
        px, coefs = _ref(f)
        assert (b.result(i).status, b.result(i).detail) == (0, 0), i
        if handoff == "split":
            want = _expected_words(coefs, dri, bpm)
            got = _flag_words(b, i, len(want))
            assert np.array_equal(got, want), (i, [(int(j), hex(int(got[j])), hex(int(want[j]))) for j in np.flatnonzero(got != want)[:8]])
        else:
            assert _FLAGS(b._h, i, np.zeros(1, np.uint64).ctypes.data, 1) == -1  # (this leg really is dense)
        assert np.array_equal(b.output(i), px), (i, int((b.output(i) != px).sum()))
        assert np.array_equal(b.coefficients(i), coefs), i
    stats = b.plan_stats()
    b.close()
    return stats


# ---- one chunk of 64 intervals

@pytest.mark.parametrize("sub", ["gray", "420"])
@pytest.mark.parametrize("flush_pass", [0, 1, 2, 3])
def test_one_flagged_block_in_one_pass(flush_pass, sub, handoff):
    """64 intervals; exactly one block is flagged, staged by a lane of pass `flush_pass`: that pass alone runs its hi side"""
    if sub == "gray":  # 16 x 8 blocks, DRI = 2: block k is MCU k & 1 of interval k >> 1
        shape, dri, bpm, k = (128, 64), 2, 1, (16 * flush_pass + 5) * 2 + 1
    else:              # 8 x 8 MCUs, DRI = 1: block k is block k % 6 of interval k // 6
        shape, dri, bpm, k = (128, 128), 1, 6, (16 * flush_pass + 10) * 6 + 4
    f, blocks = _file(*shape, sub, dri, {k: _only(47)}, seed=flush_pass)
    assert np.array_equal(_ref(f)[1], blocks)  # (the oracle reads what the writer meant)
    _check([f], handoff, dri, bpm, [{k}])


@pytest.mark.parametrize("which", ["even", "odd"])
def test_a_flagged_block_beside_a_clean_partner(which, handoff):
    """intervals 6 and 7 share a line of each plane; one of them is flagged at MCU 1, the other's hi slot comes back as zeros"""
    k = (6 + (which == "odd")) * 2 + 1
    f, blocks = _file(128, 64, "gray", 2, {k: _only(40), k ^ 2: _clean(np.random.default_rng(9), 31)})
    assert not blocks[k ^ 2][32:].any() and blocks[k ^ 2][31] != 0
    _check([f], handoff, 2, 1, [{k}])
    # ... and in 4:2:0, where the pair's blocks are six apart
    k = (20 + (which == "odd")) * 6 + 2
    f, _ = _file(128, 128, "420", 1, {k: _only(63)})
    _check([f], handoff, 1, 6, [{k}])


def test_blocks_that_end_at_31_at_32_and_at_63(handoff):
    """last non-zero coefficient at 31 and an EOB behind it: unflagged everywhere; a non-zero at 32 alone or at 63 alone: flagged"""
    f, blocks = _file(128, 64, "gray", 2, {}, last=31)
    assert (blocks[:, 31] != 0).all()
    _check([f], handoff, 2, 1, [set()])
    special = {9: _only(32), 40: _only(63), 41: _only(32), 77: _only(63), 126: _only(32), 127: _only(63)}
    f, _ = _file(128, 64, "gray", 2, special)
    _check([f], handoff, 2, 1, [set(special)])


def test_flags_in_every_pass_and_in_none(handoff):
    """noise at Q100 (96 x 64 4:2:0 DRI = 3: eight intervals; 128 x 128 DRI = 1: 64 intervals, all four passes) and flat images"""
    for w, h, dri in ((96, 64, 3), (128, 128, 1)):
        noise = bytes(jpegsynth.encode(w, h, "420", 100, dri, seed=21))
        flagged = (_ref(noise)[1][:, 32:] != 0).any(axis=1)
        assert flagged.mean() > 0.9
        n_int = len(flagged) // 6 // dri
        assert all(flagged.reshape(n_int, -1)[16 * p:16 * p + 16].any() for p in range(-(-n_int // 16)))  # (every pass that has lanes)
        flat, _ = _file(w, h, "420", dri, {}, last=0)
        _check([noise, flat], handoff, dri, 6, [None, set()])


@pytest.mark.parametrize("w,h,n_int", [(80, 56, 18), (56, 56, 13)])
def test_short_last_interval_holds_the_flagged_block(w, h, n_int, handoff):
    """gray DRI = 4: 70 blocks in 18 intervals, the last of two MCUs; 49 blocks in 13 (an odd count), the last of one"""
    n = (w // 8) * (h // 8)
    assert -(-n // 4) == n_int and n % 4 != 0
    f, _ = _file(w, h, "gray", 4, {n - 1: _only(50)})
    _check([f], handoff, 4, 1, [{n - 1}])


@pytest.mark.parametrize("steps,shape", [(63, (144, 56)), (64, (128, 64)), (65, (104, 80))])
def test_waves_of_63_64_and_65_block_steps(steps, shape, handoff):
    """gray, two intervals of `steps` MCUs: the flag store goes out at step 63 and the scan ends on it, in front of it or one behind it;
    flagged blocks in the steps either side of the store"""
    assert (shape[0] // 8) * (shape[1] // 8) == 2 * steps
    special = {m: _only(33 + m % 30) for m in (0, 61, 62, steps - 1)}
    special.update({steps + m: _only(34 + m % 29) for m in (1, 62, steps - 1)})
    f, _ = _file(*shape, "gray", steps, special)
    _check([f], handoff, steps, 1, [set(special)])


# ---- the staging stays zero from one chunk of a wave to the next

def _noise_mcus(rng, n):
    """n MCUs of 4:2:0 whose every block reaches coefficient 63 (quantisation of ones: what noise at Q100 gives)"""
    out = []
    for _ in range(n):
        blk = rng.integers(-200, 201, size=(6, 64)).astype(np.int16)
        blk[:, 63] |= 1
        out.append(blk)
    return out


def _flat_mcu():
    blk = np.zeros((6, 64), np.int16)
    blk[:, 0] = 40
    return blk


def test_pooled_waves_carry_no_hi_half_into_their_next_chunk(handoff):
    """One upload of 1080p 4:2:0 DRI = 1 images (8 160 intervals = 128 chunks each, the same tables: one pool) with more chunks than the
    pooled launch has waves.  The first images are noise -- as many as it takes for EVERY wave's first chunk to be one of theirs: a wave
    that finishes takes the next ticket, so the flat images behind them are decoded by waves that have had flagged blocks in every
    lane's staging.  A hi half left behind would show in a flat image's coefficients and flag words."""
    noise_iv = _noise_mcus(np.random.default_rng(17), 7)
    order = [i % 7 for i in range(8160)]
    noise = _write(1920, 1080, "420", 1, noise_iv, order, full_tables=True)
    flat = _write(1920, 1080, "420", 1, [_flat_mcu()], [0] * 8160, full_tables=True)
    assert (_ref(noise)[1][:, 32:] != 0).any(axis=1).all()
    assert not _ref(flat)[1][:, 1:].any()  # all-zero AC
    probe = jl.Batch().upload([flat, flat], jl.FMT_INTERLEAVED_U8)
    _DEBUG.jpgpu_debug_batch_cus.argtypes = [C.c_void_p]
    cus = _DEBUG.jpgpu_debug_batch_cus(probe._h)
    assert cus > 0
    waves = probe.plan_stats()["huffman_waves"] * cus  # (a pooled launch: one workgroup per CU, huffman_waves waves each)
    probe.close()
    n_noise = -(-waves // 128)
    files = [noise] * n_noise + [flat] * 2
    assert len(files) * 128 > waves
    stats = _check(files, handoff, 1, 6)
    assert stats["k2_pools"] == 1 and stats["k2_plain_work"] == 0, stats


def test_the_same_contents_through_the_plain_kernel(handoff):
    """Tables that differ from scan to scan and one chunk per scan: nothing is pooled, every image takes huffman_decode_kernel (a wave
    of it decodes one chunk and ends, so there is no second chunk to carry anything into; what this pins is the flush itself there)."""
    noise_iv = _noise_mcus(np.random.default_rng(18), 5)
    files = []
    for k in range(6):  # noise, flat, noise, ...: the file's own symbols make its tables; the noise files differ in one block
        if k % 2 == 0:
            iv = [m.copy() for m in noise_iv]
            iv[0][5, 1:] = 0
            iv[0][5, 1 + k] = 1 << 9  # a symbol of its own: a run of k zeros in front of a ten-bit value
            files.append(_write(128, 128, "420", 1, iv, [i % 5 for i in range(64)]))
        else:
            files.append(_write(128, 128, "420", 1, [_flat_mcu()], [0] * 64))
    for f in files[1::2]:
        assert not _ref(f)[1][:, 1:].any()
    stats = _check(files, handoff, 1, 6)
    assert stats["k2_pools"] == 0 and stats["k2_plain_work"] >= len(files), stats
