"""The inputs of tests/test_transcode_regimes_gpu.py, proven against the oracle alone.

Each input is aimed at one place where the optimizer's transcode kernels (kt_transcode.hip: KT for restart intervals, KTS for DRI = 0)
decide something, and carries a PRECONDITION: the property of the oracle's output, or of the writer's own bit positions, that makes the
input reach that place.  This file checks, without a GPU, that the oracle optimizes every input, that the optimized file still holds
the coefficients that were written, and that every precondition holds.  The preconditions are conditions, not measurements: an input
that misses one gets another seed or size.  The GPU suite asserts them again, so a later edit of a generator cannot empty a case.

The catalogue (INPUTS, build, oracle, check_precondition) is shared with the GPU suite; everything is generated in memory."""
import functools

import numpy as np
import pytest

import scan_writer as sw
from golden_util import read_jpeg
from oracle import pyoracle as po
from tools import jpegsynth

KTS_MIN_BYTES = 512          # a DRI = 0 scan shorter than this goes through the interval kernel as ONE interval (device_batch_layout.cpp)
STUFF_CHUNK = 4096           # kEncStuffChunk: the stuffing stage's chunk, with a per-chunk FF prefix count
SAMPLINGS = {"4x1": ((4, 1), (1, 1), (1, 1)), "2x2_2x1_1x2": ((2, 2), (2, 1), (1, 2)), "4x2_2x2_1x1": ((4, 2), (2, 2), (1, 1))}


class Input:
    def __init__(self, name, data, dri, coefs=None, info=None, most_optimal=False, precondition=None):
        self.name, self.data, self.dri, self.coefs, self.info = name, data, dri, coefs, info
        self.most_optimal, self.precondition = most_optimal, precondition


def _written(name, coefs, bw, bh, ncomp=1, dri=0, shape="flat", **kw):
    data, info = sw.write_baseline(coefs, bw * 8, bh * 8, ncomp, dri, shape)
    assert not dri or (bw * bh) % dri, "a DRI that divides the MCU count makes the reference give up (tested elsewhere)"
    return Input(name, data, dri, np.asarray(coefs, np.int16), info, **kw)


def _zeros(bw, bh):
    return np.zeros((bw * bh, 64), np.int16)


def _ff_gray(bw, bh):
    c = _zeros(bw, bh)
    c[:, 1:40] = 255  # eight magnitude bits, all ones
    return c


def _ff_color(bw, bh, seed):
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array([127, 255, 511, 1023], np.int16), (bw * bh * 3, 64))  # magnitudes of 7 .. 10 one bits
    c[:, 0] = rng.integers(-1000, 1001, bw * bh * 3)
    return c


def _ranked_symbols(counts, seed, runs):
    """Blocks whose AC symbols (run, size), run < `runs`, occur counts[k] times for the k-th symbol in the order size 1 .. 10, run
    0 .. runs - 1 inside a size: the rarest symbols carry the longest magnitudes, so the longest output codes sit in front of ten
    magnitude bits.  The symbols come in a seeded random order; a block is closed with EOB when the next one does not fit."""
    rng = np.random.default_rng(seed)
    kinds = [(r, s) for s in range(1, 11) for r in range(runs)][:len(counts)]
    assert len(kinds) == len(counts)
    order = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(order)
    blocks, blk, k = [], np.zeros(64, np.int16), 1
    for o in order:
        r, s = kinds[o]
        if k + r > 63:
            blocks.append(blk)
            blk, k = np.zeros(64, np.int16), 1
        v = int(rng.integers(1 << (s - 1), 1 << s))
        blk[k + r] = v if rng.integers(2) else -v
        k += r + 1
    blocks.append(blk)
    return blocks


def _pad_to_grid(blocks, dri_free=(5,)):
    """the smallest bw x bh grid (bw within one of bh) that holds the blocks and whose MCU count no interval of dri_free divides"""
    n = len(blocks)
    bw = int(np.ceil(np.sqrt(n)))
    while any(bw % d == 0 for d in dri_free):
        bw += 1
    bh = (n + bw - 1) // bw
    while any((bw * bh) % d == 0 for d in dri_free) and bh < n + 64:
        bh += 1
    assert all((bw * bh) % d for d in dri_free)
    out = np.zeros((bw * bh, 64), np.int16)
    out[:n] = np.stack(blocks)
    dc = np.random.default_rng(n).integers(-300, 301, bw * bh)
    out[:, 0] = dc
    return out, bw, bh


def _fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n][::-1]  # falling


def _dense(bw, bh, seed, lo, hi, n_ac=63):
    """every block: the first n_ac AC coefficients nonzero with sizes lo .. hi, DC uniform in +-500"""
    rng = np.random.default_rng(seed)
    n = bw * bh
    size = rng.integers(lo, hi + 1, (n, n_ac))
    mag = (rng.random((n, n_ac)) * (1 << (size - 1))).astype(np.int64) + (1 << (size - 1))
    c = np.zeros((n, 64), np.int16)
    c[:, 1:1 + n_ac] = np.where(rng.integers(0, 2, (n, n_ac)) == 1, mag, -mag)
    c[:, 0] = rng.integers(-500, 501, n)
    return c


# ---- preconditions: (input, the oracle's output with strip = False) -> raises AssertionError when the input misses its place

def _single_symbol(inp, opt):
    lengths, _ = sw.parse_baseline(opt)
    assert sorted(lengths) == [(0, 0), (1, 0)] and all(list(t.values()) == [1] for t in lengths.values()), lengths


def _ff_at_chunk_edges(inp, opt):
    raw = sw.unstuff(sw.parse_baseline(opt)[1])
    chunks = (len(raw) + STUFF_CHUNK - 1) // STUFF_CHUNK
    edges = [k * STUFF_CHUNK for k in range(1, chunks) if raw[k * STUFF_CHUNK - 1] == 0xFF or raw[k * STUFF_CHUNK] == 0xFF]
    assert chunks >= 4 and len(edges) >= 3, (len(raw), raw.count(0xFF), edges)


def _ff_in_many_intervals(inp, opt):
    scan = sw.parse_baseline(opt)[1]
    cuts = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    parts = [scan[a:b] for a, b in zip([0] + [c + 2 for c in cuts], cuts + [len(scan)])]
    assert len(parts) == len(inp.info["intervals"])
    assert sum(b"\xff\x00" in p for p in parts) >= 100, len(parts)


def _code_of_16_bits(inp, opt):
    lengths, _ = sw.parse_baseline(opt)
    assert max(lengths[(1, 0)].values()) == 16, sorted(lengths[(1, 0)].values())


def _subsequences_inside_a_block(inp, opt):
    """at shift 9: ten or more 512-bit subsequences that lie wholly inside one block (their lanes own no block: count == 0), two or
    more of them in a row somewhere"""
    edges = np.array(inp.info["block_bits"] + [sw.unstuffed_length(inp.info) * 8])
    n_subs = -(-int(edges[-1]) // 512)
    lo = np.arange(n_subs) * 512
    # no block starts in [lo, lo + 512): the subsequence is inside the block that started before it
    starts = np.searchsorted(edges[:-1], lo, "left")
    inside = (starts == np.searchsorted(edges[:-1], lo + 512, "left")) & (lo + 512 <= edges[-1])
    runs = np.flatnonzero(inside[1:] & inside[:-1])
    assert inside.sum() >= 10 and len(runs) >= 1, (int(inside.sum()), len(runs))


def n_subs_at_shift_9(inp):
    return -(-sw.unstuffed_length(inp.info) * 8 // 512)


def _subs(lo, hi):
    def check(inp, opt):
        assert sw.unstuffed_length(inp.info) >= KTS_MIN_BYTES and lo <= n_subs_at_shift_9(inp) <= hi, n_subs_at_shift_9(inp)
    return check


def _intervals(lo, hi):
    def check(inp, opt):
        assert lo <= len(inp.info["intervals"]) <= hi, len(inp.info["intervals"])
    return check


# ---- the catalogue

def _zero(bw, bh, dri=0):
    return lambda name: _written(name, _zeros(bw, bh), bw, bh, dri=dri, precondition=_single_symbol)


def _codes16(most_optimal, dri, shape):
    def make(name):
        if most_optimal:  # package merge: Fibonacci counts use every length 1 .. 16
            blocks = _ranked_symbols(_fibonacci(20), 5, runs=2)
        else:  # the default builder holds about two codes per length: 32 or more symbols of falling frequency
            blocks = _ranked_symbols([max(1, int(1.4 ** k)) for k in range(32)][::-1], 6, runs=4)
        coefs, bw, bh = _pad_to_grid(blocks)
        return _written(name, coefs, bw, bh, dri=dri, shape=shape, most_optimal=most_optimal, precondition=_code_of_16_bits)
    return make


def _synth(w, h, sampling, dri):
    return lambda name: Input(name, bytes(jpegsynth.encode(w, h, quality=75, restart_interval=dri, seed=w + dri, sampling=SAMPLINGS[sampling])), dri)


_MAKERS = {
    # single-symbol tables: every code one bit.  Raw totals of 8 / 32 / 30 / 512 / 3200 bits on the interval kernel (scans below
    # 512 bytes), 8192 / 8190 bits through KTS: pad == 0, fill == 0 at the end, and a last word partly filled
    "zero_2x2": _zero(2, 2), "zero_4x4": _zero(4, 4), "zero_5x3": _zero(5, 3), "zero_16x16": _zero(16, 16), "zero_40x40": _zero(40, 40),
    "zero_5x3_dri2": _zero(5, 3, 2), "zero_64x64": _zero(64, 64), "zero_65x63": _zero(65, 63),
    # magnitudes of all ones: FF bytes everywhere, at the stuffing stage's chunk edges too
    "ff_gray": lambda name: _written(name, _ff_gray(24, 24), 24, 24, precondition=_ff_at_chunk_edges),
    "ff_color": lambda name: _written(name, _ff_color(24, 24, 1), 24, 24, ncomp=3, precondition=_ff_at_chunk_edges),
    "ff_gray_dri5": lambda name: _written(name, _ff_gray(24, 24), 24, 24, dri=5, precondition=_ff_in_many_intervals),
    "ff_color_dri5": lambda name: _written(name, _ff_color(24, 24, 1), 24, 24, ncomp=3, dri=5, precondition=_ff_in_many_intervals),
    # output codes of 16 bits in front of ten magnitude bits
    "codes16_merge": _codes16(True, 0, "flat"), "codes16_merge_dri5": _codes16(True, 5, "flat"),
    "codes16_default": _codes16(False, 0, "deep"), "codes16_default_dri5": _codes16(False, 5, "deep"),
    # blocks of more than 1000 bits: subsequences of 512 bits that hold no block start
    "long_blocks": lambda name: _written(name, _dense(12, 12, 2, 8, 10), 12, 12, precondition=_subsequences_inside_a_block),
    # scan sizes: one workgroup of subsequences, several, the offset scan's per > 1 (above 1024), per == 4
    "subs_le_256": lambda name: _written(name, _dense(8, 8, 3, 1, 6), 8, 8, precondition=_subs(1, 256)),
    "subs_le_1024": lambda name: _written(name, _dense(20, 20, 4, 1, 6), 20, 20, precondition=_subs(257, 1024)),
    "subs_le_2048": lambda name: _written(name, _dense(33, 33, 5, 1, 6), 33, 33, precondition=_subs(1025, 2048)),
    "subs_gt_3072": lambda name: _written(name, _dense(48, 48, 6, 1, 6), 48, 48, precondition=_subs(3073, 1 << 20)),
    # interval counts: one workgroup of intervals, several, the offset scan's per > 1.  (DRI = 1 divides every MCU count, which makes
    # the reference give up: DRI = 2 on odd MCU counts.)
    "intervals_le_256": lambda name: _written(name, _dense(15, 15, 7, 1, 4, 5), 15, 15, dri=2, precondition=_intervals(1, 256)),
    "intervals_le_1024": lambda name: _written(name, _dense(33, 33, 8, 1, 4, 5), 33, 33, dri=2, precondition=_intervals(257, 1024)),
    "intervals_gt_1024": lambda name: _written(name, _dense(47, 47, 9, 1, 4, 5), 47, 47, dri=2, precondition=_intervals(1025, 1 << 20)),
    "testorig12": lambda name: Input(name, read_jpeg("testorig12.jpg"), 0),
}
# per-component sampling factors (up to 13 blocks per MCU), with and without restart intervals.  DRI = 3 divides the MCU count of four
# of the six layouts (the reference gives up: the same exception class is expected); DRI = 4 divides none of them.
for _s in SAMPLINGS:
    for _w, _h in ((48, 40), (129, 65)):
        for _dri in (0, 3, 4):
            _MAKERS[f"sampling_{_s}_{_w}x{_h}_dri{_dri}"] = _synth(_w, _h, _s, _dri)

INPUTS = list(_MAKERS)
WRITTEN = [n for n in INPUTS if not n.startswith(("sampling_", "testorig12"))]


@functools.lru_cache(maxsize=None)
def build(name) -> Input:
    return _MAKERS[name](name)


@functools.lru_cache(maxsize=None)
def oracle(name, strip):
    """the oracle's optimized bytes, or the OracleError it raised"""
    inp = build(name)
    try:
        return po.optimize(inp.data, strip, most_optimal=inp.most_optimal)
    except po.OracleError as e:
        return e


def check_precondition(name):
    inp = build(name)
    if inp.precondition is not None:
        opt = oracle(name, False)
        assert isinstance(opt, bytes), opt
        inp.precondition(inp, opt)


def truncated(name, where, min_sub=300, eoi=True):
    """A written DRI = 0 input cut at a byte edge that lies inside subsequence `min_sub` or a later one at shift 9 and
    where == "block": exactly between two blocks; "code": inside a code word; "magnitude": inside a symbol's magnitude bits.
    Returns (file, subsequence the cut lies in)."""
    inp = build(name)
    first_of_block = set(inp.info["block_bits"])
    for pos, ln, s, _ in inp.info["symbols"]:
        cut = (pos + 7) // 8 * 8 if where != "magnitude" else (pos + ln + 7) // 8 * 8
        if cut < min_sub * 512:
            continue
        if (where == "block" and cut == pos and pos in first_of_block) or (where == "code" and pos < cut < pos + ln) or \
           (where == "magnitude" and pos + ln < cut < pos + ln + s):
            break
    else:
        raise AssertionError(f"{name} has no such cut")
    head = inp.info["header_bytes"]
    entropy = inp.data[head:-2]
    return inp.data[:head + sw.stuffed_offset(entropy, cut // 8)] + (b"\xff\xd9" if eoi else b""), cut // 512


# ---- the checks of this file

@pytest.mark.parametrize("name", INPUTS)
def test_the_oracle_takes_the_input_and_keeps_its_coefficients(name):
    inp = build(name)
    ref_coefs = inp.coefs if inp.coefs is not None else po.decode_coefficients(inp.data)[0]
    if inp.coefs is not None:  # (the oracle reads the file: the writer wrote what it meant to)
        assert np.array_equal(po.decode_coefficients(inp.data)[0], inp.coefs)
    for strip in (False, True):
        opt = oracle(name, strip)
        if inp.dri and _mcus(inp) % inp.dri == 0:  # the reference gives up (written inputs never get here: _written)
            assert name not in WRITTEN and isinstance(opt, po.OracleError) and opt.kind == "InvalidOperationException", opt
        else:
            assert isinstance(opt, bytes), opt
            if not (strip and inp.dri):  # (strip drops the DRI segment with the other "default" markers: such a file no longer decodes)
                assert np.array_equal(po.decode_coefficients(opt)[0], ref_coefs)


def _mcus(inp):
    info, _ = po.identify(inp.data)
    comps = [info.comp[i] for i in range(info.ncomp)]
    hmax, vmax = max(c.h for c in comps), max(c.v for c in comps)
    return -(-info.width // (8 * hmax)) * -(-info.height // (8 * vmax))


@pytest.mark.parametrize("name", WRITTEN)
def test_the_input_reaches_the_place_it_is_named_for(name):
    assert build(name).precondition is not None
    check_precondition(name)


def test_the_single_symbol_scans_have_the_lengths_their_bit_totals_give():
    """2 bits per block, padded with ones to a byte: 8 / 32 / 30 / 512 / 3200 / 8192 / 8190 bits; with DRI = 2 eight intervals of one
    byte and seven RSTn"""
    want = {"zero_2x2": 1, "zero_4x4": 4, "zero_5x3": 4, "zero_16x16": 64, "zero_40x40": 400, "zero_64x64": 1024, "zero_65x63": 1024,
            "zero_5x3_dri2": 22}
    for name, n in want.items():
        lengths, scan = sw.parse_baseline(oracle(name, False))
        assert len(scan) == n == sw.expected_scan_length(build(name).info, lengths, scan), (name, len(scan))
    assert sw.parse_baseline(oracle("zero_5x3_dri2", False))[1].count(0xFF) == 7


def test_the_writer_counts_what_the_oracle_counts():
    """info's symbol counts against the oracle's Scan() statistics, and the scan-length arithmetic against the oracle's output"""
    for name in ("ff_color", "ff_gray_dri5", "codes16_default", "long_blocks", "intervals_le_256"):
        inp = build(name)
        stats = {(c, t): f for c, t, f in po.optimizer_statistics(inp.data)}
        assert sorted(stats) == sorted(inp.info["tables"])
        for key, counts in inp.info["tables"].items():
            assert {int(s): int(n) for s, n in enumerate(stats[key]) if n} == counts, (name, key)
        lengths, scan = sw.parse_baseline(oracle(name, False))
        assert len(scan) == sw.expected_scan_length(inp.info, lengths, scan), name
        assert len(inp.data) == inp.info["header_bytes"] + inp.info["entropy_bytes"] + 2


def test_truncations_lie_where_they_are_meant_to():
    """the mixed batch's failing file: cut behind subsequence 300 at shift 9 (the second workgroup of its scan), and the oracle throws"""
    inp = build("subs_le_1024")
    for where in ("block", "code", "magnitude"):
        data, sub = truncated("subs_le_1024", where)
        assert 300 <= sub < n_subs_at_shift_9(inp) and data[:inp.info["header_bytes"]] == inp.data[:inp.info["header_bytes"]]
        with pytest.raises(po.OracleError):
            po.optimize(data, False)
    with pytest.raises(po.OracleError):
        po.optimize(truncated("subs_le_1024", "code", eoi=False)[0], False)
