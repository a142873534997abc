"""The inputs of tests/test_entropy_stages_gpu.py, proven against the oracle alone.

The encoder's entropy stages (encode_kernels.hip: E2 block_bits_kernel / block_stats_kernel / block_offsets_kernel, E3 emit_kernel and
bits_emit_kernel, E4 stuff_count_kernel / stuff_write_kernel) serve the encoder, the optimizer's DRI = 0 road and the optimizer's whole
coefficient road.  Each input here is aimed at one place where they decide something and carries a PRECONDITION: the property of the
oracle's output, or of the writer's own symbols priced with the output's tables, that makes the input reach that place.  Two kinds:

  WRITTEN  coefficients written by tests/scan_writer.py.  Sent down the optimizer's coefficient road unturned (a window that is the whole
           frame), they are exactly what block_stats_kernel<true>, block_bits_kernel<true>, emit_kernel<true> and the stuffing pair see.
  FLAT     pixels.  At quality 100 the standard tables are all ones, so a grey image of flat 8 x 8 blocks of value p has DC 8 (p - 128) and
           no AC: a block costs 6, 11, 12, 14, 16, 18, 20, 22 or 24 bits by the category of its DC difference, and bit totals, word phases
           of workgroup bases and FF bytes are placed from pixels.  These reach the kernels' <false> forms and bits_emit_kernel.

This file checks, without a GPU, that the oracle takes every input, that its output holds what was written or designed, that every
precondition holds, and that the scan is as long as the priced symbols say.  The preconditions are conditions, not measurements: an input
that misses one gets another seed or size.  The GPU suite asserts them again."""
import functools

import numpy as np
import pytest

import scan_writer as sw
import test_transcode_inputs_cpu as cat
from oracle import pyoracle as po

STUFF_CHUNK = cat.STUFF_CHUNK  # kStuffChunk: raw bytes per workgroup of the stuffing pair, 256 lanes x 16 bytes
UNITS_PER_WG = 256             # blocks, or restart intervals, per workgroup of E2 / E3
# emit_kernel's LDS buffer in words.  The host asks for twice the largest AVERAGE stretch of any image whose average is within the
# maximum, rounded up to 1024 words (EncodeBatch::plan_stuffing in device_encode.cpp, OptimizeBatch::emit_turned in device_optimize.cpp);
# launch_emit clamps what is not zero to kEmitLdsWordsMin .. kEmitLdsWordsMax (encode_kernels.h)
EMIT_LDS_WORDS_MIN, EMIT_LDS_WORDS_MAX = 2048, 8192


# ------------------------------------------------------------------------------------------------ what the kernels make of an image

def unit_bits(n_blocks_per_unit, block_bits, rounded):
    """bits of every unit a lane takes: one block, or one restart interval rounded up to whole bytes"""
    bits = np.asarray(block_bits, np.int64)
    if not rounded:
        return bits
    units = np.add.reduceat(bits, np.arange(0, len(bits), n_blocks_per_unit))
    return (units + 7) // 8 * 8


def workgroup_bases(units):
    """first bit of every workgroup's stretch, and the total (raw_bits: without the pad of a DRI = 0 stream)"""
    per_wg = np.add.reduceat(units, np.arange(0, len(units), UNITS_PER_WG))
    return [int(b) for b in np.concatenate([[0], np.cumsum(per_wg)[:-1]])], int(per_wg.sum())


def average_stretch_words(total_bits, n_wg):
    return total_bits // 32 // n_wg + 1


def emit_lds_words(images):
    """images: [(total bits, workgroups)] of one launch -> the words emit_kernel gets (0: no LDS at all)"""
    want = max([2 * average_stretch_words(t, n) for t, n in images if average_stretch_words(t, n) <= EMIT_LDS_WORDS_MAX], default=0)
    words = min((want + 1023) // 1024 * 1024, EMIT_LDS_WORDS_MAX)
    return 0 if words == 0 else min(max(words, EMIT_LDS_WORDS_MIN), EMIT_LDS_WORDS_MAX)


def stretch_words(bases, total_bits):
    """the words every workgroup's stretch spans, counted as emit_kernel counts them: from the word its first bit lies in to its last bit
    (the last workgroup's: the total rounded up to a byte)"""
    ends = bases[1:] + [(total_bits + 7) // 8 * 8]
    return [(e - (b // 32) * 32 + 31) // 32 for b, e in zip(bases, ends)]


# ------------------------------------------------------------------------------------------------ written inputs

def _written(name, coefs, bw, bh, ncomp=1, dri=0, shape="flat", **kw):
    inp = cat._written(name, coefs, bw, bh, ncomp=ncomp, dri=dri, shape=shape, **kw)
    inp.ncomp, inp.size = ncomp, (bw * 8, bh * 8)
    return inp


def written_units(inp, opt):
    """the units of a written input priced with the DHT of `opt`, the oracle's output"""
    lengths, _ = sw.parse_baseline(opt)
    return unit_bits(inp.ncomp * inp.dri, sw.priced_block_bits(inp.info, lengths), inp.dri != 0)


def _last_coefficient(bw, bh):
    c = cat._zeros(bw, bh)
    c[:, 63] = 255  # a run of 62 zeros: three ZRLs in a row, then (14, 8) with eight magnitude bits of ones, and no EOB
    return c


def _fat_workgroup():
    c = cat._zeros(32, 40)
    c[256:512, 1:] = np.random.default_rng(21).integers(-1000, 1001, (256, 63))
    return c


def _no_eob_last_ff(inp, opt):
    lengths, scan = sw.parse_baseline(opt)
    assert sorted(lengths[(1, 0)]) == [0xE8, 0xF0], lengths[(1, 0)]
    assert scan[-2:] == b"\xff\x00", scan[-4:].hex()


def _marked_ff(inp, opt):
    scan = sw.parse_baseline(opt)[1]
    hits = sum(scan[i] == 0xFF and scan[i + 1] == 0 and scan[i + 2] == 0xFF and 0xD0 <= scan[i + 3] <= 0xD7 for i in range(len(scan) - 3))
    assert hits >= 100, (hits, len(inp.info["intervals"]))


def _every_byte_marked(inp, opt):
    n = len(inp.info["intervals"])
    assert n >= STUFF_CHUNK + 1, n
    assert set(written_units(inp, opt).tolist()) == {8}
    scan = sw.parse_baseline(opt)[1]
    assert scan == b"".join(bytes([0x0F, 0xFF, 0xD0 + (k & 7)]) for k in range(n - 1)) + b"\x3f"  # (the last interval holds one block)
    assert scan[3 * STUFF_CHUNK - 1] == 0xD0 + ((STUFF_CHUNK - 1) & 7) and scan[3 * STUFF_CHUNK + 2] == 0xD0 + (STUFF_CHUNK & 7)


def marks_per_chunk(units):
    """marked bytes -- the last byte of every interval but the last -- in every stuffing chunk of the raw stream"""
    last_bytes = np.cumsum(np.asarray(units) // 8)[:-1] - 1
    return np.bincount(last_bytes // STUFF_CHUNK).tolist()


def _marker_number_carried(inp, opt):
    """three or more chunks, and in front of every chunk but the first a number of markers that is no multiple of 8: a counter that
    restarted per chunk would write another RSTn"""
    marks = marks_per_chunk(written_units(inp, opt))
    assert len(marks) >= 3 and all(int(c) % 8 for c in np.cumsum(marks)[:-1]), marks


def _fat_workgroup_alone(inp, opt):
    bases, total = workgroup_bases(written_units(inp, opt))
    lds = emit_lds_words([(total, len(bases))])
    words = stretch_words(bases, total)
    assert len(bases) == 5 and lds != 0 and words[1] > lds and all(w < lds for k, w in enumerate(words) if k != 1), (lds, words)


def _no_lds_alone(inp, opt):
    bases, total = workgroup_bases(written_units(inp, opt))
    assert average_stretch_words(total, len(bases)) > EMIT_LDS_WORDS_MAX and emit_lds_words([(total, len(bases))]) == 0, (total, len(bases))


def _edges_on_words(inp, opt):
    bases, total = workgroup_bases(written_units(inp, opt))
    assert len(bases) >= 3 and all(b % 32 == 0 for b in bases) and total % 32 == 0, (bases, total)


def _edges_off_words(inp, opt):
    bases, total = workgroup_bases(written_units(inp, opt))
    assert len(bases) >= 3 and all(b % 8 != 0 for b in bases[1:]), (bases, total)


def _units(n):
    def check(inp, opt):
        units = written_units(inp, opt)
        assert len(units) == n and (len(inp.info["intervals"]) == n if inp.dri else len(inp.info["block_bits"]) == n), len(units)
    return check


def _dc_swings(inp, opt):
    lengths, _ = sw.parse_baseline(opt)
    bases, _ = workgroup_bases(written_units(inp, opt))
    assert len(bases) >= 3 and UNITS_PER_WG % inp.ncomp  # MCUs straddle the workgroups
    assert {9, 10, 11} <= set(lengths[(0, 0)]) and {9, 10, 11} <= set(lengths[(0, 1)]), (sorted(lengths[(0, 0)]), sorted(lengths[(0, 1)]))


_WRITTEN = {
    # enc_block_symbols: three ZRLs in a row and no EOB; the stream's last data byte is FF
    "no_eob_last_ff": lambda name: _written(name, _last_coefficient(5, 3), 5, 3, precondition=_no_eob_last_ff),
    # the marked byte of most intervals is itself FF: FF 00 FF Dn
    "marked_ff": lambda name: _written(name, _last_coefficient(15, 15), 15, 15, dri=2, precondition=_marked_ff),
    # a stuffing chunk in which every byte is marked: both halves of the packed scan are full.  (4096 markers per chunk are a multiple
    # of 8, so the marker NUMBER carried over the edge cannot be told from one that restarts there: the next input's place)
    "every_byte_marked": lambda name: _written(name, cat._zeros(95, 95), 95, 95, dri=2, precondition=_every_byte_marked),
    "marker_number_carried": lambda name: _written(name, cat._dense(41, 41, 39, 1, 4, 5), 41, 41, dri=2, precondition=_marker_number_carried),
    # emit_kernel: one workgroup's stretch beyond the LDS buffer (global atomics) between workgroups that use it
    "fat_workgroup": lambda name: _written(name, _fat_workgroup(), 32, 40, precondition=_fat_workgroup_alone),
    # ... and an image whose average stretch is beyond 32 KB: alone it asks for no LDS at all
    "fat_intervals": lambda name: _written(name, cat._ff_gray(39, 38), 39, 38, dri=5, precondition=_no_lds_alone),
    # workgroup bases on word edges with a whole last word, and off every byte edge
    "wg_edges_on_words": lambda name: _written(name, cat._zeros(32, 32), 32, 32, precondition=_edges_on_words),
    "wg_edges_off_words": lambda name: _written(name, cat._dense(24, 32, 31, 1, 4, 5), 24, 32, precondition=_edges_off_words),
    # the edges of wk.first + 256 >= n_units, one lane per block and one lane per restart interval
    "exact_256": lambda name: _written(name, cat._dense(16, 16, 32, 1, 4, 5), 16, 16, precondition=_units(256)),
    "exact_257": lambda name: _written(name, cat._dense(257, 1, 33, 1, 4, 5), 257, 1, precondition=_units(257)),
    "exact_512": lambda name: _written(name, cat._dense(32, 16, 34, 1, 4, 5), 32, 16, precondition=_units(512)),
    "intervals_256": lambda name: _written(name, cat._dense(73, 7, 35, 1, 4, 5), 73, 7, dri=2, precondition=_units(256)),
    "intervals_257": lambda name: _written(name, cat._dense(27, 19, 36, 1, 4, 5), 27, 19, dri=2, precondition=_units(257)),
    # 4:4:4: 256 is no multiple of 3, so the DC predictor reads across the workgroup edge; DC differences of every large category
    "color_444_dc_swings": lambda name: _written(name, cat._ff_color(16, 16, 3), 16, 16, ncomp=3, precondition=_dc_swings),
}
WRITTEN = list(_WRITTEN)


@functools.lru_cache(maxsize=None)
def build(name) -> cat.Input:
    return _WRITTEN[name](name)


@functools.lru_cache(maxsize=None)
def oracle(name, strip):
    inp = build(name)
    return po.optimize(inp.data, strip, most_optimal=inp.most_optimal)


def check_precondition(name):
    inp = build(name)
    inp.precondition(inp, oracle(name, False))


def launch_of(names):
    """[(total bits, workgroups)] of the named inputs side by side in one upload, and every input's stretches in words"""
    images, words = [], []
    for n in names:
        inp = cat.build(n) if n in cat.INPUTS else build(n)
        inp.ncomp = getattr(inp, "ncomp", 1)
        opt = cat.oracle(n, False) if n in cat.INPUTS else oracle(n, False)
        bases, total = workgroup_bases(written_units(inp, opt))
        images.append((total, len(bases)))
        words.append(stretch_words(bases, total))
    return images, words


# ------------------------------------------------------------------------------------------------ flat-block pixel inputs

DC_BITS = {0: [2, 3, 3, 3, 3, 3, 4, 5, 6, 7, 8, 9], 1: [2, 2, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]}  # Annex K.3: code length by category
EOB_BITS = {0: 4, 1: 2}                                                                      # Annex K.5 / K.6: the code of symbol 0x00


def price_dc(dc, mcu):
    """bits of every block of a scan whose blocks hold nothing but DC: dc[k] its value, mcu the components of one MCU's blocks in scan
    order (component 0 on the luminance tables, the others on the chrominance tables); each component is predicted from its own last
    block.  The standard tables' lengths, from Annex K: no encoder is asked."""
    bits, pred = [], {}
    for k, v in enumerate(dc):
        c = mcu[k % len(mcu)]
        t = 0 if c == 0 else 1
        size = abs(int(v) - pred.get(c, 0)).bit_length()
        pred[c] = int(v)
        bits.append(DC_BITS[t][size] + size + EOB_BITS[t])
    return bits


class Flat:
    def __init__(self, name, pixels, luma, dc, mcu, precondition):
        self.name, self.pixels, self.luma, self.precondition = name, pixels, luma, precondition
        self.dc, self.mcu = np.asarray(dc, np.int64), tuple(mcu)

    @property
    def blocks(self):
        out = np.zeros((len(self.dc), 64), np.int16)
        out[:, 0] = self.dc
        return out


def with_constant_chroma(inp):
    """A grey flat input as a 4:4:4 image with Cb = Cr = 128 (nothing is sub-sampled, so every block stays flat): the reference builds
    tables for three components only -- optimize_coding on one component ends in "No symbol is recorded." -- and with built tables a
    constant image then costs two bits a block, one per table."""
    if inp.pixels.ndim == 3:
        return inp
    dc = np.zeros(3 * len(inp.dc), np.int64)
    dc[0::3] = inp.dc
    return Flat(inp.name + "_444", np.stack([inp.pixels, np.full_like(inp.pixels, 128), np.full_like(inp.pixels, 128)], axis=2), (1, 1), dc, (0, 1, 2), None)


def flat_gray(name, values, bw, bh, precondition):
    """a grey image of bw x bh flat blocks: values[k] is block k's sample, in scan order"""
    values = np.asarray(values, np.uint8)
    assert values.shape == (bw * bh,)
    px = np.kron(values.reshape(bh, bw), np.ones((8, 8), np.uint8))
    return Flat(name, px, (1, 1), 8 * (values.astype(np.int64) - 128), (0,), precondition)


def flat_420(name, y, cb, cr, precondition):
    """Y given per 8 x 8 block ([2 mh, 2 mw]), Cb and Cr per MCU ([mh, mw]): the 2 x 2 averages of the chroma planes are the value itself.
    The reference's WriteScanData adds the samples of a sub-sampled block onto what its one block buffer holds -- the quantised block
    before it -- so a chroma block is flat only behind a block that is all zero: the caller keeps the fourth Y block of every MCU and Cb
    at 128, and Cr carries the swings.  (TransformBlocks, under optimize_coding, starts from zeros: the same blocks either way.)"""
    y, cb, cr = (np.asarray(a, np.uint8) for a in (y, cb, cr))
    mh, mw = cb.shape
    assert y.shape == (2 * mh, 2 * mw) and cr.shape == cb.shape and (y[1::2, 1::2] == 128).all() and (cb == 128).all()
    px = np.stack([np.kron(y, np.ones((8, 8), np.uint8)), np.kron(cb, np.ones((16, 16), np.uint8)), np.kron(cr, np.ones((16, 16), np.uint8))], axis=2)
    dc = []
    for my in range(mh):
        for mx in range(mw):
            dc += [y[2 * my, 2 * mx], y[2 * my, 2 * mx + 1], y[2 * my + 1, 2 * mx], y[2 * my + 1, 2 * mx + 1], cb[my, mx], cr[my, mx]]
    return Flat(name, px, (2, 2), 8 * (np.array(dc, np.int64) - 128), (0, 0, 0, 0, 1, 2), precondition)


def ff_edge_design(targets, n_blocks):
    """Block samples 0 / 255 such that the unstuffed scan holds an FF at every byte offset of `targets`.  A step 0 -> 255 is a DC
    difference of +2040 -- the nine-bit code 111111110, the magnitude 11111111000 --, a step back -2040 -- the same code, 00000000111:
    24 bits either way, eight ones first, so a step that starts on a byte edge puts an FF there.  Between two targets the steps go on
    (three bytes each); the distance left is made up of blocks that repeat the sample (6 bits) and pairs that step by one and back
    (11 + 11 bits)."""
    values, pos, cur = [0], 24, 0  # block 0: 128 -> 0, difference -1024, category 11
    for t in sorted(targets):
        want = 8 * t
        assert want - pos >= 200, "targets too close"
        while want - pos >= 24 + 100:
            cur = 255 - cur
            values.append(cur)
            pos += 24
        rest = want - pos
        pairs = next(b for b in range(3) if (rest - 22 * b) % 6 == 0)
        for _ in range(pairs):
            values += [cur + (1 if cur == 0 else -1), cur]
        values += [cur] * ((rest - 22 * pairs) // 6)
        pos = want
        cur = 255 - cur
        values.append(cur)
        pos += 24
    assert len(values) <= n_blocks, len(values)
    while len(values) < n_blocks:
        cur = 255 - cur
        values.append(cur)
    return values


def flat_units(inp, coefs):
    """the blocks' bits, priced from the DC values of the oracle's own coefficients (which must hold nothing else)"""
    assert not coefs[:, 1:].any()
    return np.asarray(price_dc(coefs[:, 0], inp.mcu), np.int64)


def _flat_const(inp, data, coefs):
    units = flat_units(inp, coefs)
    bases, total = workgroup_bases(units)
    assert set(units.tolist()) == {6} and len(bases) >= 3 and all(b % 32 == 0 for b in bases) and total % 32 == 0, (bases, total)


def _flat_random(inp, data, coefs):
    bases, total = workgroup_bases(flat_units(inp, coefs))
    assert len(bases) >= 3 and any(b % 32 for b in bases[1:]) and total % 8 != 0, (bases, total)


def _flat_byte_end(inp, data, coefs):
    bases, total = workgroup_bases(flat_units(inp, coefs))
    assert len(bases) >= 2 and total % 8 == 0 and total % 32 != 0, (bases, total)


def _flat_ff_edges(inp, data, coefs):
    raw = sw.unstuff(sw.parse_baseline(data)[1])
    chunks = (len(raw) + STUFF_CHUNK - 1) // STUFF_CHUNK
    edges = [k * STUFF_CHUNK for k in range(1, chunks) if raw[k * STUFF_CHUNK - 1] == 0xFF or raw[k * STUFF_CHUNK] == 0xFF]
    last_of_lane = [i for i in range(15, len(raw), 16) if raw[i] == 0xFF]
    first_of_lane = [i for i in range(16, len(raw), 16) if raw[i] == 0xFF]
    assert chunks >= 4 and len(edges) >= 3 and last_of_lane and first_of_lane, (len(raw), edges, len(last_of_lane), len(first_of_lane))
    assert raw[STUFF_CHUNK - 1] == 0xFF and raw[2 * STUFF_CHUNK] == 0xFF  # one edge from each side


def _flat_raw_len(inp, data, coefs):
    _, total = workgroup_bases(flat_units(inp, coefs))
    raw = sw.unstuff(sw.parse_baseline(data)[1])
    assert len(raw) == (total + 7) // 8 and len(raw) % STUFF_CHUNK == 0 and len(raw) > 0, len(raw)


def _flat_blocks(n):
    def check(inp, data, coefs):
        assert len(coefs) == n == len(flat_units(inp, coefs))
    return check


def _flat_420(inp, data, coefs):
    units = flat_units(inp, coefs)
    bases, _ = workgroup_bases(units)
    assert len(bases) >= 3 and UNITS_PER_WG % 6  # bpm = 6: MCUs straddle the workgroups
    chroma = coefs[:, 0].astype(np.int64).reshape(-1, 6)[:, 4:]
    cats = {abs(int(d)).bit_length() for col in (0, 1) for d in np.diff(np.concatenate([[0], chroma[:, col]]))}
    assert max(cats) >= 8, sorted(cats)


def _random_values(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n)


def _make_flat_420(name):
    rng = np.random.default_rng(44)
    y = rng.integers(0, 256, (24, 40))
    y[1::2, 1::2] = 128
    return flat_420(name, y, np.full((12, 20), 128), rng.integers(0, 256, (12, 20)), _flat_420)


_FLAT = {
    # bits_emit_kernel: p == 0 and r == 0 everywhere, no partial last word; with restart_interval = 1 every interval is one byte
    "flat_const": lambda name: flat_gray(name, [128] * 768, 32, 24, _flat_const),
    # ... p != 0 at an interior workgroup (the predecessor's tail supplies the missing bits), a partial last word with pad
    "flat_random": lambda name: flat_gray(name, _random_values(768, 41), 24, 32, _flat_random),
    # ... r != 0 and rem == 0: a partial last word without pad
    "flat_byte_end": lambda name: flat_gray(name, _random_values(520, 105), 26, 20, _flat_byte_end),
    # the stuffing pair: FF in the last byte of a lane's 16 and in the first of the next lane's, and either side of three chunk edges
    "flat_ff_edges": lambda name: flat_gray(name, ff_edge_design([47, 96, 4095, 8192, 12288], 72 * 60), 72, 60, _flat_ff_edges),
    # raw_len a multiple of 4096 (and of 16): the last lane of the last chunk holds 16 bytes and writes EOI
    "flat_raw_len_4096k": lambda name: flat_gray(name, [128] * 5461, 43, 127, _flat_raw_len),
    # one workgroup; one workgroup and one block
    "flat_256": lambda name: flat_gray(name, _random_values(256, 43), 16, 16, _flat_blocks(256)),
    "flat_257": lambda name: flat_gray(name, _random_values(257, 45), 257, 1, _flat_blocks(257)),
    # three components, six blocks per MCU, chroma tables
    "flat_420": _make_flat_420,
}
FLAT = list(_FLAT)


@functools.lru_cache(maxsize=None)
def build_flat(name) -> Flat:
    return _FLAT[name](name)


@functools.lru_cache(maxsize=None)
def flat_oracle(name):
    """(file, coefficients) of the oracle's encoder at quality 100, standard tables, no restart interval"""
    inp = build_flat(name)
    return po.encode_8bit(inp.pixels, inp.luma[0], inp.luma[1], 100, want_coefficients=True)


def check_flat_precondition(name):
    inp = build_flat(name)
    inp.precondition(inp, *flat_oracle(name))


# ------------------------------------------------------------------------------------------------ the checks of this file

@pytest.mark.parametrize("name", WRITTEN)
def test_the_oracle_takes_the_written_input_and_keeps_its_coefficients(name):
    inp = build(name)
    assert np.array_equal(po.decode_coefficients(inp.data)[0], inp.coefs)  # (the writer wrote what it meant to)
    for strip in (False, True):
        opt = oracle(name, strip)
        if not (strip and inp.dri):  # (strip drops the DRI segment with the other "default" markers: such a file no longer decodes)
            assert np.array_equal(po.decode_coefficients(opt)[0], inp.coefs)
    lengths, scan = sw.parse_baseline(oracle(name, False))
    assert len(scan) == sw.expected_scan_length(inp.info, lengths, scan)


@pytest.mark.parametrize("name", WRITTEN)
def test_the_written_input_reaches_the_place_it_is_named_for(name):
    assert build(name).precondition is not None
    check_precondition(name)


def test_the_priced_blocks_add_up_to_the_scan():
    """written_units against the oracle's scan: the units, the pad of a DRI = 0 stream, two bytes per marker, one per stuffed FF"""
    for name in WRITTEN:
        inp = build(name)
        scan = sw.parse_baseline(oracle(name, False))[1]
        _, total = workgroup_bases(written_units(inp, oracle(name, False)))
        assert len(scan) == (total + 7) // 8 + 2 * (len(inp.info["intervals"]) - 1) + scan.count(b"\xff\x00"), name


def test_the_batch_of_fat_and_thin_images_mixes_lds_and_fallback_workgroups():
    """fat_intervals | zero_64x64 | fat_workgroup in one launch: the buffer is sized by the thin images; fat_intervals' full workgroup and
    fat_workgroup's workgroup 1 do not fit it, every other workgroup does (fat_intervals' last, of four intervals, among them)"""
    images, words = launch_of(["fat_intervals", "zero_64x64", "fat_workgroup"])
    lds = emit_lds_words(images)
    assert lds != 0 and emit_lds_words(images[:1]) == 0
    assert [[w > lds for w in image] for image in words] == [[True, False], [False] * 16, [False, True, False, False, False]], (lds, words)


def test_the_written_figures_found_when_the_inputs_were_made():
    lengths, scan = sw.parse_baseline(oracle("no_eob_last_ff", False))
    assert lengths[(1, 0)] in ({0xF0: 1, 0xE8: 2}, {0xF0: 2, 0xE8: 1}) and scan[-4:].hex() == "f0bfff00"
    assert len(build("every_byte_marked").info["intervals"]) == 4513 and len(sw.parse_baseline(oracle("every_byte_marked", False))[1]) == 13537
    inp = build("fat_workgroup")
    bases, total = workgroup_bases(written_units(inp, oracle("fat_workgroup", False)))
    assert [b - a for a, b in zip(bases, bases[1:] + [total])] == [1280, 179686, 1280, 1280, 1280] and emit_lds_words([(total, 5)]) == 3072
    assert stretch_words(bases, total)[1] == 5616


@pytest.mark.parametrize("name", FLAT)
def test_the_flat_blocks_come_out_as_designed(name):
    """coefs[:, 0] is the designed DC sequence, every AC coefficient is zero, and the scan is as long as the blocks priced with the
    standard tables' lengths plus the bytes stuffed"""
    inp = build_flat(name)
    data, coefs = flat_oracle(name)
    assert np.array_equal(coefs, inp.blocks)
    scan = sw.parse_baseline(data)[1]
    assert len(scan) == (sum(price_dc(inp.dc, inp.mcu)) + 7) // 8 + scan.count(b"\xff\x00")
    assert np.array_equal(po.decode_coefficients(data)[0], inp.blocks)


@pytest.mark.parametrize("name", FLAT)
def test_the_flat_blocks_stay_as_designed_in_every_way_they_are_encoded(name):
    """with restart intervals, and -- grey inputs with a constant chroma beside them -- with built tables"""
    inp = build_flat(name)
    for ri in (1, 7):
        assert np.array_equal(po.encode_8bit(inp.pixels, inp.luma[0], inp.luma[1], 100, want_coefficients=True, restart_interval=ri)[1], inp.blocks)
    colour = with_constant_chroma(inp)
    data, coefs = po.encode_8bit(colour.pixels, colour.luma[0], colour.luma[1], 100, want_coefficients=True, optimize_coding=True)
    assert np.array_equal(coefs, colour.blocks)
    if name == "flat_const":  # two bits a block: every workgroup base on a word edge by construction
        lengths, scan = sw.parse_baseline(data)
        assert all(t == {0: 1} for t in lengths.values()) and len(lengths) == 4 and len(scan) * 8 == 2 * len(colour.dc)
    data = po.encode_8bit(colour.pixels, colour.luma[0], colour.luma[1], 100)
    assert len(sw.parse_baseline(data)[1]) == (sum(price_dc(colour.dc, colour.mcu)) + 7) // 8 + sw.parse_baseline(data)[1].count(b"\xff\x00")


@pytest.mark.parametrize("name", FLAT)
def test_the_flat_input_reaches_the_place_it_is_named_for(name):
    check_flat_precondition(name)


def test_a_flat_block_is_eight_times_its_level_at_quality_100():
    """40 x 30 random flat blocks: DC 8 (p - 128), no AC -- what every flat input rests on"""
    values = _random_values(1200, 46)
    inp = flat_gray("probe", values, 40, 30, None)
    _, coefs = po.encode_8bit(inp.pixels, 1, 1, 100, want_coefficients=True)
    assert np.array_equal(coefs[:, 0], 8 * (values.astype(np.int64) - 128)) and not coefs[:, 1:].any()
    assert sorted(set(price_dc(inp.dc, inp.mcu))) ==[6, 11, 12, 14, 16, 18, 20, 22, 24]


def test_the_steps_of_2040_are_the_codes_the_design_counts_on():
    """0 -> 255: 111111110 11111111000 and EOB; 255 -> 0: 111111110 00000000111 and EOB"""
    inp = flat_gray("probe", [128, 0, 255, 0], 4, 1, None)
    data, _ = po.encode_8bit(inp.pixels, 1, 1, 100, want_coefficients=True)
    bits = "".join(f"{b:08b}" for b in sw.unstuff(sw.parse_baseline(data)[1]))
    assert bits.startswith("00" "1010" + "111111110" "01111111111" "1010" + "111111110" "11111111000" "1010" + "111111110" "00000000111" "1010")
