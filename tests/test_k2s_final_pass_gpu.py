"""The K2S final pass (k2s_subseq.hip: subseq_order_kernel, sf_lane_range, sf_wave, subseq_final_kernel) with TWO subsequences per lane,
and the regimes that feed it, from small batches.

The planner gives a lane two subsequences only from 2^20 subsequences in a batch on (kSubFinalFewSubs): 64 MB of DRI = 0 data, which no
test uploads.  JPGPU_SUBSEQ_TWO_PER_LANE_FROM (a test hook of the layout, read per upload) lowers that threshold, and JPGPU_SUBSEQ_SHIFT
pins the subsequence length, so a scan of a few kilobytes reaches the form the benchmark's DRI = 0 workload runs.  Every test asserts
through Batch.plan_stats() that it got there: k2s_subs_per_lane, k2s_sub_shift, k2s_subs against a count made here from the file's own
bytes, and the final pass's pools and plain list against a model of the planner's rule (_expected_lists).

No expectation comes from the decoder under test and none has a tolerance: coefficients are compared bit for bit with the oracle's
(and, for the files tests/scan_writer.py wrote, with the coefficients the writer was given, which pass through no decoder at all),
interleaved samples with the oracle's decode, and a failing file with the oracle's exception class, message and partial picture.
What a case needs of its input is asserted on the CPU in front of the upload.

What the planner counts: it cuts the bytes from the scan's first entropy byte to the END OF THE FILE (stuffed zeros and the EOI marker
included; the device unstuffs later) into subsequences of 1 << shift bits, and a DRI = 0 scan of fewer than 512 such bytes does not
take K2S at all.  So at shift 9 a K2S scan has eight subsequences or more: the counts 1, 2 and 3 exist at shift 12 only, and are
reached there.

The files scan_writer.py writes have codes of one length per table ("flat"), which never re-synchronise: the rounds advance one
subsequence at a time, the enqueued budget does not suffice and the host-checked loop takes over (subseq_fallbacks() == 1) in front of
the same final pass.  The rounds are therefore asserted only where the files have real tables (cases 4 and 8); every call's rounds and
fallbacks are printed."""
import functools
import io
import os

import numpy as np
import pytest

import jpeglibrary_amd as jl
import scan_writer as sw
import test_batch_planner_gpu as planner
import test_huffman_shapes_gpu as shapes
import test_transcode_inputs_cpu as cat
from golden_util import read_jpeg
from oracle import pyoracle as po
from tools import jpegsynth

pytestmark = pytest.mark.gpu

K2S_MIN_BYTES = 512        # a DRI = 0 scan shorter than this takes K2 as one interval (device_batch_layout.cpp: plan_entropy_work)
SF_WAVES = 4               # subseq_final_waves(): waves of 64 lanes per workgroup of the plain final pass (kernels.h)
POOL_MIN_WAVES = 40        # kSubFinalPoolMinChunks
K2S_MAX_POOLS = planner.K2S_MAX_POOLS
ORDER_KEYS = 256           # subseq_order_kernel's counting sort: a lane that owns 255 MCUs or more takes the last key
FIRST_BUDGET = 16          # kSubseqFirstBudget: rounds a first decode enqueues without the host looking
FLAT_ROUNDS_BOUND = 48     # test_reference_benchmark_gpu.py: test_flat_regions_do_not_cost_a_round_per_subsequence
SHIFTS = (9, 10, 11, 12)


# ------------------------------------------------------------------------------------------------ the regime, and a model of the planner

def _set_regime(monkeypatch, shift, spl):
    """spl = 2: two subsequences per lane from the first subsequence on; spl = 1: the switch unset (every batch here is far below 2^20)."""
    monkeypatch.delenv("JPGPU_SUBSEQ_BUDGET", raising=False)
    monkeypatch.setenv("JPGPU_SUBSEQ_SHIFT", str(shift))
    if spl == 2:
        monkeypatch.setenv("JPGPU_SUBSEQ_TWO_PER_LANE_FROM", "1")
    else:
        monkeypatch.delenv("JPGPU_SUBSEQ_TWO_PER_LANE_FROM", raising=False)


def _planned_bytes(data):
    return len(data) - planner._entropy_start(data)


def _planned_subs(data, shift):
    """subsequences the planner cuts a single-scan DRI = 0 file into (see the head of this file)"""
    n = _planned_bytes(data)
    assert n >= K2S_MIN_BYTES, n
    return -(-n * 8 // (1 << shift))


def _run_key(data):
    """what makes two consecutive scans one run of the final pass: the same Huffman tables in the same slots, the same components with
    the same sampling factors and table selectors (device_batch_layout.cpp: same_tables)"""
    segs, sos = planner._segments(data)
    sof = [p[5:] for m, p in segs if m in (0xC0, 0xC1)]
    return repr(sorted(planner._huffman_tables(data).items())), sof[0], data[sos:planner._entropy_start(data)]


def _expected_lists(files, shift, spl):
    """(pools, entries of the plain list, subsequences) of the final pass for an upload of single-scan DRI = 0 files: a run of 40 waves
    of 64 * spl subsequences or more is pooled while there are fewer than eight pools, every other scan takes one entry per SF_WAVES waves"""
    pools = plain = 0
    i = 0
    while i < len(files):
        k = i + 1
        while k < len(files) and _run_key(files[k]) == _run_key(files[i]):
            k += 1
        subs = [_planned_subs(f, shift) for f in files[i:k]]
        if sum(-(-n // (64 * spl)) for n in subs) >= POOL_MIN_WAVES and pools < K2S_MAX_POOLS:
            pools += 1
        else:
            plain += sum(-(-n // (64 * spl * SF_WAVES)) for n in subs)
        i = k
    return pools, plain, sum(_planned_subs(f, shift) for f in files)


def _assert_regime(st, files, shift, spl):
    pools, plain, subs = _expected_lists(files, shift, spl)
    want = {"k2s_scans": len(files), "k2s_subs_per_lane": spl, "k2s_sub_shift": shift, "k2s_subs": subs, "k2s_pools": pools, "k2s_plain_work": plain,
            "k2s_table_sets": len({_run_key(f) for f in files})}
    assert {k: st[k] for k in want} == want, (st, want)
    return want


# ------------------------------------------------------------------------------------------------ references and the comparison

@functools.lru_cache(maxsize=None)
def _ref(data):
    return planner._Ref(data)


class _CoefficientsOnly:
    """the reference of a file whose samples INTERLEAVED_U8 does not hold (12-bit): the oracle's coefficients"""
    def __init__(self, data):
        self.kind, self.msg, self.px, self.coefs = "OK", "", None, po.decode_coefficients(data)[0]


def _coefficients(b, refs, written, what):
    for i, r in enumerate(refs):
        res = b.result(i)
        assert planner.NAMES[res.status] == r.kind, (what, i, r.kind, r.msg, res.status, res.detail)
        if r.coefs is None:
            continue
        c = b.coefficients(i)
        assert c.shape == r.coefs.shape and np.array_equal(c, r.coefs), (what, i, "oracle", int((c != r.coefs).any(axis=1).sum()))
        if written[i] is not None:
            assert np.array_equal(c, written[i]), (what, i, "writer", int((c != written[i]).any(axis=1).sum()))


def _decode_and_compare(files, shift, spl, written=None, pixels=True, what="", refs=None):
    """One PLANAR_I16 upload through run_entropy() (coefficients against the oracle and the writer) and one INTERLEAVED_U8 decode()
    (samples, and status class, message and partial picture of a failing file, against the oracle).  Returns the asserted plan_stats
    values and the (rounds, fallbacks) of the two."""
    files = list(files)
    written = list(written) if written is not None else [None] * len(files)
    refs = refs if refs is not None else [_ref(f) for f in files]
    b = jl.Batch().upload(files, jl.FMT_PLANAR_I16)
    try:
        regime = _assert_regime(b.plan_stats(), files, shift, spl)
        b.run_entropy().sync()
        _coefficients(b, refs, written, (what, shift, spl))
        calls = [(b.subseq_rounds(), b.subseq_fallbacks())]
    finally:
        b.close()
    if pixels:
        b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8)
        try:
            _assert_regime(b.plan_stats(), files, shift, spl)
            b.decode().sync()
            planner._check(b, refs, (what, shift, spl), coefs=False)
            calls.append((b.subseq_rounds(), b.subseq_fallbacks()))
        finally:
            b.close()
    print(what, regime, "rounds, fallbacks:", calls)
    return regime, calls


# ------------------------------------------------------------------------------------------------ 1. sampling classes

def _write(coefs, bw, bh, ncomp=1, shape="flat"):
    data, info = sw.write_baseline(coefs, bw * 8, bh * 8, ncomp, 0, shape)
    return data, np.asarray(coefs, np.int16), info


@functools.lru_cache(maxsize=None)
def _sampling_class_files():
    """(blocks per MCU, file, the coefficients its writer was given or None) for 1, 3, 4, 6, four components at 1 x 1, and 13"""
    gray_written = cat.build("subs_le_256")
    color_written = _write(cat._ff_color(11, 9, 3), 11, 9, ncomp=3)
    rows = [(1, jpegsynth.encode(168, 120, "gray", 90, 0, seed=31), None),
            (1, gray_written.data, gray_written.coefs),
            (3, jpegsynth.encode(152, 120, "444", 90, 0, seed=32), None),
            (3, color_written[0], color_written[1]),
            (4, jpegsynth.encode(176, 104, "422", 90, 0, seed=33), None),
            (6, jpegsynth.encode(184, 136, "420", 90, 0, seed=34), None),
            (4, planner._cmyk(96, 96, seed=11), None),
            (13, cat.build("sampling_4x2_2x2_1x1_129x65_dri0").data, None)]
    for bpm, f, _ in rows:
        segs, sos = planner._segments(f)
        sof = [p for m, p in segs if m in (0xC0, 0xC1)][0]
        assert (1 if sof[5] == 1 else sum((sof[7 + 3 * c] >> 4) * (sof[7 + 3 * c] & 15) for c in range(sof[5]))) == bpm, bpm
        assert f[sos + 4] == sof[5] and not any(m == 0xDD for m, _ in segs)  # (one interleaved scan, no restart interval)
        assert _planned_subs(f, 12) >= 3, (bpm, _planned_bytes(f))  # (at the longest subsequence still a lane of two and a lane of one, or more)
    assert rows[6][1][planner._segments(rows[6][1])[1] + 4] == 4  # (Ns of the CMYK file's scan)
    return rows


@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("shift", SHIFTS)
def test_every_sampling_class_at_every_subsequence_length(shift, spl, monkeypatch):
    """Blocks per MCU of 1, 3, 4, 6, 4 (four components) and 13 in one upload: where a lane's first MCU starts (skip), the block it stands
    at and the DC chains of up to four components.  Shift 12 is the only one with the round kernel's warm start (2048 < 1 << shift)."""
    rows = _sampling_class_files()
    _set_regime(monkeypatch, shift, spl)
    regime, _ = _decode_and_compare([f for _, f, _ in rows], shift, spl, [w for _, _, w in rows], what="sampling classes")
    assert regime["k2s_pools"] == 0 and regime["k2s_plain_work"] >= len(rows)


# ------------------------------------------------------------------------------------------------ 2. counts around the unit edges

COLUMN_MAX_BLOCKS = 8191  # (a frame is at most 65 535 lines high)


@functools.lru_cache(maxsize=None)
def _column_with_subs(count, shift):
    """A gray file one block wide (about 20 bytes of scan per block, flat tables) that the planner cuts into exactly `count`
    subsequences: a search over the seed and the height, the height stepped by what the last try missed the window by."""
    lo, hi = max(K2S_MIN_BYTES, ((count - 1) << shift) // 8 + 1), (count << shift) // 8
    assert lo <= hi, (count, shift, "no K2S scan has this count: 512 bytes are %d subsequences" % (K2S_MIN_BYTES * 8 >> shift))
    tried = 0
    for seed in range(64):
        coefs = cat._dense(1, COLUMN_MAX_BLOCKS, 500 + seed, 1, 6, 12)
        k = max(1, (lo + hi) // 2 // 20)
        for _ in range(12):
            data, written, info = _write(coefs[:k], 1, k)
            n = len(data) - info["header_bytes"]
            tried += 1
            if lo <= n <= hi:
                # the planner's count from what the writer knows: data bytes, stuffed zeros, EOI
                assert n == sw.unstuffed_length(info) + info["stuffed"] + 2 == _planned_bytes(data)
                return data, written, info
            step = int(round(((lo + hi) / 2 - n) / 20))
            k = min(COLUMN_MAX_BLOCKS, max(1, k + (step if step else (1 if n < lo else -1))))
    raise AssertionError(f"no column of {count} subsequences at shift {shift} in {tried} tries")


# (shift, count): the last lane with one subsequence (odd counts), one lane in all (1, 2), a wave with one live lane (129 and 257: lanes
# 64 and 128), the rounds' workgroup of 256, the gather / order group of 1024 (1023, 1025, 2049).  1, 2, 3: see the head of this file.
UNIT_EDGES = [(12, 1), (12, 2), (12, 3), (9, 8), (9, 9), (9, 127), (9, 128), (9, 129), (9, 255), (9, 257), (9, 1023), (9, 1025), (9, 2049)]


@pytest.mark.parametrize("shift,count", UNIT_EDGES)
def test_subsequence_counts_around_the_unit_edges(shift, count, monkeypatch):
    data, written, info = _column_with_subs(count, shift)
    assert _planned_subs(data, shift) == count
    _set_regime(monkeypatch, shift, 2)
    regime, _ = _decode_and_compare([data], shift, 2, [written], what=f"{count} subsequences")
    assert regime["k2s_subs"] == count and regime["k2s_subs_per_lane"] == 2
    assert regime["k2s_pools"] == 0 and regime["k2s_plain_work"] == -(-count // (128 * SF_WAVES))


# ------------------------------------------------------------------------------------------------ 3. lanes that own nothing

def _inside_a_block(info, shift):
    """per subsequence of 1 << shift bits: it lies wholly inside one block (no block starts in it)"""
    edges = np.array(info["block_bits"] + [sw.unstuffed_length(info) * 8])
    span = 1 << shift
    lo = np.arange(-(-int(edges[-1]) // span)) * span
    return (np.searchsorted(edges[:-1], lo, "left") == np.searchsorted(edges[:-1], lo + span, "left")) & (lo + span <= edges[-1])


@functools.lru_cache(maxsize=None)
def _long_block_files():
    color = _write(cat._dense(7, 5 * 3, 12, 8, 10), 7, 5, ncomp=3)
    return color


@pytest.mark.parametrize("spl", [1, 2])
def test_lanes_whose_subsequences_lie_inside_one_block(spl, monkeypatch):
    """Blocks of more than 1000 bits at 512-bit subsequences: lanes that own nothing, several in a row, and with two per lane a lane
    whose two subsequences both lie inside one block -- gray, and three components (a lane that starts in the middle of an MCU and owns
    none).  A quality-100 noise file (blocks of its own lengths) rides along."""
    cat.check_precondition("long_blocks")  # (ten or more such subsequences, two in a row somewhere)
    gray = cat.build("long_blocks")
    color_data, color_coefs, color_info = _long_block_files()
    for info in (gray.info, color_info):
        inside = _inside_a_block(info, 9)
        pairs = inside[0:len(inside) // 2 * 2:2] & inside[1::2]  # (lane k of two-per-lane takes subsequences 2k and 2k + 1)
        assert inside.sum() >= 10 and pairs.sum() >= 2 and (inside[1:] & inside[:-1]).any(), (int(inside.sum()), int(pairs.sum()))
    noise = jpegsynth.encode(96, 80, "444", 100, 0, seed=41)
    _set_regime(monkeypatch, 9, spl)
    # (the written files' codes all have one length per table: nothing re-synchronises, the rounds advance a subsequence at a time and the
    # host-checked loop takes over -- subseq_fallbacks() == 1 is the expected path to the final pass here)
    _decode_and_compare([gray.data, color_data, noise], 9, spl, [gray.coefs, color_coefs, None], what="long blocks")


# ------------------------------------------------------------------------------------------------ 4. the order kernel's key clamp

@functools.lru_cache(maxsize=None)
def _flat_canvas(optimize):
    from PIL import Image

    rng = np.random.default_rng(7)
    px = np.full((1536, 2048), 200, np.uint8)
    px[:64, :320] = rng.integers(0, 256, (64, 320), dtype=np.uint8)            # content, then a long flat stretch
    px[696:760, 896:1496] = rng.integers(0, 256, (64, 600), dtype=np.uint8)    # an island inside the flat region
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="JPEG", quality=75, optimize=optimize)
    return buf.getvalue(), (1536 - 760) // 8 * (2048 // 8)  # (the MCUs behind the island's last row: all flat)


@pytest.mark.parametrize("optimize", [False, True])
def test_lanes_that_own_more_mcus_than_the_order_kernel_has_keys(optimize, monkeypatch):
    """A flat gray canvas with an island of content at shift 12, two per lane: a flat MCU is the DC code of a zero difference and the
    EOB code, so a lane of 8192 bits owns far more than 255 MCUs and takes the order kernel's last key with all its kind; the twin
    subsequences of the flat stretch arm the rounds' flat-region walk, which keeps the rounds bounded."""
    data, flat_tail_mcus = _flat_canvas(optimize)
    lengths, scan = sw.parse_baseline(data)
    mcu_bits = lengths[(0, 0)][0] + lengths[(1, 0)][0x00]
    lane_bits = 2 << 12
    assert lane_bits // mcu_bits > ORDER_KEYS - 1, mcu_bits
    assert flat_tail_mcus * mcu_bits >= 4 * lane_bits  # (three or more lanes lie wholly in the flat stretch behind the island)
    # ... and the file really ends so: the tail repeats with the period of the flat MCU
    period = mcu_bits // np.gcd(mcu_bits, 8)
    tail = sw.unstuff(scan)[-(3 * lane_bits // 8) - 8:-8]
    assert tail[period:] == tail[:-period] and len(tail) == 3 * lane_bits // 8
    _set_regime(monkeypatch, 12, 2)
    _, calls = _decode_and_compare([data], 12, 2, what=f"flat canvas, optimize={optimize}")
    assert all(2 <= rounds <= FLAT_ROUNDS_BOUND for rounds, _ in calls), calls


# ------------------------------------------------------------------------------------------------ 5. tables

@functools.lru_cache(maxsize=None)
def _table_files():
    optimized = planner._optimized(jpegsynth.encode(200, 152, "420", 90, 0, seed=51))
    deep = cat.build("codes16_default")  # written with the "deep" shape: every rare symbol a code of 16 bits
    wide, wide_coefs = shapes._recode(shapes._image(168, 136, 5), (2, 2), 92, 0, "wide", "deep")
    twelve = read_jpeg("testorig12.jpg")
    return optimized, deep, wide, wide_coefs, twelve


@functools.lru_cache(maxsize=None)
def _twelve_bit_ref():
    return _CoefficientsOnly(read_jpeg("testorig12.jpg"))


@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("shift", [9, 12])
def test_tables_of_other_shapes_than_the_standard_ones(shift, spl, monkeypatch):
    """Tables the oracle's optimizer built for one file; tables with codes longer than the round kernel's 10-bit lookup decides (16
    bits, gray and 4:2:0, the latter with short codes for the large DC categories); and the 12-bit SOF1 file (coefficients only: its
    samples do not fit INTERLEAVED_U8)."""
    optimized, deep, wide, wide_coefs, twelve = _table_files()
    assert planner._huffman_tables(optimized) != planner._huffman_tables(jpegsynth.encode(200, 152, "420", 90, 0, seed=51))
    for f in (deep.data, wide):
        assert max(max(t.values()) for t in sw.parse_baseline(f)[0].values()) == 16 > 10
    segs = planner._segments(twelve)[0]
    assert [p[0] for m, p in segs if m == 0xC1] == [12] and not any(m == 0xDD for m, _ in segs)
    _set_regime(monkeypatch, shift, spl)
    _decode_and_compare([optimized, deep.data, wide], shift, spl, [None, deep.coefs, wide_coefs.reshape(-1, 64)], what="tables")
    # the 12-bit file: coefficients against the oracle's, through K2S (k2s_scans == 1 is part of the regime)
    _decode_and_compare([twelve], shift, spl, pixels=False, what="testorig12", refs=[_twelve_bit_ref()])


# ------------------------------------------------------------------------------------------------ 6. failures

FAIL_BASE = "subs_gt_3072"  # a written gray file of 3 316 subsequences at shift 9 (flat tables of its own)


@functools.lru_cache(maxsize=None)
def _truncated_with_parity(shift, parity):
    """FAIL_BASE cut inside a code word so that the subsequence (of 1 << shift bits) the data ends in is even / odd: with two per lane the
    first / the second subsequence of its lane.  Returns (file, that subsequence)."""
    for min_sub in range(1500, 1600):
        data, sub9 = cat.truncated(FAIL_BASE, "code", min_sub=min_sub)
        sub = sub9 >> (shift - 9)
        if sub % 2 == parity:
            return data, sub
    raise AssertionError("no such cut")


def _pool_mates(good, shift):
    """copies of `good` that make a pooled run with two per lane on their own (so the run stays pooled whatever joins it)"""
    waves_each = -(-_planned_subs(good, shift) // 128)
    return [good] * -(-POOL_MIN_WAVES // waves_each)


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("kind", ["even", "odd", "late"])
@pytest.mark.parametrize("shift", [9, 12])
def test_a_failing_scan_alone_and_inside_a_pooled_run(shift, kind, pooled, monkeypatch):
    """open_end is ORed over a lane's two exit states: a stream that ends in the lane's first subsequence and one that ends in its second;
    and a lane that owns MCUs but starts behind the data (stress/dri0_invalid_code_late.jpg).  Each alone (the plain list) and in the
    middle of a pooled run of good files with its tables, which stay exact.  All three files fail by design in today's suite.
    (A cut file's data ENDS in the failing subsequence, so that one is the last or the last but one the planner counts: what differs
    between the two cuts is whether the lane that reports the failure holds one more subsequence in front of it or behind it.)"""
    if kind == "late":
        bad = read_jpeg(os.path.join("stress", "dri0_invalid_code_late.jpg"))
        good = jpegsynth.encode(768, 640, "444", 90, 0, seed=14)
        written = None
    else:
        bad, sub = _truncated_with_parity(shift, kind == "odd")
        base = cat.build(FAIL_BASE)
        good, written = base.data, base.coefs
        assert sub % 2 == (kind == "odd") and 0 < sub < _planned_subs(bad, shift)
        assert bad[:base.info["header_bytes"]] == good[:base.info["header_bytes"]]
    assert _run_key(bad) == _run_key(good)
    ref = _ref(bad)
    assert ref.kind == "InvalidDataException" and ref.px.any(), (ref.kind, ref.msg)  # (fails on the device, behind decoded MCUs)
    if pooled:
        mates = _pool_mates(good, shift)
        files = mates[:len(mates) // 2] + [bad] + mates[len(mates) // 2:] + [bad]
    else:
        files = [bad]
    _set_regime(monkeypatch, shift, 2)
    regime, _ = _decode_and_compare(files, shift, 2, [written if f is good else None for f in files], what=f"failing: {kind}")
    assert (regime["k2s_pools"], regime["k2s_plain_work"] == 0) == ((1, True) if pooled else (0, False)), regime


# ------------------------------------------------------------------------------------------------ 7. the work lists

@functools.lru_cache(maxsize=None)
def _list_files():
    a = jpegsynth.encode(1280, 960, "420", 90, 0, seed=71)     # a pooled run on its own at shift 9, two per lane
    b = jpegsynth.encode(896, 736, "444", 90, 0, seed=72)      # the same tables, another sampling: a run of its own
    short = jpegsynth.encode(320, 240, "422", 90, 0, seed=73)  # too short to pool
    own = planner._optimized(jpegsynth.encode(320, 240, "420", 90, 0, seed=74))  # tables of its own
    return a, b, short, own


def test_pooled_plain_and_overflowing_runs_in_one_upload(monkeypatch):
    """One upload with two per lane: a run too short to pool, eight pooled runs, a file with tables of its own between them, and a ninth
    poolable run, which takes the plain list (entries of 64 * 2 * SF_WAVES subsequences) because the pools are used up."""
    a, b, short, own = _list_files()
    files = [short, a, b, a, b, own, a, b, a, b, a]
    assert planner._huffman_tables(a) == planner._huffman_tables(b) == planner._huffman_tables(short) != planner._huffman_tables(own)
    for f in (a, b):
        assert -(-_planned_subs(f, 9) // 128) >= POOL_MIN_WAVES > -(-_planned_subs(short, 9) // 128)
    poolable = sum(f is a or f is b for f in files)
    assert poolable == K2S_MAX_POOLS + 1
    pools, plain, _ = _expected_lists(files, 9, 2)
    assert pools == K2S_MAX_POOLS and plain == sum(-(-_planned_subs(f, 9) // (128 * SF_WAVES)) for f in (short, own, a))
    _set_regime(monkeypatch, 9, 2)
    regime, _ = _decode_and_compare(files, 9, 2, what="lists")
    assert regime["k2s_pools"] == K2S_MAX_POOLS and regime["k2s_plain_work"] == plain
    assert regime["k2s_table_sets"] == 4  # (the standard tables under three samplings, and the file's own)


# ------------------------------------------------------------------------------------------------ 8. repeated and staged calls

def test_repeated_and_staged_calls_with_two_per_lane(monkeypatch):
    """decode().decode().sync(), a third decode with the learned budget, a fresh upload whose budget cannot suffice (host-checked rounds
    in front of the same final pass) and run_entropy().run_idct() without a sync between: the same, exact, results.  The coefficients
    are overwritten with noise between the calls, so a final pass that drew no work shows."""
    a, _, short, own = _list_files()
    files = [a, short, own]
    refs = [_ref(f) for f in files]
    rng = np.random.default_rng(8)
    _set_regime(monkeypatch, 9, 2)
    b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8)
    regime = _assert_regime(b.plan_stats(), files, 9, 2)
    assert regime["k2s_pools"] == 1 and regime["k2s_plain_work"] > 0
    b.decode().decode().sync()
    rounds = b.subseq_rounds()
    assert 2 <= rounds <= FIRST_BUDGET and b.subseq_fallbacks() == 0, (rounds, b.subseq_fallbacks())
    planner._check(b, refs, "decode x2")
    planner._poison(b, refs, rng)
    b.decode().sync()  # the learned budget: exactly `rounds` rounds
    assert b.subseq_rounds() == rounds and b.subseq_fallbacks() == 0
    planner._check(b, refs, "third decode")
    planner._poison(b, refs, rng)
    b.run_entropy().run_idct().sync()
    assert b.subseq_fallbacks() == 0
    planner._check(b, refs, "run_entropy, run_idct")
    b.close()
    monkeypatch.setenv("JPGPU_SUBSEQ_BUDGET", "2")
    b2 = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8)
    assert _assert_regime(b2.plan_stats(), files, 9, 2) == regime
    b2.decode().sync()
    assert b2.subseq_fallbacks() == 1 and b2.subseq_rounds() >= rounds, (b2.subseq_fallbacks(), b2.subseq_rounds(), rounds)
    planner._check(b2, refs, "budget 2")
    planner._poison(b2, refs, rng)
    b2.run_entropy().run_idct().sync()
    assert b2.subseq_fallbacks() == 1
    planner._check(b2, refs, "budget 2: run_entropy, run_idct")
    b2.close()
    print("calls", regime, "rounds:", rounds)


# ------------------------------------------------------------------------------------------------ 9. the switch itself

def test_the_switch_unset_changes_nothing_and_its_value_is_a_threshold(monkeypatch):
    """Unset, a small batch takes one subsequence per lane at the planner's own shift.  Set, the value is the batch's subsequence count
    from which a lane takes two: the count itself gives two, one more gives one, 1 always two."""
    files = [f for _, f, _ in _sampling_class_files()][:4]
    refs = [_ref(f) for f in files]
    for name in ("JPGPU_SUBSEQ_SHIFT", "JPGPU_SUBSEQ_TWO_PER_LANE_FROM", "JPGPU_SUBSEQ_BUDGET"):
        monkeypatch.delenv(name, raising=False)
    # (under 4096 subsequences of 1024 bits the planner's own choice is 512 bits: choose_batch_shapes)
    assert sum(map(len, files)) * 8 < 4096 << 10
    b = jl.Batch().upload(files)
    st = _assert_regime(b.plan_stats(), files, 9, 1)
    for value, spl in ((st["k2s_subs"], 2), (st["k2s_subs"] + 1, 1), (1, 2), (1 << 20, 1)):
        monkeypatch.setenv("JPGPU_SUBSEQ_TWO_PER_LANE_FROM", str(value))
        b.upload(files)
        _assert_regime(b.plan_stats(), files, 9, spl)
        b.decode().sync()
        planner._check(b, refs, ("threshold", value))
    b.close()
    b = jl.Batch().upload([jpegsynth.encode(64, 64, "420", 75, 4, seed=1)])  # no K2S scan: the fields read zero
    st = b.plan_stats()
    assert (st["k2s_scans"], st["k2s_sub_shift"], st["k2s_subs"]) == (0, 0, 0), st
    b.close()
