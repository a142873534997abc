"""The entropy-stage planner between the parser and the kernels (device_batch_layout.cpp): K2's pooled runs of restart-interval
scans, the K2S final pass's pools and table sets, and what repeated and staged calls on one upload do with them.

Every image is checked against the oracle (coefficients, interleaved u8 samples, the status class of a failing file), and every
test asserts through Batch.plan_stats() that the batch took the branch the test is named for.  The inputs are made at test time
with fixed seeds by jpegsynth, Pillow (its own optimised tables) and the oracle's optimizer (per-image tables)."""
import io
import os

import numpy as np
import pytest

import jpeglibrary_amd as jl
from golden_util import middle_scan_swallow_files
from jpeglibrary_amd import _capi
from oracle import pyoracle as po
from tools import jpegsynth

pytestmark = pytest.mark.gpu

NAMES = {0: "OK", 1: "InvalidDataException", 2: "InvalidOperationException", 3: "NotSupportedException", 4: "ArgumentException"}
K2_CHUNK = 64              # restart intervals per pooled K2 entry (device_batch_layout.cpp)
K2_MAX_POOLS = 8           # kK2MaxPools
K2S_MAX_POOLS = 8          # kSubFinalMaxPools
FULL_WAVES = 11            # huffman_waves() of a batch whose largest table set is the standard four tables


# ------------------------------------------------------------------------------------------------ inputs

def _segments(data):
    """(marker, payload) of every segment in front of the first SOS, and the SOS's offset."""
    segs, i = [], 2
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        if m == 0xDA:
            return segs, i
        n = int.from_bytes(data[i + 2:i + 4], "big")
        segs.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n


def _huffman_tables(data):
    """{(class, id): (counts, values)} of the DHT segments in front of the first scan."""
    tabs = {}
    for m, p in _segments(data)[0]:
        if m != 0xC4:
            continue
        k = 0
        while k < len(p):
            counts = p[k + 1:k + 17]
            nv = sum(counts)
            tabs[(p[k] >> 4, p[k] & 15)] = (bytes(counts), bytes(p[k + 17:k + 17 + nv]))
            k += 17 + nv
    return tabs


def _intervals(data):
    """Restart intervals of the (single, interleaved) scan of a baseline file; 0 without DRI."""
    dri, w, h, comps = 0, 0, 0, []
    for m, p in _segments(data)[0]:
        if m == 0xDD:
            dri = int.from_bytes(p[0:2], "big")
        elif m in (0xC0, 0xC1):
            h, w = int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big")
            comps = [(p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15) for c in range(p[5])]
    if dri == 0:
        return 0
    if len(comps) == 1:
        mcus = -(-w // 8) * -(-h // 8)
    else:
        hm, vm = max(c[0] for c in comps), max(c[1] for c in comps)
        mcus = -(-w // (8 * hm)) * -(-h // (8 * vm))
    return -(-mcus // dri)


def _chunks(data):
    return -(-_intervals(data) // K2_CHUNK)


def _synth(w, h, ss="420", q=75, dri=1, seed=0):
    return bytes(jpegsynth.encode(w, h, ss, q, dri, seed=seed))


def _pillow(w, h, subsampling=2, q=80, blocks=1, seed=0):
    """libjpeg-turbo through Pillow with optimize=True: Huffman tables of this image's own."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    img = Image.fromarray(rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)).resize((w, h), Image.BILINEAR)
    buf = io.BytesIO()
    kw = dict(quality=q, subsampling=subsampling, optimize=True)
    if blocks:
        kw["restart_marker_blocks"] = blocks
    img.save(buf, "JPEG", **kw)
    return buf.getvalue()


def _optimized(data):
    """The oracle's optimizer: the same scan with Huffman tables built for this file alone."""
    out = po.optimize(data, False)
    assert _intervals(out) == _intervals(data)
    return out


def _extra_slots(data):
    """The third component of a 3-component scan decoded with copies of tables 1 defined as tables 2 (a second DHT in front of the
    SOS): the scan stages six tables instead of four (k2_scan_tab_bytes), so this file alone lowers the batch's waves per K2
    workgroup and leaves no room for the pooled K2S final pass."""
    tabs = _huffman_tables(data)
    payload = b"".join(bytes([(tc << 4) | 2]) + tabs[(tc, 1)][0] + tabs[(tc, 1)][1] for tc in (0, 1))
    sos = _segments(data)[1]
    scan = bytearray(data[sos:])
    assert scan[4] == 3 and scan[10] == 0x11  # (Ns; the third component's Td / Ta)
    scan[10] = 0x22
    return data[:sos] + b"\xff\xc4" + (len(payload) + 2).to_bytes(2, "big") + payload + bytes(scan)


def _entropy_start(data):
    sos = _segments(data)[1]
    return sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")


def _cut(data, frac=0.55):
    """Cut inside the entropy data, EOI behind it: Identify passes, the scan fails on the device."""
    e0 = _entropy_start(data)
    at = e0 + int((len(data) - e0) * frac)
    while data[at - 1] == 0xFF:
        at -= 1
    return data[:at] + b"\xff\xd9"


def _flip(data, frac=0.4):
    """One entropy byte changed (no 0xFF made or broken)."""
    e0 = _entropy_start(data)
    at = e0 + int((len(data) - e0) * frac)
    while data[at] == 0xFF or data[at - 1] == 0xFF or data[at] ^ 0x5A == 0xFF:
        at += 1
    return data[:at] + bytes([data[at] ^ 0x5A]) + data[at + 1:]


# ------------------------------------------------------------------------------------------------ checks

class _Ref:
    def __init__(self, data):
        self.px, _, err = po.decode_8bit_partial(data)
        self.kind = "OK" if err is None else err.kind
        self.msg = "" if err is None else err.message
        self.coefs = po.decode_coefficients(data)[0] if err is None else None


def _refs(files):
    return [_Ref(f) for f in files]


def _check(b, refs, what="", pixels=True, coefs=True):
    for i, r in enumerate(refs):
        res = b.result(i)
        assert NAMES[res.status] == r.kind, (what, i, r.kind, r.msg, res.status, res.detail)
        if res.detail in (1, 2, 3, 4):  # device-reported failures carry the reference's text
            assert _capi.lib.jpgpu_detail_string(res.detail).decode() == r.msg, (what, i, r.msg, res.detail)
        if pixels:
            out = np.asarray(b.output(i))
            assert out.shape == r.px.shape and np.array_equal(out, r.px), (what, i, r.kind, int((out != r.px).sum()))
        if coefs and r.coefs is not None:
            c = b.coefficients(i)
            assert c.shape == r.coefs.shape and np.array_equal(c, r.coefs), (what, i, int((c != r.coefs).sum()))


def _decode(files, refs=None, **kw):
    refs = refs if refs is not None else _refs(files)
    b = jl.Batch().upload(files).decode().sync()
    _check(b, refs, **kw)
    return b, b.plan_stats(), refs


def _poison(b, refs, rng):
    for i, r in enumerate(refs):
        if r.kind == "OK":
            n = b.image_info(i).total_blocks
            b.set_coefficients(i, rng.integers(-1024, 1024, size=(n, 64), dtype=np.int16))


def _plain_entries(files, waves):
    """K2's plain list for restart-interval scans that do not pool: one entry per 64 * waves intervals."""
    return sum(-(-_intervals(f) // (K2_CHUNK * waves)) for f in files)


# ------------------------------------------------------------------------------------------------ K2 (DRI > 0)

def _separator(seed):
    """A one-chunk gray scan: tables and geometry of its own, never pooled -- it ends the run in front of it."""
    return _synth(64, 64, "gray", 75, 2, seed=seed)


def test_k2_pool_thresholds():
    """64 intervals (one chunk) stay on the plain list, 65 (two chunks) are pooled; a run of fewer chunks than one workgroup has
    waves, and one whose chunk count is no multiple of them, are pooled and exact."""
    one = _synth(128, 128, seed=1)         # 8 x 8 MCUs, DRI 1: 64 intervals
    two = _synth(208, 80, seed=2)          # 13 x 5: 65 intervals
    few = _synth(320, 256, seed=3)         # 320 intervals: 5 chunks, below one workgroup
    odd = _synth(736, 512, seed=4)         # 1472 intervals: 23 chunks
    assert [_intervals(f) for f in (one, two, few, odd)] == [64, 65, 320, 1472]
    files = [one, _separator(10), two, _separator(11), few, _separator(12), odd]
    b, st, _ = _decode(files)
    assert st["huffman_waves"] == FULL_WAVES
    assert 5 < FULL_WAVES and 23 % FULL_WAVES != 0
    assert st["k2_pools"] == 3 and st["k2_pooled_chunks"] == 2 + 5 + 23, st
    assert st["k2_plain_work"] == _plain_entries([one] + files[1::2], FULL_WAVES), st
    b.close()


def _alternating_runs(n, seed0):
    """n single-file runs, each pool-eligible, alternating standard tables (jpegsynth) and Pillow-optimised tables."""
    files = []
    for k in range(n):
        w, h = 160 + 32 * (k % 4), 128 + 16 * (k % 3)
        files.append(_synth(w, h, "420", 75, 1, seed=seed0 + k) if k % 2 == 0 else _pillow(w, h, 2, 80, 1, seed=seed0 + k))
        assert _chunks(files[-1]) >= 2
    for a, c in zip(files, files[1:]):
        assert _huffman_tables(a) != _huffman_tables(c)
    return files


def test_k2_more_than_eight_runs_alternating_tables():
    files = _alternating_runs(12, 100)
    b, st, _ = _decode(files)
    assert st["k2_pools"] == K2_MAX_POOLS, st
    assert st["k2_pooled_chunks"] == sum(_chunks(f) for f in files[:K2_MAX_POOLS]), st
    assert st["k2_plain_work"] == _plain_entries(files[K2_MAX_POOLS:], st["huffman_waves"]), st
    b.close()


def test_k2_scans_split_over_several_entries_pooled_and_plain():
    """1024 x 768 4:2:0 DRI 1 (3072 intervals, more than one workgroup's 64 * waves) inside a pool, and again past the 8th pool."""
    big_std = _synth(1024, 768, "420", 75, 1, seed=200)
    big_pil = _pillow(1024, 768, 2, 80, 1, seed=201)
    assert _intervals(big_std) == _intervals(big_pil) == 3072 > K2_CHUNK * FULL_WAVES
    files = [big_std] + _alternating_runs(8, 210)[1:] + [big_pil]
    for a, c in zip(files, files[1:]):
        assert _huffman_tables(a) != _huffman_tables(c)
    b, st, _ = _decode(files)
    assert st["k2_pools"] == K2_MAX_POOLS, st
    assert st["k2_pooled_chunks"] == sum(_chunks(f) for f in files[:K2_MAX_POOLS]), st
    assert st["k2_plain_work"] == _plain_entries([big_pil], st["huffman_waves"]) >= 2, st
    b.close()


def test_k2_same_tables_different_geometry_are_not_pooled_together():
    files = [_synth(256, 128, "420", 75, 1, seed=300), _synth(256, 128, "422", 75, 1, seed=301), _synth(128, 128, "444", 75, 1, seed=302),
             _synth(128, 128, "gray", 75, 1, seed=303), _synth(256, 128, "420", 75, 1, seed=304)]
    assert [_chunks(f) for f in files] == [2, 4, 4, 4, 2]
    assert _huffman_tables(files[0]) == _huffman_tables(files[1]) == _huffman_tables(files[2])
    b, st, _ = _decode(files)
    assert st["k2_pools"] == 5 and st["k2_pooled_chunks"] == 16 and st["k2_plain_work"] == 0, st
    b.close()


def test_k2_every_image_with_tables_of_its_own():
    files = []
    for k in range(6):
        # (a DRI that divides the MCU count makes the reference's optimizer give up: 325 MCUs, DRI 3)
        files.append(_optimized(_synth(400, 208, "420", 85, 3, seed=400 + k)) if k % 2 == 0 else _pillow(224, 144, 1, 85, 2, seed=400 + k))
    for a, c in zip(files, files[1:]):
        assert _huffman_tables(a) != _huffman_tables(c)
    b, st, _ = _decode(files)
    assert st["k2_pools"] == 6 and st["k2_pooled_chunks"] == sum(_chunks(f) for f in files), st
    b.close()


def test_k2_failures_inside_a_pool():
    """A cut scan (EOI behind it) and one with a changed entropy byte in the middle of pooled runs: neighbours exact, status of the oracle."""
    g = [_synth(320, 256, "420", 75, 2, seed=500 + k) for k in range(6)]
    cut, flip = _cut(_synth(320, 256, "420", 75, 2, seed=510)), _flip(_synth(320, 256, "420", 75, 2, seed=511))
    files = [g[0], cut, g[1], g[2], _separator(512), g[3], flip, g[4], g[5]]
    refs = _refs(files)
    assert refs[1].kind != "OK"
    b, st, _ = _decode(files, refs)
    assert st["k2_pools"] == 2 and st["k2_pooled_chunks"] == 8 * _chunks(g[0]), st
    b.close()


def test_k2_order_of_the_files_does_not_change_their_outputs():
    files = _alternating_runs(12, 600)
    refs = _refs(files)
    orders = {"given": list(range(12)), "sorted": sorted(range(12), key=lambda i: files[i]),
              "alternating": list(range(0, 12, 2)) + list(range(1, 12, 2)), "reversed": list(range(11, -1, -1))}
    outs = {}
    for name, order in orders.items():
        b = jl.Batch().upload([files[i] for i in order]).decode().sync()
        _check(b, [refs[i] for i in order], name)
        for pos, i in enumerate(order):
            outs.setdefault(i, []).append((np.asarray(b.output(pos)).copy(), b.coefficients(pos)))
        b.close()
    for i, got in outs.items():
        for px, co in got[1:]:
            assert np.array_equal(px, got[0][0]) and np.array_equal(co, got[0][1]), i


def test_k2_file_with_more_table_slots_lowers_the_waves_of_the_batch():
    files = _alternating_runs(4, 700) + [_separator(710), _synth(1024, 768, "420", 75, 1, seed=711)]
    _, st, _ = _decode(files)
    assert st["huffman_waves"] == FULL_WAVES and st["k2_pools"] == 5, st
    extra = _extra_slots(_synth(256, 192, "420", 75, 1, seed=712))
    assert set(_huffman_tables(extra)) == {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)}
    files2 = files[:2] + [extra] + files[2:]
    b, st2, refs = _decode(files2)
    assert refs[2].kind == "OK"
    assert st2["huffman_waves"] < FULL_WAVES and st2["k2_pools"] == 6, st2
    assert st2["k2_plain_work"] == _plain_entries([files[4]], st2["huffman_waves"]), st2
    b.close()


def _cmyk(w, h, q=90, blocks=0, seed=0):
    """Pillow, CMYK noise: ONE interleaved scan of FOUR components at 1 x 1 (the fourth DC predictor) with the standard tables."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    buf = io.BytesIO()
    kw = dict(quality=q)
    if blocks:
        kw["restart_marker_blocks"] = blocks
    Image.fromarray(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8), "CMYK").save(buf, "JPEG", **kw)
    data = buf.getvalue()
    sos = _segments(data)[1]
    assert data[sos + 4] == 4  # (Ns)
    return data


def _separated(files, seed0):
    """The files with a scan of another shape between every two: no two of them share a run."""
    out = []
    for k, f in enumerate(files):
        out += [f, _separator(seed0 + k)]
    return out[:-1]


def test_k2_corners_of_the_wave_through_the_plain_and_the_pooled_kernel():
    """What K2's two kernels share with the K2S final pass (k2_wave.h), at the corners of it, each through huffman_decode_kernel (a scan
    of one chunk) and through huffman_pool_kernel (two chunks or more): a scan of four interleaved components; a last restart interval
    shorter than DRI beside full ones; waves with fewer than 64 live lanes (every plain scan here, the last chunk of every pooled one);
    data that ends in the middle of a block (the fail-block record: the blocks in front of it reach the writer, no others).
    264 x 16 at 4:4:4 with DRI 2 is 33 intervals, all of them full; 264 x 24 has 50 with one MCU in the last."""
    four_plain, four_pool = _cmyk(64, 48, blocks=1, seed=1), _cmyk(104, 80, blocks=1, seed=2)
    few_420, few_422 = _synth(64, 48, "420", 75, 1, seed=3), _synth(64, 48, "422", 75, 1, seed=4)
    full = _synth(264, 16, "444", 75, 2, seed=5)
    short_plain, short_pool = _synth(264, 24, "444", 75, 2, seed=6), _synth(104, 88, "444", 75, 2, seed=7)
    assert [_intervals(f) for f in (four_plain, four_pool, few_420, few_422, full, short_plain, short_pool)] == [48, 130, 12, 24, 33, 50, 72]
    assert (33 * 3) % 2 == 1 and (13 * 11) % 2 == 1  # (MCUs of the two `short` files: the last interval has one)
    plain = [four_plain, few_420, few_422, full, short_plain, _cut(short_plain), _cut(four_plain)]
    pooled = [four_pool, short_pool, _cut(short_pool), _cut(four_pool)]
    files = _separated(plain + pooled, 1100)
    refs = _refs(files)
    kinds = [r.kind for r in refs[::2]]
    assert kinds[:5] == ["OK"] * 5 and kinds[7:9] == ["OK"] * 2 and "OK" not in kinds[5:7] + kinds[9:], kinds
    b, st, _ = _decode(files, refs)
    assert st["huffman_waves"] == FULL_WAVES, st
    assert st["k2_pools"] == len(pooled) and st["k2_pooled_chunks"] == sum(_chunks(f) for f in pooled) == 3 + 2 + 2 + 3, st
    assert st["k2_plain_work"] == len(plain) + len(files) // 2, st  # (every plain scan and every separator: one chunk, one workgroup)
    b.close()


# ------------------------------------------------------------------------------------------------ K2S (DRI = 0)

def test_k2s_pool_threshold_and_repeated_table_sets():
    """A run below 40 waves stays plain, one above is pooled; a run with the first run's tables, behind another set, is mapped back
    to the first set.  (The batch stays under 512 KB of DRI = 0 data: 512-bit subsequences, 40 waves = 160 KB.)"""
    small = _synth(512, 384, "420", 90, 0, seed=800)
    large = _optimized(_synth(1152, 864, "420", 90, 0, seed=801))
    again = _synth(512, 384, "420", 90, 0, seed=802)
    assert _huffman_tables(small) == _huffman_tables(again) != _huffman_tables(large)
    assert len(small) < 80_000 and 200_000 < len(large) and sum(map(len, (small, large, again))) < 450_000
    b, st, _ = _decode([small, large, again])
    assert st["k2s_scans"] == 3 and st["k2s_pools"] == 1 and st["k2s_plain_work"] > 0, st
    assert st["k2s_table_sets"] == 2, st
    b.close()


def test_k2s_more_than_eight_runs_with_distinct_tables():
    """Ten pool-eligible runs, each with tables of its own: eight pools, the last two runs plain, ten table sets.
    (Over 512 KB of DRI = 0 data: 1024-bit subsequences, 40 waves = 320 KB; each file is ~430 KB.)"""
    files = [_optimized(_synth(1408, 1152, "420", 90, 0, seed=900 + k)) for k in range(10)]
    assert all(400_000 < len(f) < 1_000_000 for f in files)
    assert len({tuple(sorted(_huffman_tables(f).items())) for f in files}) == 10
    b, st, _ = _decode(files, coefs=False)
    assert st["k2s_scans"] == 10 and st["k2s_pools"] == K2S_MAX_POOLS and st["k2s_plain_work"] > 0, st
    assert st["k2s_table_sets"] == 10 and st["k2s_subs_per_lane"] == 1, st
    b.close()


def test_k2s_pools_that_do_not_fit_beside_the_tables():
    """A file whose scan stages two more tables leaves no room for the pooled final pass's waves: no pools, still exact."""
    small = _synth(512, 384, "420", 90, 0, seed=800)
    large = _optimized(_synth(1152, 864, "420", 90, 0, seed=801))
    extra = _extra_slots(_synth(128, 96, "420", 75, 0, seed=1000))
    b, st, refs = _decode([small, large, extra])
    assert refs[2].kind == "OK"
    assert st["k2s_scans"] == 3 and st["k2s_pools"] == 0, st
    b.close()


def test_k2s_corners_of_the_wave_through_the_plain_and_the_pooled_final_pass():
    """The corners of test_k2_corners_... for the final pass, each in a run below 40 waves (subseq_final_kernel<false>) and in one above
    (<true>): four interleaved components; a scan of a few dozen lanes; data that ends in the middle of a block; and a lane that owns
    MCUs but starts behind the data (tests/golden/stress/dri0_invalid_code_late.jpg: 4:4:4, the standard tables -- alone, and in one
    run with a large file of that shape).  Two uploads, each under 512 KB of DRI = 0 data: 512-bit subsequences, 40 waves = 160 KB."""
    from golden_util import read_jpeg

    four_plain, four_pool = _cmyk(96, 96, seed=11), _cmyk(288, 256, seed=12)
    noise = _synth(96, 96, "420", 90, 0, seed=13)
    files = [four_plain, noise, four_pool, _cut(four_pool), _cut(noise), _cut(four_plain)]
    assert len(four_plain) < 80_000 and 200_000 < len(four_pool) and sum(map(len, files)) < 450_000
    refs = _refs(files)
    assert [r.kind == "OK" for r in refs] == [True, True, True, False, False, False]
    b, st, _ = _decode(files, refs)
    assert st["k2s_scans"] == 6 and st["k2s_pools"] == 1 and st["k2s_plain_work"] >= 4 and st["k2s_subs_per_lane"] == 1, st
    b.close()

    late = read_jpeg(os.path.join("stress", "dri0_invalid_code_late.jpg"))
    large = _synth(768, 640, "444", 90, 0, seed=14)
    assert _huffman_tables(late) == _huffman_tables(large) and 200_000 < len(large) < 450_000
    files = [large, late, noise, late]
    refs = _refs(files)
    assert [r.kind for r in refs] == ["OK", "InvalidDataException", "OK", "InvalidDataException"]
    b, st, _ = _decode(files, refs)
    assert st["k2s_scans"] == 4 and st["k2s_pools"] == 1 and st["k2s_plain_work"] >= 2, st
    b.close()


# ------------------------------------------------------------------------------------------------ repeated and staged calls

def _staged_batch(seed0):
    """At least three K2 pools (one with a failing file in it) and two K2S pools (under 512 KB of DRI = 0 data)."""
    k2 = _alternating_runs(4, seed0)
    k2.insert(1, _cut(_synth(160, 128, "420", 75, 1, seed=seed0 + 50)))
    k2s = [_synth(1024, 768, "420", 90, 0, seed=seed0 + 60), _optimized(_synth(1024, 768, "420", 90, 0, seed=seed0 + 61))]
    assert sum(map(len, k2s)) < 480_000
    return k2[:3] + [k2s[0]] + k2[3:] + [k2s[1]]


def _staged_sequence(b, refs, rng, what):
    for k in range(3):
        b.decode()
    b.sync()
    _check(b, refs, f"{what}: decode x3")
    _poison(b, refs, rng)
    b.run_entropy().sync()
    _check(b, refs, f"{what}: poisoned, run_entropy", pixels=False)
    _poison(b, refs, rng)
    b.run_entropy()
    b.run_entropy()
    b.run_idct().sync()
    _check(b, refs, f"{what}: poisoned, run_entropy x2, run_idct")
    _poison(b, refs, rng)
    b.decode().sync()
    _check(b, refs, f"{what}: poisoned, decode")


def test_repeated_and_staged_calls_on_one_upload():
    """Every pooled launch of every call must do its work: the coefficients are overwritten with noise in between, so a pooled
    launch that drew no work (its ticket counter and the host's count of it apart) shows in the output."""
    rng = np.random.default_rng(1)
    files = _staged_batch(1100)
    refs = _refs(files)
    assert refs[1].kind != "OK"
    b = jl.Batch().upload(files)
    st = b.plan_stats()
    assert st["k2_pools"] >= 3 and st["k2s_pools"] >= 2, st
    _staged_sequence(b, refs, rng, "first upload")
    # a different batch into the same object
    files2 = _staged_batch(1200)[::-1]
    refs2 = _refs(files2)
    b.upload(files2)
    st2 = b.plan_stats()
    assert st2["k2_pools"] >= 3 and st2["k2s_pools"] >= 2, st2
    _staged_sequence(b, refs2, rng, "second upload")
    # two batches of one context, their decodes interleaved
    ctx = b.ctx
    c = jl.Batch(ctx).upload(files)
    _poison(b, refs2, rng)
    c.decode()
    b.decode()
    c.decode()
    b.sync()
    c.sync()
    _check(b, refs2, "interleaved: b")
    _check(c, refs, "interleaved: c")
    _poison(c, refs, rng)
    b.decode()
    c.run_entropy()
    b.decode()
    c.run_idct()
    b.sync()
    c.sync()
    _check(b, refs2, "interleaved again: b")
    _check(c, refs, "interleaved again: c")
    b.close()
    c.close()


# ------------------------------------------------------------------------------------------------ re-planned images through stage calls

def test_replanned_images_through_stage_calls():
    """An image whose middle scan leaves one byte unread is planned again (DeviceBatch::redo_swallowed): its result and pixels stay
    the oracle's behind every stage call, not only behind decode(); its coefficients are refused (NotSupportedException)."""
    files, tags = middle_scan_swallow_files()
    refs = []
    for f in files:
        px, _, err = po.decode_8bit_partial(f)
        refs.append(("OK" if err is None else err.kind, px))
    # (with restart intervals the first scan already fails, "Expect restart marker.": nothing is planned again)
    replanned = [i for i, t in enumerate(tags) if t[0] == 0 and t[1] == 1 and t[2] != "eoi"]
    assert len(replanned) == 4 and all(refs[i][0] == "OK" for i in replanned)

    def check(what, coefs):
        for i, (kind, px) in enumerate(refs):
            out = np.asarray(b.output(i))
            assert np.array_equal(out, px), (what, tags[i], int((out != px).sum()))
            res = b.result(i)
            assert NAMES[res.status] == kind, (what, tags[i], kind, res.status, res.detail)
        if not coefs:
            return
        for i in replanned:
            with pytest.raises(jl.NotSupportedException):
                b.coefficients(i)
        for i, t in enumerate(tags):  # (a plan that held: its coefficients are there)
            if i not in replanned and refs[i][0] == "OK":
                assert b.coefficients(i).shape == (b.image_info(i).total_blocks, 64)

    b = jl.Batch().upload(files).decode().sync()
    # twice through the stage calls: results and pixels alone, then with the coefficients asked for too
    for coefs in (False, True):
        check("decode", coefs)
        b.run_idct().sync()
        check("decode, run_idct", coefs)
        b.run_entropy().sync()
        check("run_entropy", coefs)
        b.run_idct().sync()
        check("run_entropy, run_idct", coefs)
        b.decode().sync()
    check("decode again", True)
    b.close()
