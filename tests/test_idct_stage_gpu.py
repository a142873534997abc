"""K3 (k3_idct.hip) on every output layout class, sink and precision, every sample of every image compared.

K3 dequantises, runs the float32 IDCT on packed pairs, rounds half to even, adds the level shift with a 16-bit wrap, and writes
one of six sinks -- the YCbCr -> RGB(A) conversion fused into the fast layout classes (kLayYccH1V1 / H2V1 / H2V2, kLayGray).  Real
encoders give it moderate coefficients and 8-bit tables; here it gets full int16 coefficients, 16-bit tables, table selectors
0..3, the clamp edges and the int16 wrap, at every precision the sinks take.  Two ways in:
  * the frame hand-off (upload_frames + set_coefficients + run_idct): any geometry, tables and precision;
  * files written by the tiny entropy coder of golden_util (16-bit DQT, selectors 2 / 3, SOF1 with P != 8, AC categories 11..15)
    through the host parser, K1, K2 / K2S and K3.
Expected values: the oracle's block transform (held against the float64 IDCT in test_idct_float64_cpu.py) through a numpy model of
each writer; PLANAR_I16 is also held against the float64 model directly.  Batch.plan_stats()["idct_work"] proves which layout
class each case reached."""
import numpy as np
import pytest

import jpeglibrary_amd as jl
from golden_util import BitWriter, block_symbols, canonical_codes
from oracle import pyoracle as po
from test_idct_float64_cpu import check_tau_rule, in_envelope

pytestmark = pytest.mark.gpu

GENERIC, H1V1, H2V1, H2V2, GRAY = 0, 1, 2, 3, 4
S444, S422, S420 = [(1, 1), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)]
NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME = 3, 6


def _expected_class(w, h, sampling):
    """idct_layout_class (k3_idct.hip) for a frame of one scan with every component (image offsets are 256-byte aligned)"""
    if len(sampling) == 1:
        return GRAY if sampling[0] == (1, 1) and w % 8 == 0 else GENERIC
    if len(sampling) != 3 or sampling[0] not in ((1, 1), (2, 1), (2, 2)) or sampling[1:] != [(1, 1), (1, 1)]:
        return GENERIC
    if sampling[0] == (1, 1):
        return H1V1 if w % 8 == 0 else GENERIC
    if w % 16 != 0:
        return GENERIC
    return H2V1 if sampling[0] == (2, 1) else H2V2


# ------------------------------------------------------------------------------------------------ inputs

def _tables(rng):
    """quantisation table slots 0..3 (zig-zag): random 1..255, all 1, all 255, random 16-bit"""
    return np.stack([rng.integers(1, 256, 64), np.ones(64, np.int64), np.full(64, 255), rng.integers(1, 65536, 64)]).astype(np.uint16)


def _block(rng, q, shift):
    """one zig-zag block for table q: the regimes of test_idct_float64_cpu plus the clamp edges and the int16 wrap"""
    z = np.zeros(64, np.int64)
    kind = rng.random()
    if kind < 0.30:
        keep = rng.random(64) < 0.3
        z[keep] = rng.integers(-64, 65, int(keep.sum()))
    elif kind < 0.45:
        keep = rng.random(64) < 0.05
        z[keep] = rng.integers(-32768, 32768, int(keep.sum()))
        z[0] = rng.integers(-32768, 32768)
    elif kind < 0.55:
        z[rng.integers(0, 64)] = rng.choice([-1, 1]) * rng.choice([1, 7, 100, 1000, 32767])
    elif kind < 0.80:
        # DC only, the exact output after the shift at (or next to) -1, 0, 255, 256
        target = int(rng.choice([-1, 0, 255, 256])) + int(rng.integers(-1, 2)) * (kind < 0.7)
        z[0] = int(np.clip(round(8 * (target - shift) / int(q[0])), -32768, 32767))
        if kind > 0.75:
            z[1:4] = rng.integers(-2, 3, 3)
    elif kind < 0.88:
        z[0] = rng.choice([32767, -32768, 30000, -30000])  # past the int16 wrap with q >= 8
    # (else: a zero block)
    if int(q.max()) > 255 and not in_envelope(z, q):  # 16-bit tables: inside the int32 envelope here
        z[1:] = 0
        z[0] = np.clip(z[0], -4000, 4000)
        if not in_envelope(z, q):
            z[0] = 0
    return z.astype(np.int16)


def _frame(rng, w, h, sampling, precision=8, selectors=None):
    """(frame dict, tables [4][64], coefficient blocks in MCU scan order)"""
    n = len(sampling)
    sel = selectors if selectors is not None else [int(t) for t in rng.permutation(4)[:n]]
    comps = [(i + 1, hh, vv, sel[i]) for i, (hh, vv) in enumerate(sampling)]
    max_h, max_v = max(s[0] for s in sampling), max(s[1] for s in sampling)
    mcus = (-(-w // (8 * max_h))) * (-(-h // (8 * max_v)))
    qt = _tables(rng)
    shift = 1 << (precision - 1)
    blocks = [_block(rng, qt[sel[c]], shift) for _ in range(mcus) for c, (hh, vv) in enumerate(sampling) for _ in range(hh * vv)]
    return {"width": w, "height": h, "precision": precision, "components": comps}, qt, np.stack(blocks)


# ------------------------------------------------------------------------------------------------ writer models

def _planes(frame, qt, blocks):
    """the oracle's samples on each component's own grid (PLANAR_I16: WriteBlock's arguments before replication)"""
    w, h, comps = frame["width"], frame["height"], frame["components"]
    shift = 1 << (frame["precision"] - 1)
    max_h, max_v = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-w // (8 * max_h)), -(-h // (8 * max_v))
    planes = [np.zeros((my * c[2] * 8, mx * c[1] * 8), np.int16) for c in comps]
    bpm = sum(c[1] * c[2] for c in comps)
    samples = np.empty((len(blocks), 8, 8), np.int16)
    k = 0
    for ci, (_, hh, vv, tq) in enumerate(comps):
        idx = [m * bpm + sum(c[1] * c[2] for c in comps[:ci]) + j for m in range(mx * my) for j in range(hh * vv)]
        samples[idx] = po.block_dequant_idct_shift(blocks[idx], qt[tq], shift).reshape(-1, 8, 8)
    for m in range(mx * my):
        for ci, (_, hh, vv, _) in enumerate(comps):
            for y in range(vv):
                for x in range(hh):
                    by, bx = (m // mx) * vv + y, (m % mx) * hh + x
                    planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = samples[k]
                    k += 1
    return planes


def _full(frame, planes):
    """each component replicated to the frame's resolution (WriteBlockSlow, factors that are the maximum or 1) and cropped"""
    comps, w, h = frame["components"], frame["width"], frame["height"]
    max_h, max_v = max(c[1] for c in comps), max(c[2] for c in comps)
    return [np.repeat(np.repeat(p, max_v // c[2], axis=0), max_h // c[1], axis=1)[:h, :w] for p, c in zip(planes, comps)]


def _interleaved(frame, planes):
    return np.stack([np.clip(f, 0, 255).astype(np.uint8) for f in _full(frame, planes)], axis=-1)  # signed clamp of int16


def _expand(bits, p):
    """JpegExtendingOutputWriter.FastExpandBits / ExpandBits (JpegExtendingOutputWriter.cs:83-110), uint32 arithmetic"""
    bits = bits.astype(np.uint64)
    if p >= 8:
        rem = 16 - p
        return ((bits << np.uint64(rem)) | (bits & np.uint64((1 << rem) - 1))) & np.uint64(0xFFFFFFFF)
    cur = p
    while cur < 16:
        bits = ((bits << np.uint64(p)) | bits) & np.uint64(0xFFFFFFFF)
        cur += p
    if cur > 16:
        bits >>= np.uint64(p)
        cur -= p
        rem = 16 - cur
        bits = ((bits << np.uint64(rem)) | (bits & np.uint64((1 << rem) - 1))) & np.uint64(0xFFFFFFFF)
    return bits


def _extended(frame, planes):
    """EXTENDED_U16: [H, W, 4] ushort, (ushort)sample clamped to 2^P - 1 and spread over 16 bits; absent channels 0"""
    p = frame["precision"]
    out = np.zeros((frame["height"], frame["width"], 4), np.uint16)
    for c, f in enumerate(_full(frame, planes)):
        v = np.minimum(f.astype(np.uint16).astype(np.uint64), (1 << p) - 1)
        out[..., c] = _expand(v, p).astype(np.uint16)
    return out


def _expected(fmt, frame, planes):
    if fmt == jl.FMT_PLANAR_I16:
        return planes
    if fmt == jl.FMT_PLANAR_U8:
        return [np.clip(p, 0, 255).astype(np.uint8) for p in planes]
    if fmt == jl.FMT_EXTENDED_U16:
        return _extended(frame, planes)
    il = _interleaved(frame, planes)
    if fmt == jl.FMT_INTERLEAVED_U8:
        return il
    return po.ycbcr8_to_rgb(il, rgba=fmt == jl.FMT_RGBA_U8, gray=il.shape[2] == 1)


def _run_frames(frames, qts, blocks, fmt):
    b = jl.Batch().upload_frames(frames, np.stack(qts), fmt)
    for i in range(len(frames)):
        assert b.image_info(i).status == 0, (i, b.image_info(i).status)
        b.set_coefficients(i, blocks[i])
    b.run_idct().sync()
    return b


def _assert_same(got, want, what):
    if isinstance(want, list):
        assert len(got) == len(want), what
        for c, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(g, w), (what, c, int((g != w).sum()))
    else:
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


# ------------------------------------------------------------------------------------------------ geometry matrix

GEOMETRIES = [
    # (W, H, sampling): gray and 4:4:4 with W % 8 = 0 / != 0; 4:2:2 and 4:2:0 with W % 16 in {0, 8, other}; H % (8 Vmax) in {0, 1, 8}
    (64, 40, [(1, 1)]), (61, 40, [(1, 1)]), (1, 1, [(1, 1)]), (8, 8, [(1, 1)]), (8, 8 * 9, [(1, 1)]),
    (64, 48, S444), (59, 48, S444), (64, 49, S444), (1, 1, S444), (8, 8, S444), (8 * 11, 8, S444),
    (64, 32, S422), (72, 32, S422), (37, 32, S422), (64, 33, S422), (64, 24, S422), (16, 8, S422),
    (64, 32, S420), (72, 32, S420), (45, 32, S420), (64, 33, S420), (64, 40, S420), (16, 16, S420), (16, 16 * 7, S420), (1, 1, S420),
    # generic layouts: 1x2 luma, 4x1 luma, chroma ABOVE the luma, two and four components
    (40, 48, [(1, 2), (1, 1), (1, 1)]), (64, 24, [(4, 1), (1, 1), (1, 1)]), (48, 48, [(1, 1), (2, 2), (2, 2)]),
    (40, 24, [(1, 1), (1, 1)]), (33, 17, [(2, 2), (1, 1), (1, 1), (2, 2)]),
]
# whole MCU counts one below, at and one above a tile (kIdctBlocksPerWg / bpm MCUs, and the 128-byte aligned tile the planner
# cuts, device_batch_layout.cpp): one MCU row of each
TILE_ROWS = [(8 * n, 8, [(1, 1)]) for n in (255, 256, 257)] + [(8 * n, 8, S444) for n in (79, 80, 81, 84, 85, 86)] + \
            [(16 * n, 8, S422) for n in (63, 64, 65)] + [(16 * n, 16, S420) for n in (39, 40, 41, 42, 43)] + \
            [(8, 8 * n, S444) for n in (84, 85, 86)]  # ... and one MCU column
BIG = [(16 * (4 * 42 + 3), 16 * 5 + 1, S420)]  # at least four tiles of MCUs per row, five MCU rows


def _cases(seed, geometries, precision=8):
    rng = np.random.default_rng(seed)
    return [_frame(rng, w, h, s, precision) for (w, h, s) in geometries]


@pytest.mark.parametrize("fmt", [jl.FMT_INTERLEAVED_U8, jl.FMT_RGB_U8, jl.FMT_RGBA_U8], ids=["interleaved", "rgb", "rgba"])
def test_every_layout_class_reaches_its_class_alone(fmt):
    """each geometry in a batch of its own: the class it reaches (plan_stats) and every sample"""
    for i, (frame, qt, blocks) in enumerate(_cases(1, GEOMETRIES)):
        sampling = [(c[1], c[2]) for c in frame["components"]]
        if fmt != jl.FMT_INTERLEAVED_U8 and len(sampling) not in (1, 3):
            continue
        b = _run_frames([frame], [qt], [blocks], fmt)
        work = b.plan_stats()["idct_work"]
        cls = _expected_class(frame["width"], frame["height"], sampling)
        assert work[cls] > 0 and sum(work) == work[cls], (i, frame["width"], frame["height"], sampling, work)
        _assert_same(b.output(0), _expected(fmt, frame, _planes(frame, qt, blocks)), (fmt, i))


@pytest.mark.parametrize("fmt", [jl.FMT_INTERLEAVED_U8, jl.FMT_RGB_U8, jl.FMT_RGBA_U8, jl.FMT_PLANAR_U8, jl.FMT_PLANAR_I16, jl.FMT_EXTENDED_U16],
                         ids=["interleaved", "rgb", "rgba", "planar_u8", "planar_i16", "extended_u16"])
def test_all_classes_in_one_batch_in_two_orders(fmt):
    cases = [c for c in _cases(2, GEOMETRIES + TILE_ROWS + BIG)
             if fmt not in (jl.FMT_RGB_U8, jl.FMT_RGBA_U8) or len(c[0]["components"]) in (1, 3)]
    want = [_expected(fmt, f, _planes(f, q, bl)) for f, q, bl in cases]
    for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
        b = _run_frames([cases[i][0] for i in order], [cases[i][1] for i in order], [cases[i][2] for i in order], fmt)
        for k, i in enumerate(order):
            _assert_same(b.output(k), want[i], (fmt, i))
            if fmt == jl.FMT_PLANAR_I16:  # the GPU against the float64 IDCT, not the oracle alone
                frame, qt, blocks = cases[i]
                _check_planes_tau(frame, qt, blocks, b.output(k))
        work = b.plan_stats()["idct_work"]
        if fmt in (jl.FMT_INTERLEAVED_U8, jl.FMT_RGB_U8, jl.FMT_RGBA_U8):
            reached = {_expected_class(f["width"], f["height"], [(c[1], c[2]) for c in f["components"]]) for f, _, _ in cases}
            assert reached == {GENERIC, H1V1, H2V1, H2V2, GRAY} and all(work[c] > 0 for c in reached) and work[5] == 0, work
        else:
            assert work[0] > 0 and sum(work) == work[0], work


def _check_planes_tau(frame, qt, blocks, planes):
    comps = frame["components"]
    shift = 1 << (frame["precision"] - 1)
    max_h, max_v = max(c[1] for c in comps), max(c[2] for c in comps)
    mx = -(-frame["width"] // (8 * max_h))
    bpm = sum(c[1] * c[2] for c in comps)
    k = 0
    got = np.empty((len(blocks), 8, 8), np.int16)
    tq = np.empty(len(blocks), np.int64)
    for m in range(len(blocks) // bpm):
        for ci, (_, hh, vv, t) in enumerate(comps):
            for y in range(vv):
                for x in range(hh):
                    by, bx = (m // mx) * vv + y, (m % mx) * hh + x
                    got[k] = planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]
                    tq[k] = t
                    k += 1
    for t in range(4):
        sel = tq == t
        if sel.any():
            check_tau_rule(got[sel], blocks[sel], qt[t], shift, what=("gpu", t))


def test_precisions_on_planar_i16_and_extended_u16():
    """P = 1..16 (level shift 1 << (P - 1)) on the two sinks that take any precision; 8 and 12 on the 8-bit planar and
    interleaved sinks; RGB / RGBA refuse P != 8 by themselves"""
    geos = [(64, 32, S420), (40, 24, [(1, 1)]), (24, 17, S444)]
    for p in range(1, 17):
        cases = _cases(100 + p, geos, precision=p)
        fmts = [jl.FMT_PLANAR_I16, jl.FMT_EXTENDED_U16] + ([jl.FMT_PLANAR_U8, jl.FMT_INTERLEAVED_U8] if p in (8, 12) else [])
        for fmt in fmts:
            b = _run_frames([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], fmt)
            for i, (f, q, bl) in enumerate(cases):
                _assert_same(b.output(i), _expected(fmt, f, _planes(f, q, bl)), (p, fmt, i))
                if fmt == jl.FMT_PLANAR_I16:
                    _check_planes_tau(f, q, bl, b.output(i))
        if p != 8:
            for fmt in (jl.FMT_RGB_U8, jl.FMT_RGBA_U8):
                b = jl.Batch().upload_frames([cases[0][0]], np.stack([cases[0][1]]), fmt)
                assert (b.image_info(0).status, b.image_info(0).detail) == (NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME), (p, fmt)


@pytest.mark.parametrize("p", [0, 17, 255])
def test_extended_u16_refuses_precisions_outside_1_to_16(p):
    """The test writer's ExpandBits loop never ends at P = 0 and its shifts leave 32 bits above 16: the image fails by itself on
    the host, asserted straight after the upload and before any kernel runs.  (The oracle's writer is never asked: it loops.)"""
    rng = np.random.default_rng(p)
    frame, qt, _ = _frame(rng, 16, 16, S444, precision=8)
    frame["precision"] = p
    b = jl.Batch().upload_frames([frame], np.stack([qt]), jl.FMT_EXTENDED_U16)
    assert (b.image_info(0).status, b.image_info(0).detail) == (NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME)
    b.run_idct().sync()
    assert b.result(0).status == NOT_SUPPORTED
    # the same frame as a file (SOF1, precision byte p), also in a batch of its own
    data = write_file(16, 16, p, [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)], {0: (0, qt[0]), 1: (0, qt[2])},
                      np.zeros((12, 64), np.int16), dri=0)
    b = jl.Batch().upload([data], jl.FMT_EXTENDED_U16)
    assert (b.image_info(0).status, b.image_info(0).detail) == (NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME)
    b.decode().sync()
    assert b.result(0).status == NOT_SUPPORTED


def test_out_of_int32_samples_are_a_fence_with_a_pinned_value():
    """A first transform with 16-bit tables can leave int32 (|v| up to 6.98 * 32767 * 65535).  (int)MathF.Round gives INT_MIN
    there on x64 -- the oracle's sample is the level shift -- while K3's conversion saturates (selecting INT_MIN cost
    K3 4 % on the headline workload): a sample >= 2^31 comes out as (0xFFFF + shift) mod 2^16 = shift - 1, one <= -2^31 as the
    shift, like the oracle.  Everything inside int32 equals the oracle."""
    from test_idct_float64_cpu import idct_float64
    q = np.full(64, 65535, np.uint16)
    blocks = np.zeros((12, 64), np.int16)
    blocks[0], blocks[1], blocks[2] = 32767, -32768, 0
    blocks[3, 0] = 32767  # DC alone: 2.68e8 per sample, inside int32, wrapped
    blocks[4, :10] = 32767
    blocks[5:] = np.random.default_rng(32).integers(-32768, 32768, (7, 64))
    qt = np.stack([q, q, q, q])
    exact, _ = idct_float64(blocks, q)
    assert not ((np.abs(exact) > 2.0 ** 31 * 0.99) & (np.abs(exact) < 2.0 ** 31 * 1.01)).any()  # nothing at float32's edge
    high = exact > 2.0 ** 31
    assert high.sum() > 10 and (exact < -(2.0 ** 31)).sum() > 10
    for p in (8, 12):
        shift = 1 << (p - 1)
        frame = {"width": 16, "height": 16, "precision": p, "components": [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 2)]}
        planes = _planes(frame, qt, blocks)
        assert planes[0][0, 0] == shift  # (the oracle: INT_MIN's low 16 bits + the shift)
        gpu = [pl.copy() for pl in planes]  # the GPU's rule: the oracle's samples, shift - 1 where the value is >= 2^31
        for i in range(len(blocks)):
            m, c = divmod(i, 3)
            blk = gpu[c][(m // 2) * 8:(m // 2) * 8 + 8, (m % 2) * 8:(m % 2) * 8 + 8]
            blk[high[i]] = shift - 1
        fmts = [jl.FMT_PLANAR_I16, jl.FMT_INTERLEAVED_U8, jl.FMT_EXTENDED_U16] + ([jl.FMT_RGB_U8] if p == 8 else [])
        for fmt in fmts:
            b = _run_frames([frame], [qt], [blocks], fmt)
            _assert_same(b.output(0), _expected(fmt, frame, gpu), (p, fmt))


# ------------------------------------------------------------------------------------------------ files

def write_file(w, h, precision, comps, tables, blocks, dri):
    """A sequential Huffman file (SOF1, or SOF0 at P = 8) of the given zig-zag blocks in MCU order.  comps = [(id, h, v, tq)],
    tables = {tq: (Pq, uint16[64])}.  One DC and one AC table of fixed-length codes for the symbols the blocks use (DC
    categories up to 16, AC sizes up to 15); restart markers every `dri` MCUs."""
    bpm = sum(c[1] * c[2] for c in comps)
    owner = [ci for ci, c in enumerate(comps) for _ in range(c[1] * c[2])]
    per_interval = bpm * dri if dri else len(blocks) + 1
    syms, pred, dc_used, ac_used = [], [0] * len(comps), set(), set()
    for i, blk in enumerate(blocks):
        ci = owner[i % bpm]
        if i % per_interval == 0:
            pred = [0] * len(comps)
        (dcat, dbits), ac = block_symbols(blk, pred[ci])
        assert dcat <= 16
        pred[ci] = int(blk[0])
        dc_used.add(dcat)
        ac_used.update(s for s, _, _ in ac)
        syms.append((dcat, dbits, ac))
    dc = canonical_codes({s: 5 for s in dc_used})
    ac = canonical_codes({s: 8 for s in (ac_used or {0})})
    out = bytearray(b"\xff\xd8")
    for tq, (pq, q) in sorted(tables.items()):
        body = bytes([(pq << 4) | tq]) + (bytes(int(v) for v in q) if pq == 0 else b"".join(int(v).to_bytes(2, "big") for v in q))
        out += b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + body
    sof = bytes([precision & 0xFF]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)])
    sof += b"".join(bytes([cid, (hh << 4) | vv, tq]) for cid, hh, vv, tq in comps)
    out += (b"\xff\xc0" if precision == 8 and all(p == 0 for p, _ in tables.values()) else b"\xff\xc1") + (len(sof) + 2).to_bytes(2, "big") + sof
    for cls, (codes, bits, vals) in ((0, dc), (1, ac)):
        body = bytes([cls << 4]) + bytes(bits) + bytes(vals)
        out += b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
    if dri:
        out += b"\xff\xdd\x00\x04" + dri.to_bytes(2, "big")
    sos = bytes([len(comps)]) + b"".join(bytes([c[0], 0x00]) for c in comps) + b"\x00\x3f\x00"
    out += b"\xff\xda" + (len(sos) + 2).to_bytes(2, "big") + sos
    bw = BitWriter()
    for i, (dcat, dbits, acs) in enumerate(syms):
        if i and i % per_interval == 0:
            bw.flush()
            bw.out += bytes([0xFF, 0xD0 + ((i // per_interval - 1) & 7)])
        bw.put(*dc[0][dcat])
        if dcat:
            bw.put(dbits, dcat)
        for s, m, size in acs:
            bw.put(*ac[0][s])
            if size:
                bw.put(m, size)
    bw.flush()
    return bytes(out) + bytes(bw.out) + b"\xff\xd9"


def _file_case(seed, w, h, sampling, precision, dri):
    """every component its own selector (2 and 3 among them), 16-bit DQT for slots 1 and 3, DC differences within category 16"""
    rng = np.random.default_rng(seed)
    sel = [3, 2, 1, 0][:len(sampling)]
    frame, qt, blocks = _frame(rng, w, h, sampling, precision, selectors=sel)
    # large AC coefficients (sizes 11..15) on the 8-bit slots; the 16-bit slot 3 stays inside the int32 envelope
    owner = [sel[c] for c, (hh, vv) in enumerate(sampling) for _ in range(hh * vv)]
    for i in range(len(blocks)):
        if owner[i % len(owner)] != 3 and rng.random() < 0.2:
            k = rng.integers(1, 64, 3)
            blocks[i, k] = rng.choice([-1, 1], 3) * rng.integers(1024, 32768, 3)
    tables = {t: (1 if t in (1, 3) else 0, qt[t]) for t in sel}  # slot 1 (all ones) and slot 3 written with 16-bit entries (Pq = 1)
    data = write_file(w, h, precision, frame["components"], tables, blocks, dri)
    return frame, qt, blocks, data


@pytest.mark.parametrize("dri", [0, 3])
def test_files_with_16_bit_tables_selectors_2_3_and_sof1_precisions(dri):
    cases = []
    for i, (w, h, s, p) in enumerate([(64, 32, S420, 8), (72, 24, S422, 8), (61, 23, S444, 8), (64, 40, [(1, 1)], 12),
                                      (40, 16, S444, 12), (33, 17, [(1, 1)], 16), (24, 16, S420, 5), (16, 8, S444, 1)]):
        cases.append(_file_case(1000 + 10 * i + dri, w, h, s, p, dri))
    files = [c[3] for c in cases]
    for frame, qt, blocks, data in cases:
        ref, _ = po.decode_coefficients(data)  # (the writer wrote what it meant to)
        assert np.array_equal(ref, blocks)
    for fmt in (jl.FMT_PLANAR_I16, jl.FMT_EXTENDED_U16, jl.FMT_INTERLEAVED_U8, jl.FMT_RGBA_U8):
        outs, res = jl.decode_batch(files, fmt)
        for i, (frame, qt, blocks, data) in enumerate(cases):
            if fmt == jl.FMT_RGBA_U8 and frame["precision"] != 8:
                assert (res[i].status, res[i].detail) == (NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME), i
                continue
            if fmt == jl.FMT_INTERLEAVED_U8 and frame["precision"] not in (8, 12):
                continue
            assert (res[i].status, res[i].detail) == (0, 0), (fmt, i, res[i].status)
            planes = _planes(frame, qt, blocks)
            _assert_same(outs[i], _expected(fmt, frame, planes), (fmt, i))
            if fmt == jl.FMT_INTERLEAVED_U8:
                _assert_same(outs[i], po.decode_8bit(data)[0], (fmt, i, "oracle"))
            elif fmt == jl.FMT_EXTENDED_U16:
                _assert_same(outs[i], po.decode_16bit(data)[0], (fmt, i, "oracle"))
            elif fmt == jl.FMT_RGBA_U8:
                _assert_same(outs[i], po.ycbcr8_to_rgb(po.decode_8bit(data)[0], rgba=True, gray=frame["components"].__len__() == 1), (fmt, i, "oracle"))
            else:
                _check_planes_tau(frame, qt, blocks, outs[i])
