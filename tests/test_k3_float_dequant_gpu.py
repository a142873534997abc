"""K3 dequantises in float with tables that carry the transform's 1/8 (DevQuantTable::qf, pair order) and packs its bytes with a
saturating pack.  Every sample of every case is compared with the oracle bit for bit.

What can go wrong that the rest of the suite would only show as a blur of wrong samples:
  * a table entry in the wrong place of the pair order, or a component reading another component's table: blocks that hold ONE
    coefficient each, under tables of 64 distinct quantisers -- a wrong entry shows in exactly one block;
  * the clamp: DC-only blocks whose samples land on and next to -129, -1, 0, 255, 256 and behind the int16 wrap of the level shift
    (a value that wraps to 126 where a saturating add would give 255);
  * the same through files, split and dense, and through dispose_pass_kernel, which keeps the integer dequantisation."""
import numpy as np
import pytest

import jpeglibrary_amd as jl
from oracle import pyoracle as po
from test_dispose_gpu import _progressive, _units
from test_idct_float64_cpu import in_envelope
from test_idct_stage_gpu import S420, S444, _assert_same, _expected, _file_case, _planes, _run_frames
from tools import jpegsynth

pytestmark = pytest.mark.gpu

GRAY = [(1, 1)]
FMTS = {"planar_i16": jl.FMT_PLANAR_I16, "interleaved_u8": jl.FMT_INTERLEAVED_U8, "planar_u8": jl.FMT_PLANAR_U8, "rgb_u8": jl.FMT_RGB_U8}


def _frame(w, h, sampling, selectors):
    return {"width": w, "height": h, "precision": 8, "components": [(i + 1, hh, vv, selectors[i]) for i, (hh, vv) in enumerate(sampling)]}


def _n_blocks(frame):
    comps = frame["components"]
    max_h, max_v = max(c[1] for c in comps), max(c[2] for c in comps)
    mcus = -(-frame["width"] // (8 * max_h)) * -(-frame["height"] // (8 * max_v))
    return mcus * sum(c[1] * c[2] for c in comps)


def _distinct_tables(rng, wide):
    """four tables (zig-zag) of 64 distinct quantisers each, no value in two tables: 8-bit ones, or 16-bit ones above 255"""
    pool = rng.permutation(np.arange(256, 65536) if wide else np.arange(1, 256))
    if wide:
        return pool[:256].reshape(4, 64).astype(np.uint16)
    return np.stack([pool[:64], pool[64:128], pool[128:192], pool[191:255]]).astype(np.uint16)  # (255 values: the last two share one)


@pytest.fixture(scope="module")
def one_coefficient_cases():
    """[(frames, tables, blocks, expected planes)] for the 8-bit and the 16-bit tables: block k of the batch (counted through its frames)
    holds zig-zag coefficient k % 64 alone.  A gray 64 x 64 frame (64 blocks: every entry of its table once) and three 4:2:0 32 x 32 frames
    (72 blocks: every coefficient index once and again, a table of its own per component)."""
    cases = []
    for wide in (False, True):
        rng = np.random.default_rng(7 + wide)
        qt = _distinct_tables(rng, wide)
        frames = [_frame(64, 64, GRAY, [1])] + [_frame(32, 32, S420, [0, 2, 3]) for _ in range(3)]
        blocks, k = [], 0
        for fi, fr in enumerate(frames):
            if fi == 1:
                k = 0
            z = np.zeros((_n_blocks(fr), 64), np.int16)
            for i in range(len(z)):
                z[i, k % 64] = int(rng.integers(3, 40)) * int(rng.choice([-1, 1]))
                k += 1
            blocks.append(z)
        for fr, z in zip(frames, blocks):  # (16-bit tables: inside the int32 envelope)
            bpm = sum(c[1] * c[2] for c in fr["components"])
            owner = [c[3] for c in fr["components"] for _ in range(c[1] * c[2])]
            assert all(in_envelope(z[i].astype(np.int64), qt[owner[i % bpm]]) for i in range(len(z)))
        cases.append((frames, qt, blocks, [_planes(fr, qt, z) for fr, z in zip(frames, blocks)]))
    return cases


@pytest.mark.parametrize("fmt", ["planar_i16", "interleaved_u8"])
@pytest.mark.parametrize("wide", [0, 1], ids=["8bit_tables", "16bit_tables"])
def test_one_coefficient_per_block_under_tables_of_distinct_quantisers(one_coefficient_cases, wide, fmt):
    frames, qt, blocks, planes = one_coefficient_cases[wide]
    assert sorted(int(np.flatnonzero(z)[0]) for z in blocks[0]) == list(range(64))
    assert {int(np.flatnonzero(z)[0]) for zs in blocks[1:] for z in zs} == set(range(64))
    b = _run_frames(frames, [qt] * len(frames), blocks, FMTS[fmt])
    for i, fr in enumerate(frames):
        want = _expected(FMTS[fmt], fr, planes[i])
        if fmt == "planar_i16":  # (the cases do tell the blocks apart: no block is flat at the level shift)
            assert all((p[y:y + 8, x:x + 8] != 128).any() for p in want for y in range(0, p.shape[0], 8) for x in range(0, p.shape[1], 8))
        _assert_same(b.output(i), want, (wide, fmt, i))
    b.close()


# DC-only blocks under q[0] = 8: sample = c + 128 exactly; under q[0] = 16: 2 * c + 128
EDGES_Q8 = [t - 128 for t in (-130, -129, -128, -2, -1, 0, 1, 254, 255, 256, 257, 300, -300)] + [32767, -32768, 32639, 32640]  # 32640 + 128 = 2^15: the wrap
EDGES_Q16 = [32767, -32768, 32703, 16320, 16319, -16449, -16448]  # 65662 -> 126, -65408 -> 128, ...: behind the wrap, back inside 0..255


@pytest.fixture(scope="module")
def clamp_cases():
    qt = np.stack([np.full(64, 8), np.full(64, 16), np.full(64, 8), np.full(64, 16)]).astype(np.uint16)
    frames = [_frame(64, 24, GRAY, [0]), _frame(64, 8, GRAY, [1]), _frame(32, 32, S420, [0, 1, 2]), _frame(24, 16, S444, [1, 0, 3])]
    blocks = []
    for fr in frames:
        z = np.zeros((_n_blocks(fr), 64), np.int16)
        bpm = sum(c[1] * c[2] for c in fr["components"])
        owner = [c[3] for c in fr["components"] for _ in range(c[1] * c[2])]
        for i in range(len(z)):
            edges = EDGES_Q8 if int(qt[owner[i % bpm]][0]) == 8 else EDGES_Q16
            z[i, 0] = edges[(i // bpm + i % bpm) % len(edges)]
        blocks.append(z)
    planes = [_planes(fr, qt, z) for fr, z in zip(frames, blocks)]
    seen = {int(v) for p in planes for c in p for v in np.unique(c)}
    assert {-130, -129, -128, -2, -1, 0, 1, 254, 255, 256, 257, 126}.issubset(seen), sorted(seen)  # (the oracle's samples are the edges meant)
    return frames, qt, blocks, planes


@pytest.mark.parametrize("fmt", ["interleaved_u8", "planar_u8", "rgb_u8"])
def test_the_saturating_pack_at_the_clamp_edges_and_behind_the_int16_wrap(clamp_cases, fmt):
    frames, qt, blocks, planes = clamp_cases
    b = _run_frames(frames, [qt] * len(frames), blocks, FMTS[fmt])
    for i, fr in enumerate(frames):
        _assert_same(b.output(i), _expected(FMTS[fmt], fr, planes[i]), (fmt, i))
    b.close()


@pytest.fixture(params=["split", "dense"])
def handoff(request, monkeypatch):
    monkeypatch.setenv("JPGPU_DENSE_HANDOFF", "1" if request.param == "dense" else "0")
    return request.param


_REF = {}


def _ref(f):
    if f not in _REF:
        _REF[f] = po.decode_8bit(f)[0]
    return _REF[f]


FILES = [(48, 32, "420", 1), (48, 32, "420", 4), (64, 16, "420", 1), (64, 16, "420", 4), (24, 24, "444", 2), (8, 8, "gray", 1)]


def test_small_files_split_and_dense(handoff):
    files = [bytes(jpegsynth.encode(w, h, sub, 75 + 5 * (i % 3), dri, seed=70 + i)) for i, (w, h, sub, dri) in enumerate(FILES)]
    for fmt in ("interleaved_u8", "rgb_u8"):
        outs, res = jl.decode_batch(files, FMTS[fmt])
        for i, f in enumerate(files):
            assert (res[i].status, res[i].detail) == (0, 0), (fmt, i)
            want = _ref(f) if fmt == "interleaved_u8" else po.ycbcr8_to_rgb(_ref(f), rgba=False, gray=_ref(f).shape[2] == 1)
            _assert_same(outs[i], want, (handoff, fmt, FILES[i]))


def test_a_12_bit_sof1_file_with_a_16_bit_table(handoff):
    frame, qt, blocks, data = _file_case(4242, 64, 40, GRAY, 12, 2)  # table slot 3: 16-bit entries, inside the int32 envelope
    assert int(qt[3].max()) > 255 and np.array_equal(po.decode_coefficients(data)[0], blocks)
    planes = _planes(frame, qt, blocks)
    for fmt in (jl.FMT_PLANAR_I16, jl.FMT_INTERLEAVED_U8):
        outs, res = jl.decode_batch([data], fmt)
        assert (res[0].status, res[0].detail) == (0, 0), fmt
        _assert_same(outs[0], _expected(fmt, frame, planes), fmt)
    _assert_same(outs[0], po.decode_8bit(data)[0], "oracle")


def test_a_progressive_file_whose_slots_end_out_of_order_goes_through_the_dispose_pass():
    """slots {Cb, Cb, Cr} (test_dispose_gpu.py): dispose_pass_kernel transforms Cb twice and Y never -- with its own integer
    dequantisation and the 1/8 multiplied in there -- and the flush writes the store out"""
    data = _progressive(48, 32, "4:2:0", seed=5)
    units, tail = _units(data)
    assert len(units) == 10
    odd = b"".join(units[:7] + [units[9], units[7], units[8]]) + tail
    for f in (data, odd):
        outs, res = jl.decode_batch([f], jl.FMT_INTERLEAVED_U8)
        assert res[0].status == 0, (res[0].status, res[0].detail)
        _assert_same(outs[0], po.decode_8bit(f)[0], "dispose")
    assert not np.array_equal(po.decode_8bit(odd)[0], po.decode_8bit(data)[0])  # (the odd order did reach the literal pass)
