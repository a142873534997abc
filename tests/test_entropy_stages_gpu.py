"""The encoder's entropy stages (encode_kernels.hip: E2 block_bits / block_stats / block_offsets, E3 emit_kernel and bits_emit_kernel,
E4 the stuffing pair) on coefficients that were written for them, regime by regime.

Every other test that reaches these kernels starts from pixels or natural files.  The inputs here (tests/test_entropy_stage_inputs_cpu.py)
are aimed at the places where the kernels decide something -- a workgroup's stretch in LDS or in global atomics, first and last words
shared with the neighbouring workgroup, fill == 0 against a partial last word, the pad of the stream and of every restart interval, the
mark bit and the marker number over a stuffing chunk's edge, FF bytes at the edges of a lane's 16 bytes and of a chunk, the phase of a
workgroup's base in bits_emit_kernel -- and reach them two ways that need no entry of their own:

  the optimizer's coefficient road, unturned: a window that is the whole frame hands the file's coefficients to block_stats_kernel<true>,
  block_bits_kernel<true>, emit_kernel<true> and the stuffing pair, and the bytes must be Optimize()'s;
  the encoder, from flat 8 x 8 blocks at quality 100, where every block is a DC difference and EOB.

Each input's precondition -- that it reaches its place -- is asserted again here.  Every comparison is byte for byte."""
import os

import numpy as np
import pytest

import encoder_arrangements as ea
import encoder_model as em
import jpeglibrary_amd as jl
import scan_writer as sw
import test_entropy_stage_inputs_cpu as es
import test_transcode_inputs_cpu as cat
from golden_util import read_jpeg
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The only inputs the coefficient road may refuse, by name, with the refusal of transform_plan.h and the words include/jpgpu.h documents
# it with ("Window", Refusals).  (testorig12 is SOF1: transform_plan.h refuses SOF2 and above only, so it is not among them.)
TEN_BLOCKS = ("More than ten blocks per MCU cannot be turned.", "more than ten blocks per MCU")
REFUSED = {n: TEN_BLOCKS for n in cat.INPUTS if n.startswith("sampling_4x2_2x2_1x1_")}


def _source(path):
    with open(os.path.join(ROOT, path)) as f:
        return " ".join(f.read().split())


def _frame(data):
    info = po.identify(data)[0]
    return (0, 0, info.width, info.height)


def _outcome(b, i):
    try:
        return b.output(i)
    except jl.JpegError as e:
        return e


def _first_difference(got, ref):
    return len(got), len(ref), next((k for k in range(min(len(got), len(ref))) if got[k] != ref[k]), None)


def _same(got, ref, what):
    if isinstance(ref, po.OracleError):
        assert isinstance(got, getattr(jl, ref.kind)), (what, ref, got)
    else:
        assert isinstance(got, bytes), (what, got)
        assert got == ref, (what,) + _first_difference(got, ref)


def _road(files, strip, most_optimal=False, windows=True):
    """one upload down the coefficient road (every file's window its whole frame) or, windows=False, the untouched road"""
    b = jl.OptimizeBatch().set_most_optimal_coding(most_optimal)
    if windows:
        b.set_windows([_frame(f) for f in files])
    return b.upload(files, strip).run()


# ---- a. the transcode catalogue down the coefficient road

def test_the_refusals_allowed_are_the_documented_ones():
    assert len(REFUSED) == 6 and not set(REFUSED) & set(cat.WRITTEN)
    for refusal, documented in set(REFUSED.values()):
        assert refusal in _source("jpeglibrary_amd/csrc/transform_plan.h") and documented in _source("include/jpgpu.h")

@pytest.mark.parametrize("strip", [False, True])
@pytest.mark.parametrize("name", cat.INPUTS)
def test_the_transcode_catalogue_down_the_coefficient_road(name, strip):
    """The whole frame written out: the encoder's kernels on the file's coefficients.  The same bytes as the untouched road -- the transcode
    kernels -- and as the oracle."""
    inp = cat.build(name)
    cat.check_precondition(name)
    ref = cat.oracle(name, strip)
    b = _road([inp.data], strip, inp.most_optimal)
    u = _road([inp.data], strip, inp.most_optimal, windows=False)
    try:
        got, untouched = _outcome(b, 0), _outcome(u, 0)
        _same(untouched, ref, (name, "untouched"))
        if isinstance(got, jl.NotSupportedException):
            assert name in REFUSED and REFUSED[name][0] in str(got), (name, got)
            return
        assert name not in REFUSED, name  # (a fence stays a fence)
        assert b.turn_sources() == 1 and u.turn_sources() == 0
        _same(got, ref, (name, "coefficient road"))
        if name in cat.WRITTEN:
            assert isinstance(got, bytes) and got == untouched
    finally:
        b.close()
        u.close()


# ---- b. the inputs written for the encoder's kernels

def _check_written(inp, b, i, got, strip):
    """the three checks that do not go through the oracle"""
    stats = {(c, t): {s: int(n) for s, n in enumerate(f) if n} for c, t, f in b.statistics(i)}
    assert stats == inp.info["tables"], inp.name  # block_stats_kernel<true>: the writer's own counts
    lengths, scan = sw.parse_baseline(got)
    assert len(scan) == sw.expected_scan_length(inp.info, lengths, scan), inp.name
    if not (strip and inp.dri):  # (strip drops the DRI segment: such an output no longer decodes)
        assert np.array_equal(po.decode_coefficients(got)[0], inp.coefs), inp.name


@pytest.mark.parametrize("strip", [False, True])
@pytest.mark.parametrize("name", es.WRITTEN)
def test_the_written_inputs_down_the_coefficient_road(name, strip):
    inp = es.build(name)
    es.check_precondition(name)
    ref = es.oracle(name, strip)
    b = _road([inp.data], strip)
    try:
        assert b.turn_sources() == 1
        got = _outcome(b, 0)
        _same(got, ref, name)
        _check_written(inp, b, 0, got, strip)
    finally:
        b.close()
    assert jl.optimize_batch([inp.data], strip) == [ref]  # the transcode kernels agree


# ---- c. batches

def _any(name):
    return (cat.build(name), cat.oracle(name, False)) if name in cat.INPUTS else (es.build(name), es.oracle(name, False))


@pytest.mark.parametrize("names", [("fat_intervals", "zero_64x64", "fat_workgroup"), ("fat_intervals", "zero_64x64"), ("zero_64x64", "fat_intervals", "fat_intervals")])
def test_lds_and_fallback_workgroups_in_one_launch(names):
    """lds_words is sized by the thin images; the fat image's workgroups, and the fat workgroup, write with global atomics beside them"""
    for n in set(names):
        (cat if n in cat.INPUTS else es).check_precondition(n)
    images, words = es.launch_of(names)
    lds = es.emit_lds_words(images)
    fits = [[w <= lds for w in image] for image in words]
    assert lds != 0 and all(fits[names.index("zero_64x64")]) and not fits[names.index("fat_intervals")][0], (lds, words)
    if "fat_workgroup" in names:
        assert fits[names.index("fat_workgroup")] == [True, False, True, True, True] and fits[0] == [False, True], (lds, words)
    pairs = [_any(n) for n in names]
    b = _road([inp.data for inp, _ in pairs], False)
    try:
        assert b.turn_sources() == len(set(names))
        for i, (inp, ref) in enumerate(pairs):
            got = _outcome(b, i)
            _same(got, ref, (i, names[i]))
            _check_written(inp, b, i, got, False)
    finally:
        b.close()


def test_a_batch_with_a_hole():
    """a progressive file the host refuses between two written inputs: work lists, bases and chunk descriptors are indexed across it"""
    names = ["marked_ff", None, "wg_edges_off_words", "color_444_dc_swings"]
    pairs = [_any(n) if n else None for n in names]
    files = [p[0].data if p else read_jpeg("progress.jpg") for p in pairs]
    for strip in (False, True):
        b = _road(files, strip)
        try:
            assert b.turn_sources() == 3
            for i, p in enumerate(pairs):
                got = _outcome(b, i)
                if p is None:
                    with pytest.raises(po.OracleError) as refused:  # (a file the optimizer's own walk fails keeps that status, window or not)
                        po.optimize(files[i], strip)
                    _same(got, refused.value, (i, "progressive", strip))
                else:
                    _same(got, es.oracle(names[i], strip), (i, names[i], strip))
                    _check_written(p[0], b, i, got, strip)
        finally:
            b.close()


# ---- d. the flat-block inputs through the encoder

def _other(inp):
    """a different image that the same upload takes"""
    if inp.pixels.ndim == 3:
        return np.random.default_rng(5).integers(0, 256, (40, 56, 3)).astype(np.uint8)
    return es.build_flat("flat_257" if inp.name == "flat_random" else "flat_random").pixels


def _encoded(images, luma, passes, **kw):
    """encode() twice (the second call sizes its buffers from the first): [(stream, coefficients)] per image, the same both times"""
    b = jl.EncodeBatch().upload(images, luma, 100, **kw)
    try:
        runs = []
        for rep in range(2):
            b.encode()
            assert b.emit_passes() == ((rep + 1) * passes, 0)
            runs.append([(b.output(i), b.coefficients(i)) for i in range(len(images))])
        assert all(a[0] == c[0] and np.array_equal(a[1], c[1]) for a, c in zip(*runs))
        return runs[0]
    finally:
        b.close()


def _alone_and_in_a_batch(inp, **kw):
    """The image alone -- emit_kernel<false> behind block_bits_kernel<false> -- and as images 0 and 2 of three: bits_emit_kernel, whose
    workgroups learn their bases from their predecessors, unless restart intervals keep the batch on the two kernels.  Every stream is
    the oracle's, every block the designed one."""
    ref = po.encode_8bit(inp.pixels, inp.luma[0], inp.luma[1], 100, **kw)
    (got, coefs), = _encoded([inp.pixels], inp.luma, 0, **kw)
    assert np.array_equal(coefs, inp.blocks)
    assert got == ref, ("alone",) + _first_difference(got, ref)
    other = _other(inp)
    outs = _encoded([inp.pixels, other, inp.pixels], inp.luma, 0 if kw.get("restart_interval") else 1, **kw)
    for i in (0, 2):
        assert np.array_equal(outs[i][1], inp.blocks)
        assert outs[i][0] == ref, (i,) + _first_difference(outs[i][0], ref)
    assert outs[1][0] == po.encode_8bit(other, inp.luma[0], inp.luma[1], 100, **kw)
    return ref


@pytest.mark.parametrize("name", es.FLAT)
def test_flat_blocks_with_the_standard_tables(name):
    inp = es.build_flat(name)
    es.check_flat_precondition(name)
    assert _alone_and_in_a_batch(inp) == es.flat_oracle(name)[0]


@pytest.mark.parametrize("name", es.FLAT)
def test_flat_blocks_with_built_tables(name):
    """block_stats_kernel<false>.  (Grey inputs with a constant chroma beside them: the reference builds tables for three components.)
    flat_const then costs two bits a block: every workgroup base on a word edge, the total a whole number of words."""
    inp = es.with_constant_chroma(es.build_flat(name))
    ref = _alone_and_in_a_batch(inp, optimize_coding=True)
    if name == "flat_const":
        lengths, scan = sw.parse_baseline(ref)
        assert all(t == {0: 1} for t in lengths.values()) and len(scan) * 8 == 2 * len(inp.dc) and len(scan) % 4 == 0


@pytest.mark.parametrize("ri", [1, 7])
@pytest.mark.parametrize("name", es.FLAT)
def test_flat_blocks_with_restart_intervals(name, ri):
    """one lane per interval, the pad and the mark of every interval; flat_const at ri = 1: a marker behind every byte, over a chunk's edge"""
    inp = es.build_flat(name)
    ref = _alone_and_in_a_batch(inp, restart_interval=ri)
    if name == "flat_const" and ri == 1:
        n = len(inp.dc)
        assert sw.parse_baseline(ref)[1] == b"".join(bytes([0x2B, 0xFF, 0xD0 + (k & 7)]) for k in range(n - 1)) + b"\x2b"


# ---- e. a described arrangement: emit_kernel<true> from the encoder's side

def _four_flat_components(mw, mh, seed):
    values = np.random.default_rng(seed).integers(0, 256, (mh, mw, 4)).astype(np.uint8)
    return values, np.ascontiguousarray(np.kron(values, np.ones((8, 8, 1), np.uint8)))


@pytest.mark.parametrize("ri", [0, 3])
@pytest.mark.parametrize("built", [False, True], ids=["given", "built"])
def test_a_described_arrangement_of_flat_blocks(built, ri):
    """arrangement A (four 1 x 1 components) with quantisation tables of ones: 528 blocks, three workgroups of the general kernels"""
    values, px = _four_flat_components(12, 11, 51)
    arr = ea.arrangement("A", built, restart_interval=ri)
    ones = [1] * 64
    for c in arr.components:
        c.quant = ones
    arr.quant_tables = [(0, ones), (1, ones)]
    ref, ref_coefs, in_grid = em.encode(px, arr)
    want = np.zeros((12 * 11 * 4, 64), np.int16)
    want[:, 0] = 8 * (values.reshape(-1).astype(np.int64) - 128)
    assert in_grid.all() and np.array_equal(ref_coefs, want)
    b = jl.EncodeBatch().upload_described([px], [ea.to_description(arr, px.shape[1], px.shape[0])])
    try:
        b.encode()
        got, coefs = b.output(0), b.coefficients(0)
    finally:
        b.close()
    assert np.array_equal(coefs, want) and got == ref, _first_difference(got, ref)
