"""The optimizer's transcode kernels (kt_transcode.hip, device_optimize.cpp) regime by regime.

The other optimizer tests run natural files end to end.  These inputs (tests/test_transcode_inputs_cpu.py, written by
tests/scan_writer.py) are aimed at the places where KT (one lane per restart interval, the bit writer simulated in registers) and KTS
(DRI = 0: block-aligned ownership over K2S's subsequences, bits ORed into a zeroed buffer, the encoder's stuffing stage behind it)
decide something: tables of one symbol, 16-bit codes in front of ten magnitude bits, totals that end on a byte or word edge, FF bytes at
the stuffing chunks' edges, blocks longer than a subsequence, one / several workgroups and the offset scans' per > 1, every
subsequence length the planner can pick, holes in a batch, per-component sampling factors, 12-bit SOF1.  Each input's precondition --
that it reaches its place -- is asserted again here on the oracle's output.

Every output is compared byte for byte with the oracle's JpegOptimizer restatement, and three ways that do not go through it:
(a) the statistics against the writer's own symbol counts, (b) the coefficients of the output against the ones written, (c) the length
of the output's scan against the writer's counts priced with the output's own DHT."""
import os
import re

import numpy as np
import pytest

import jpeglibrary_amd as jl
import scan_writer as sw
import test_transcode_inputs_cpu as cat
from golden_util import read_jpeg
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

SHIFTS = (9, 10, 11, 12, None)  # JPGPU_SUBSEQ_SHIFT: what the planner can pick from a batch's DRI = 0 bits, and its own choice
# NotSupportedException where the oracle succeeds: message of the device path -> the words DESIGN.md section 5 documents the fence with
FENCES = {"ratios that are not powers of two": "ratios that are not powers of two", "More than 16 blocks per MCU": "more than 16 blocks per MCU"}


def _set_shift(monkeypatch, shift):
    if shift is None:
        monkeypatch.delenv("JPGPU_SUBSEQ_SHIFT", raising=False)
    else:
        monkeypatch.setenv("JPGPU_SUBSEQ_SHIFT", str(shift))


def _outcome(b, i):
    try:
        return b.output(i)
    except jl.JpegError as e:
        return e


def _documented_fence(err):
    design = re.sub(r"\s+", " ", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read())
    named = [words for msg, words in FENCES.items() if msg in str(err)]
    assert len(named) == 1 and named[0] in design, f"NotSupportedException that DESIGN.md does not document: {err}"
    print("fence:", named[0])


def _same_as_oracle(got, ref, what):
    if isinstance(ref, po.OracleError):
        assert isinstance(got, getattr(jl, ref.kind)), (what, ref, got)
    elif isinstance(got, jl.NotSupportedException):
        _documented_fence(got)  # a fence stays a fence, by name
    else:
        assert isinstance(got, bytes), (what, got)
        assert got == ref, (what, len(got), len(ref), next((k for k in range(min(len(got), len(ref))) if got[k] != ref[k]), None))


@pytest.mark.parametrize("strip", [False, True])
@pytest.mark.parametrize("name", cat.INPUTS)
def test_every_regime_against_the_oracle_and_the_writer(name, strip, monkeypatch):
    _set_shift(monkeypatch, None)
    inp = cat.build(name)
    cat.check_precondition(name)
    ref = cat.oracle(name, strip)
    b = jl.OptimizeBatch().set_most_optimal_coding(inp.most_optimal).upload([inp.data], strip).run()
    try:
        got = _outcome(b, 0)
        _same_as_oracle(got, ref, name)
        if not isinstance(got, bytes):
            assert name not in cat.WRITTEN  # (the written inputs never fail)
            return
        if inp.info is not None:
            # (a) Scan()'s statistics are the writer's own counts
            stats = {(c, t): {s: int(n) for s, n in enumerate(f) if n} for c, t, f in b.statistics(0)}
            assert stats == inp.info["tables"]
            # (c) the scan is as long as these symbols are with the output's own tables
            lengths, scan = sw.parse_baseline(got)
            assert len(scan) == sw.expected_scan_length(inp.info, lengths, scan)
        if not (strip and inp.dri):  # (b) (strip drops the DRI segment: such an output no longer decodes)
            want = inp.coefs if inp.coefs is not None else po.decode_coefficients(inp.data)[0]
            assert np.array_equal(po.decode_coefficients(got)[0], want)
    finally:
        b.close()


@pytest.mark.parametrize("name", [n for n in cat.INPUTS if n.endswith("dri0") or n == "testorig12" or (n in cat.WRITTEN and "dri" not in n and "intervals" not in n)])
def test_every_subsequence_length_gives_the_same_bytes(name, monkeypatch):
    """The planner picks the subsequence length from the whole batch's DRI = 0 bits, so a file is cut differently beside other files.
    Pinned to each length it can pick, and left alone: the same bytes, the oracle's."""
    inp = cat.build(name)
    assert inp.dri == 0
    cat.check_precondition(name)
    ref = cat.oracle(name, False)
    for shift in SHIFTS:
        _set_shift(monkeypatch, shift)
        b = jl.OptimizeBatch().set_most_optimal_coding(inp.most_optimal).upload([inp.data], False).run()
        try:
            _same_as_oracle(_outcome(b, 0), ref, (name, shift))
        finally:
            b.close()


def test_long_blocks_at_the_shortest_subsequence(monkeypatch):
    """Lanes whose whole subsequence lies inside one block own nothing (count == 0), several in a row: pinned to 512-bit subsequences,
    where the precondition counts them."""
    cat.check_precondition("long_blocks")
    _set_shift(monkeypatch, 9)
    inp = cat.build("long_blocks")
    for strip in (False, True):
        assert jl.optimize_batch([inp.data], strip) == [cat.oracle("long_blocks", strip)]


@pytest.mark.parametrize("where,shift,eoi", [("block", 9, True), ("code", 9, True), ("magnitude", 9, True), ("code", None, False), ("magnitude", 11, True)])
def test_one_batch_of_good_and_bad_files(where, shift, eoi, monkeypatch):
    """Holes in a batch: a progressive file (refused on the host) and a DRI = 0 file cut inside subsequence 300 or later -- the failing
    lane sits in the second workgroup of its scan -- between good files of both kinds, two more DRI = 0 files behind them.  Good files
    get the oracle's bytes, bad ones its exception class: the subsequence offsets, the raw offsets, the totals and the stuffing
    descriptors are indexed across the holes."""
    cut, sub = cat.truncated("subs_le_1024", where, eoi=eoi)
    assert sub >= 300
    names = ["zero_64x64", "ff_gray", "ff_gray_dri5", None, None, "subs_le_256", "long_blocks"]
    files = [cat.build(n).data if n else None for n in names]
    files[3], files[4] = read_jpeg("progress.jpg"), cut
    _set_shift(monkeypatch, shift)
    b = jl.OptimizeBatch().upload(files, False).run()
    try:
        for i, (n, f) in enumerate(zip(names, files)):
            if n:
                ref = cat.oracle(n, False)
                assert isinstance(ref, bytes)
            else:
                with pytest.raises(po.OracleError) as e:
                    po.optimize(f, False)
                ref = e.value
            _same_as_oracle(_outcome(b, i), ref, (i, n))
    finally:
        b.close()
