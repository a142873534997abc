"""One JpegDecoder used for several inputs, the part that needs no device (JpegDecoder(host_only=True)).

The reference keeps its Huffman and quantisation tables across SetInput: SetInput clears the frame header and the restart interval and
nothing else (JpegDecoder.cs:56-62), and the tables go only with ResetTables (:960-965).  Reset() is ResetInput, ResetHeader, ResetTables
and ResetOutputWriter together (:930-936).  The abbreviated file the GPU half decodes with the first file's tables is proven here to be
one: its table payloads are the first file's."""
import numpy as np
import pytest

import jpeglibrary_amd as jl
import reuse_cases as rc
from oracle import pyoracle as po
from tools import jpegsynth


def _decoder():
    return jl.JpegDecoder(host_only=True)


def test_set_input_forgets_the_frame_header_and_the_restart_interval():
    """JpegDecoder.cs:60-61"""
    a, b = rc.mirror_a(), rc.black_gray()
    d = _decoder()
    d.SetInput(a)
    d.Identify()
    assert (d.Width, d.Height, d.NumberOfComponents, d.GetRestartInterval()) == (112, 80, 3, 4)
    d.SetInput(b)
    with pytest.raises(jl.InvalidOperationException, match=r"Call Identify\(\)"):
        d.Width
    assert d.GetRestartInterval() == 0
    d.Identify()
    assert (d.Width, d.Height, d.NumberOfComponents, d.GetRestartInterval()) == (72, 48, 1, 0)  # (b has no DRI: a's interval is not b's)
    d.close()


def test_reset_header_does_the_same_without_a_new_input():
    """:949-955"""
    d = _decoder()
    d.SetInput(rc.mirror_a())
    d.Identify()
    d.ResetHeader()
    for name in ("Width", "Height", "Precision", "NumberOfComponents"):
        with pytest.raises(jl.InvalidOperationException, match=r"Call Identify\(\)"):
            getattr(d, name)
    assert d.GetRestartInterval() == 0
    d.Identify()  # (the input is still there)
    assert (d.Width, d.GetRestartInterval()) == (112, 4)
    d.close()


def test_reset_tables_takes_the_quantisation_tables_away():
    """:960-965; TryEstimateQuanlity without tables is false"""
    d = _decoder()
    d.SetInput(rc.mirror_a())
    d.Identify(True)
    ok, q = d.TryEstimateQuanlity()
    assert ok and q == po.identify(rc.mirror_a(), True)[1]
    d.ResetTables()
    assert d.TryEstimateQuanlity()[0] is False
    assert d.Width == 112  # (the header is not the tables')
    d.close()


def test_reset_is_the_four_resets_together():
    """:930-936"""
    d = _decoder()
    d.SetInput(rc.mirror_a())
    d.Identify(True)
    d.Reset()
    with pytest.raises(jl.InvalidOperationException, match=r"Call Identify\(\)"):
        d.Width
    assert d.GetRestartInterval() == 0 and d.TryEstimateQuanlity()[0] is False
    with pytest.raises(jl.InvalidOperationException, match="Input buffer is not specified"):
        d.Identify()
    d.ResetInput()  # (and each of them alone, on a decoder that has nothing: no error)
    d.ResetOutputWriter()
    d.SetInput(rc.mirror_a())
    d.Identify()
    assert d.Width == 112
    d.close()


def test_the_second_identify_estimates_the_second_files_quality():
    a = bytes(jpegsynth.encode(40, 24, "420", 50, 0, seed=1))
    b = bytes(jpegsynth.encode(40, 24, "420", 90, 0, seed=2))
    want_a, want_b = po.identify(a, True)[1], po.identify(b, True)[1]
    assert want_a != want_b
    d = _decoder()
    d.SetInput(a)
    d.Identify(True)
    assert d.TryEstimateQuanlity() == (True, want_a)
    d.SetInput(b)
    d.Identify(True)
    assert d.TryEstimateQuanlity() == (True, want_b)
    d.close()


def test_the_abbreviated_file_was_written_with_the_first_files_tables():
    """the precondition of test_batch_reuse_gpu.py's abbreviated decode, from the bytes alone"""
    a, b = rc.mirror_a(), rc.mirror_b()
    assert a != b and len(rc.table_payloads(a)) >= 2 and rc.table_payloads(a) == rc.table_payloads(b)
    short = rc.without_tables(b)
    assert rc.table_payloads(short) == [] and len(short) == len(b) - sum(len(p) + 4 for p in rc.table_payloads(b))
    assert short[rc.entropy_start(short):] == b[rc.entropy_start(b):]
    assert [m for m, _, _ in rc.header_segments(short)] == [m for m, _, _ in rc.header_segments(b) if m not in (0xDB, 0xC4)]
    # on its own it has no tables: the oracle, a fresh decoder, refuses it as the reference's scan decoder does
    with pytest.raises(po.OracleError, match="is not defined"):
        po.decode_8bit(short)
    d = _decoder()
    d.SetInput(short)
    d.Identify(True)
    assert (d.Width, d.Height) == (72, 56) and d.TryEstimateQuanlity()[0] is False
    d.close()
    assert np.array_equal(po.decode_8bit(b)[0].shape, (56, 72, 3))
