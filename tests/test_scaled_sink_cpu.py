"""The two precision-scaled buffer writers of the decoder mirror (JpegBufferOutputWriterLessThan8Bit / GreaterThan8Bit) against a
literal model of the reference's loops (scaled_sink_model), the model against the worked values of the issue, and -- with the
oracle alone, no GPU -- that the frames tests/test_scaled_sink_gpu.py hands to K3 reach every regime of the writers."""
import numpy as np
import pytest

import jpeglibrary_amd as jl
import scaled_sink_model as sm

EDGES = [-32768, -1, 0, 32767]


def test_the_format_constant_and_the_binding_exist():
    assert jl.FMT_INTERLEAVED_U8_SCALED == 6
    assert hasattr(jl._capi.lib, "jpgpu_decoder_set_output_buffer8_scaled")
    assert "jpgpu_decoder_set_output_buffer8_scaled" in [s[0] for s in jl._capi.SYMBOLS]


@pytest.mark.parametrize("p,v,byte", [(1, 1, 255), (2, 2, 0xAA), (3, 5, 181), (4, 9, 0x99), (5, 22, 182), (6, 33, 133), (7, 64, 128), (7, 127, 255)])
def test_the_model_reproduces_the_worked_values(p, v, byte):
    assert sm.expand_bits(v, p) == byte
    assert sm.less_than_8bit_byte(v, p) == byte and sm.decode_action_byte(v, p) == byte


def test_the_model_at_the_clamps():
    for p in range(1, 8):
        mx = (1 << p) - 1
        assert sm.less_than_8bit_byte(-1, p) == 0 and sm.less_than_8bit_byte(0, p) == 0  # a signed clamp: -1 is not the maximum
        assert sm.less_than_8bit_byte(mx, p) == 255 and sm.less_than_8bit_byte(mx + 1, p) == 255 and sm.less_than_8bit_byte(32767, p) == 255
    for p in range(9, 17):
        s = p - 8
        assert sm.greater_than_8bit_byte(-1, p) == 0 and sm.greater_than_8bit_byte(-32768, p) == 0  # -1 >> s = -1: arithmetic
        assert sm.greater_than_8bit_byte((1 << s) - 1, p) == 0 and sm.greater_than_8bit_byte(1 << s, p) == 1
        assert sm.greater_than_8bit_byte(min((256 << s) - 1, 32767), p) == min(255, 32767 >> s)
        if (256 << s) <= 32767:
            assert sm.greater_than_8bit_byte(256 << s, p) == 255
    assert [sm.decode_action_byte(v, 8) for v in (-1, 0, 255, 256)] == [0, 0, 255, 255]
    # the closed form the kernel may use, held against the loops for every value of every precision below 8
    for p, m, rem in zip(range(1, 8), (255, 0x55, 9, 0x11, 1, 1, 1), (0, 0, 2, 0, 3, 2, 1)):
        for v in range(1 << p):
            r = v * m
            assert sm.expand_bits(v, p) == ((r << rem) | (r & ((1 << rem) - 1))) and r < 256


def _writers(p):
    out = []
    if p <= 8:
        out.append((jl.JpegBufferOutputWriterLessThan8Bit, sm.less_than_8bit_byte))
    if p >= 8:
        out.append((jl.JpegBufferOutputWriterGreaterThan8Bit, sm.greater_than_8bit_byte))
    return out


@pytest.mark.parametrize("p", range(1, 17))
def test_write_block_equals_the_model(p):
    rng = np.random.default_rng(p)
    mx = min((1 << p) - 1, 32767)  # (the samples are int16)
    w, h, cc = 21, 13, 4  # neither a multiple of 8; componentCount above the component indices used (0..2)
    for cls, to_byte in _writers(p):
        got = cls(w, h, p, cc, np.zeros(w * h * cc, np.uint8))
        want = sm.ModelWriter(w, h, p, cc, to_byte)
        for y in range(0, 24, 8):  # y = 16 > h: the early return; y = 8: clipped at the bottom
            for x in range(0, 32, 8):  # x = 24 > w: the early return; x = 16: clipped at the right
                for ci in range(3):
                    blk = rng.integers(-32768, 32768, 64).astype(np.int16)
                    blk[rng.integers(0, 64, 24)] = rng.choice(np.array(EDGES + [mx, min(mx + 1, 32767)]), 24)
                    blk[rng.integers(0, 64, 16)] = rng.integers(-2, mx + 3, 16).clip(-32768, 32767)
                    got.WriteBlock(blk.copy(), ci, x, y)
                    want.WriteBlock(blk, ci, x, y)
        assert np.array_equal(got.output, want.output), (cls.__name__, int((got.output != want.output).sum()))
        assert want.output.reshape(h, w, cc)[..., 3].max() == 0 and want.output.reshape(h, w, cc)[..., :3].any()
    # x == width and y == height are NOT early returns (`>`): nothing is written (writeWidth = 0), nothing raises
    for cls, _ in _writers(p):
        wr = cls(16, 8, p, 1, np.zeros(16 * 8, np.uint8))
        wr.WriteBlock(np.full(64, mx, np.int16), 0, 16, 0)
        wr.WriteBlock(np.full(64, mx, np.int16), 0, 0, 8)
        assert not wr.output.any()


def test_every_sample_value_through_both_classes():
    """one block per 64 consecutive int16 values would be 1024 blocks per precision; the edges and a stride through the rest"""
    vals = np.unique(np.concatenate([np.arange(-32768, 32768, 97), np.arange(-300, 70000, 1).clip(-32768, 32767), np.array(EDGES)])).astype(np.int16)
    vals = np.concatenate([vals, np.zeros(-len(vals) % 64, np.int16)]).reshape(-1, 64)
    for p in (1, 3, 5, 7, 8, 9, 12, 16):
        for cls, to_byte in _writers(p):
            wr = cls(8, 8 * len(vals), p, 1, np.zeros(64 * len(vals), np.uint8))
            for i, blk in enumerate(vals):
                wr.WriteBlock(blk, 0, 0, 8 * i)
            want = np.array([to_byte(int(v), p) for v in vals.reshape(-1)], np.uint8)
            assert np.array_equal(wr.output, want), (p, cls.__name__)


def test_constructor_exceptions():
    buf = np.zeros(8 * 8 * 3, np.uint8)
    for cls in (jl.JpegBufferOutputWriterLessThan8Bit, jl.JpegBufferOutputWriterGreaterThan8Bit):
        with pytest.raises(jl.ArgumentException, match="Destination buffer is too small."):
            cls(8, 8, 8, 4, buf)
        with pytest.raises(jl.ArgumentException, match="Destination buffer is too small."):
            cls(8, 9, 99, 3, buf)  # the buffer is checked first
        cls(8, 8, 8, 3, buf)  # precision 8 is accepted by both (`> 8` / `< 8`)
    with pytest.raises(jl.ArgumentException, match="precision"):
        jl.JpegBufferOutputWriterLessThan8Bit(8, 8, 9, 3, buf)
    with pytest.raises(jl.ArgumentException, match="precision"):
        jl.JpegBufferOutputWriterGreaterThan8Bit(8, 8, 7, 3, buf)
    for p in (0, -1):  # the reference would accept these and never return from ExpandBits
        with pytest.raises(jl.ArgumentException, match="precision"):
            jl.JpegBufferOutputWriterLessThan8Bit(8, 8, p, 3, buf)
    assert jl.JpegBufferOutputWriterLessThan8Bit(8, 8, 1, 3, buf).precision == 1
    assert jl.JpegBufferOutputWriterGreaterThan8Bit(8, 8, 16, 3, buf).precision == 16
    assert issubclass(jl.JpegBufferOutputWriterLessThan8Bit, jl.JpegBlockOutputWriter)


@pytest.mark.parametrize("p", range(1, 17))
def test_the_gpu_tests_frames_reach_every_regime_of_the_writers(p):
    """On the oracle's planes alone: every (P, geometry) case of the frame hand-off test has visible samples below 0, inside the
    range and above the maximum (where an int16 can be: P <= 14), and for P > 8 negative samples whose shift is not exact."""
    cases, planes = sm.precision_cases(p)
    sm.assert_covered(cases, planes)


@pytest.mark.parametrize("p", [12, 5])
def test_the_geometry_matrix_reaches_every_regime_too(p):
    """... and so does every geometry of the layout matrix that has at least 1024 pixels (a 1 x 1 image shows one sample of each
    component), and the matrix as a whole"""
    cases, planes = sm.matrix_cases(p)
    sm.assert_covered(cases, planes, per_case_from=sm.MATRIX_COVERED_FROM)
