"""RGB_PLANAR_F16 / _F32 without a GPU: the new names, affine_from_mean_std, the numpy model the GPU suite compares against, restated with
Python floats and exact fractions on all 256 bytes for every constant set that suite uses, and _DeviceView's typestr."""
import ctypes as C
import struct
from fractions import Fraction

import numpy as np
import pytest

import jpeglibrary_amd as jl
from float_sink_model import DEFAULT, IMAGENET, NEGATIVE, TIES, model
from jpeglibrary_amd import _capi
from jpeglibrary_amd import batch as jb


def test_the_new_names_exist():
    assert (_capi.FMT_RGB_PLANAR_F16, _capi.FMT_RGB_PLANAR_F32) == (8, 9) == (jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_PLANAR_F32)
    f = _capi.lib.jpgpu_batch_set_output_affine
    assert f.restype == C.c_int and len(f.argtypes) == 3
    assert callable(jl.Batch.set_output_affine) and callable(jl.affine_from_mean_std)
    assert f(None, None, None) == _capi.ERR_ARGUMENT  # (no batch: refused before anything is read)


def test_affine_from_mean_std_is_the_float64_value_rounded_once():
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    scale, bias = jl.affine_from_mean_std(mean, std)
    assert scale.dtype == np.float32 and bias.dtype == np.float32 and scale.shape == (3,) == bias.shape
    for c in range(3):
        assert scale[c] == np.float32(1.0 / (255.0 * std[c])) and bias[c] == np.float32(-mean[c] / std[c])
        # ... which is what the consumer's own expression gives, to float32's precision, on every byte
        u = np.arange(256, dtype=np.float64)
        want = (u / 255.0 - mean[c]) / std[c]
        got = u * np.float64(scale[c]) + np.float64(bias[c])
        assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()
    for bad in (([0.5, 0.5], [1, 1, 1]), ([0.5] * 3, [1, 0, 1]), ([np.nan, 0, 0], [1, 1, 1]), ([0, 0, 0], [1, np.inf, 1])):
        with pytest.raises(ValueError):
            jl.affine_from_mean_std(*bad)


def _f32(x):
    """a Python float (or exact Fraction) rounded to float32, to nearest even -- struct does the rounding for floats; a Fraction is rounded here"""
    if isinstance(x, Fraction):
        if x == 0:
            return 0.0
        sign, x = (-1 if x < 0 else 1), abs(x)
        e = max(x.numerator.bit_length() - x.denominator.bit_length(), -126 - 1)
        while Fraction(2) ** e > x:
            e -= 1
        while Fraction(2) ** (e + 1) <= x:
            e += 1
        e = max(e, -126)
        q = x / Fraction(2) ** (e - 23)  # in units of the last place
        n = q.numerator // q.denominator
        rest = q - n
        if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
            n += 1
        return sign * float(Fraction(n) * Fraction(2) ** (e - 23))
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _f16_bits(v):
    """a float32 value (held in a Python float) -> binary16 bits, round to nearest even, subnormals kept, overflow to infinity; exact arithmetic"""
    if v != v:
        return 0x7E00
    sign = 0x8000 if (v < 0 or (v == 0 and str(v).startswith("-"))) else 0
    x = Fraction(abs(v))
    if x == 0:
        return sign
    e = -14
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    q = x / Fraction(2) ** (e - 10)  # units of the last place at exponent e (e = -14 for subnormals)
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    if n >= 2048:
        n, e = n // 2, e + 1
    if e > 15:
        return sign | 0x7C00
    if n < 1024:  # subnormal (only at e = -14)
        return sign | n
    return sign | ((e + 15) << 10) | (n - 1024)


@pytest.mark.parametrize("name,consts", [("default", DEFAULT), ("imagenet", IMAGENET), ("negative", NEGATIVE), ("ties", TIES)])
def test_the_numpy_model_is_two_rounded_float32_steps_and_one_rounding_to_binary16(name, consts):
    scale, bias = consts
    u = np.arange(256, dtype=np.uint8).reshape(1, 1, 256).repeat(3, axis=0)
    m32, m16 = model(u, scale, bias, np.float32), model(u, scale, bias, np.float16)
    assert m32.dtype == np.float32 and m16.dtype == np.float16
    for c in range(3):
        s, b = Fraction(float(scale[c])), Fraction(float(bias[c]))
        for v in range(256):
            t = _f32(Fraction(v) * s)           # the product, exact, rounded once
            w = _f32(Fraction(t) + b)           # the sum, exact, rounded once (NOT the fused v * s + b rounded once)
            assert struct.pack("<f", w) == m32[c, 0, v].tobytes(), (name, c, v)
            assert _f16_bits(w) == int(m16[c, 0, v].view(np.uint16)), (name, c, v)


def test_the_tie_set_hits_the_cases_it_is_named_for():
    scale, bias = TIES
    u = np.arange(256, dtype=np.uint8).reshape(1, 1, 256).repeat(3, axis=0)
    m32, m16 = model(u, scale, bias, np.float32)[:, 0], model(u, scale, bias, np.float16)[:, 0]
    bits = m16.view(np.uint16)
    # channel 0: zero or subnormal everywhere (exponent field 0); every odd byte an exact tie that went to the even neighbour
    assert ((bits[0] & 0x7C00) == 0).all() and (m16[0, 2:] > 0).all() and m16[0, 1] == 0  # (2^-25 itself ties to zero)
    for v in range(1, 256, 2):
        exact = Fraction(v, 2 ** 25) / Fraction(1, 2 ** 24)  # in subnormal steps: v / 2
        assert exact.denominator == 2 and int(bits[0, v]) in (v // 2, v // 2 + 1) and int(bits[0, v]) % 2 == 0, v
    assert [int(x) for x in bits[0, :6]] == [0, 0, 1, 2, 2, 2]
    # channel 1: exact in float32; the odd values from 2049 on are ties and go to the multiple of 4
    assert (m32[1] == np.arange(256) + 1800).all()
    assert [float(m16[1, v]) for v in (248, 249, 250, 251, 252, 253, 254, 255)] == [2048, 2048, 2050, 2052, 2052, 2052, 2054, 2056]
    # channel 2: negative at 0, finite up to 218, +inf from 219 on
    assert m16[2, 0] == -100 and np.isfinite(m16[2, :219]).all() and (np.isposinf(m16[2, 219:])).all() and np.isfinite(m32[2]).all()
    # the default constants are the byte as a float, exactly, in both types
    for dt in (np.float16, np.float32):
        assert np.array_equal(model(u, *DEFAULT, dt).astype(np.float64), u.astype(np.float64))
    # a fused multiply-add would differ from the model somewhere on the ImageNet set (so the GPU suite can tell): count the bytes
    s, b = IMAGENET
    fused = sum(_f32(Fraction(v) * Fraction(float(s[c])) + Fraction(float(b[c]))) != float(model(u, s, b, np.float32)[c, 0, v]) for c in range(3) for v in range(256))
    assert fused > 0, fused


def test_device_view_carries_the_typestr_of_the_format():
    assert jb._typestr(jl.FMT_RGB_PLANAR_F16) == "<f2" and jb._typestr(jl.FMT_RGB_PLANAR_F32) == "<f4"
    for fmt in (jl.FMT_INTERLEAVED_U8, jl.FMT_RGB_U8, jl.FMT_RGBA_U8, jl.FMT_RGB_PLANAR_U8, jl.FMT_INTERLEAVED_U8_SCALED):
        assert jb._typestr(fmt) == "|u1"
    v = jb._DeviceView(None, 4096, (3, 5, 7), jb._typestr(jl.FMT_RGB_PLANAR_F16))
    assert v.__cuda_array_interface__ == {"shape": (3, 5, 7), "typestr": "<f2", "data": (4096, False), "version": 2, "strides": None}
    assert jb._DeviceView(None, 4096, (5, 7, 3)).__cuda_array_interface__["typestr"] == "|u1"  # (the default: every earlier caller)
