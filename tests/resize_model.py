"""The model of the resize stage (jpgpu_batch_set_resize) that its tests share: numpy only, nothing of the library's code.

Separable antialiased bilinear resampling, a triangle filter widened by the scale when shrinking.  For an axis of input length I and output
length O, all in IEEE double:

    scale = I / O;  sup = max(scale, 1.0)
    for o in 0 .. O-1:
        c  = (o + 0.5) * scale
        lo = max(0, int(c - sup + 0.5));  hi = min(I, int(c + sup + 0.5))          (int: truncation toward zero)
        w64[k] = max(0.0, 1.0 - abs((k + lo - c + 0.5) / sup))   for k in 0 .. hi-lo-1
        w[k]   = float32(w64[k] / sum(w64))                        (the sum in ascending k)

A plane u (uint8, h x w) -> oh x ow: a horizontal pass, then a vertical pass, each  acc = 0.0f; for k ascending: t = w[k] * x; acc = acc + t
with every multiply and every add rounded to float32 on its own; x is float32(u) in the first pass and the first pass's result in the second.
v being the second pass's result:  U8 = clamp(rint(v), 0, 255), ties to even;  F32 = (v * scale[c]) + bias[c], two roundings;  F16 = that
rounded to nearest even to binary16."""
import numpy as np


def axis_table(in_len, out_len):
    """-> (lo int[O], count int[O], [float32 weights of output o], [the same weights before their rounding, float64])"""
    scale = float(in_len) / float(out_len)
    sup = max(scale, 1.0)
    los, counts, weights, exact = [], [], [], []
    for o in range(out_len):
        c = (o + 0.5) * scale
        lo, hi = max(0, int(c - sup + 0.5)), min(in_len, int(c + sup + 0.5))
        w64 = [max(0.0, 1.0 - abs((k + lo - c + 0.5) / sup)) for k in range(hi - lo)]
        total = 0.0
        for w in w64:  # ascending k
            total = total + w
        los.append(lo)
        counts.append(hi - lo)
        exact.append(np.array([w / total for w in w64], dtype=np.float64))
        weights.append(exact[-1].astype(np.float32))
    return np.array(los, np.int64), np.array(counts, np.int64), weights, exact


def _pass_last_axis(x, table, dtype):
    """x[..., I] -> [..., O] along the last axis; dtype float32: the definition's arithmetic, float64: the same sums without any rounding to
    float32 (the weights' included)"""
    los, counts, weights = table[0], table[1], table[2 if np.dtype(dtype) == np.float32 else 3]
    out = np.zeros(x.shape[:-1] + (len(los),), dtype=dtype)
    for o, (lo, n, w) in enumerate(zip(los, counts, weights)):
        acc = np.zeros(x.shape[:-1], dtype=dtype)
        for k in range(int(n)):
            t = w[k] * x[..., lo + k]  # one rounding
            acc = acc + t                            # one rounding
        out[..., o] = acc
    return out


def resample(planes, oh, ow, dtype=np.float32):
    """uint8[..., h, w] -> dtype[..., oh, ow]: the second pass's result v (before the sample is formed)"""
    x = np.asarray(planes).astype(dtype)
    h, w = x.shape[-2:]
    hor = _pass_last_axis(x, axis_table(w, ow), dtype)                                          # [..., h, ow]
    ver = _pass_last_axis(np.swapaxes(hor, -1, -2), axis_table(h, oh), dtype)                   # [..., ow, oh]
    return np.ascontiguousarray(np.swapaxes(ver, -1, -2))


def max_taps(in_len, out_len):
    return int(axis_table(in_len, out_len)[1].max())


def sample(v, np_dtype, scale=None, bias=None):
    """float32[3, oh, ow] -> the samples of np_dtype (np.uint8, np.float16, np.float32)"""
    v = np.asarray(v, np.float32)
    if np.dtype(np_dtype) == np.uint8:
        return np.clip(np.rint(v), 0.0, 255.0).astype(np.uint8)
    s = np.ones(3, np.float32) if scale is None else np.asarray(scale, np.float32)
    b = np.zeros(3, np.float32) if bias is None else np.asarray(bias, np.float32)
    with np.errstate(over="ignore"):  # (overflow to infinity is part of the definition)
        return ((v * s.reshape(3, 1, 1)).astype(np.float32) + b.reshape(3, 1, 1)).astype(np.float32).astype(np_dtype)


def model(u8_planes, oh, ow, np_dtype, scale=None, bias=None):
    """uint8[3, h, w] -> np_dtype[3, oh, ow]: what the resize stage writes for an image whose RGB_PLANAR_U8 output is u8_planes"""
    return sample(resample(u8_planes, oh, ow), np_dtype, scale, bias)
