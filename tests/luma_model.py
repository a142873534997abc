"""The model of grey output (include/jpgpu.h, "Grey output") that its tests share.

The sample of a pixel: component 0's byte for the kinds "gray" and "ycbcr"; for "rgb", "cmyk" and "ycck" L = (19595 R + 38470 G + 7471 B + 32768) >> 16
of the RGB bytes color_model.model gives -- Pillow's convert("L"), which tests/test_luma_cpu.py checks.  The plane is turned through
orient_model, cut to the window (given in pixels of the oriented frame) and, for the float forms, taken through the affine step of
float_sink_model with scale[0] and bias[0]."""
import numpy as np

import color_model as cm
import orient_model as om


def L(rgb):
    """uint8[..., 3] -> uint8[...]"""
    rgb = np.asarray(rgb).astype(np.uint32)
    return ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 32768) >> 16).astype(np.uint8)


def gray(kind, samples):
    """uint8[H, W, C] INTERLEAVED_U8 samples of the stored frame -> uint8[H, W]"""
    samples = np.asarray(samples, dtype=np.uint8)
    if kind in ("gray", "ycbcr"):
        return np.ascontiguousarray(samples[..., 0])
    return L(cm.model(kind, samples))


def plane(kind, samples, window=None, orientation=1):
    """-> uint8[1, h, w]: what RGB_PLANAR_U8 holds under "gray"; window = (x, y, w, h) in pixels of the oriented frame"""
    g = om.orient(orientation, gray(kind, samples))
    if window is not None:
        x, y, w, h = window
        g = g[y:y + h, x:x + w]
    return np.ascontiguousarray(g)[None]


def as_dtype(u8_plane, np_dtype, scale0=1.0, bias0=0.0):
    """uint8[1, h, w] -> the samples of np_dtype: (float32(u) * scale[0] + bias[0]) rounded as float_sink_model.model rounds"""
    if np.dtype(np_dtype) == np.uint8:
        return u8_plane
    with np.errstate(over="ignore"):
        return (u8_plane.astype(np.float32) * np.float32(scale0) + np.float32(bias0)).astype(np_dtype)
