"""The model of RGB_PLANAR_F16 / _F32 that the float sink's tests share, and the constant sets they run it with.

Sample (c, y, x) from the byte u RGB_PLANAR_U8 holds there: t = float32(u) * float32(scale[c]), v = t + float32(bias[c]), each one IEEE
float32 operation rounded to nearest even and never fused; F32 is v, F16 is v rounded to nearest even to binary16 (subnormals kept,
overflow to infinity).  numpy computes exactly that."""
import numpy as np

from jpeglibrary_amd import affine_from_mean_std


def model(u8_planes, scale, bias, dtype):
    """uint8[3, H, W] -> dtype[3, H, W]"""
    s = np.asarray(scale, np.float32).reshape(3, 1, 1)
    b = np.asarray(bias, np.float32).reshape(3, 1, 1)
    with np.errstate(over="ignore"):  # (overflow to infinity is part of the definition)
        return (u8_planes.astype(np.float32) * s + b).astype(dtype)


DEFAULT = (np.ones(3, np.float32), np.zeros(3, np.float32))
# what model code asks for: (u / 255 - mean) / std with the ImageNet statistics, three distinct scales and biases
IMAGENET = affine_from_mean_std([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
# a negative scale, a scale above one and a small one; biases of both signs -- no two channels alike, none trivial
NEGATIVE = (np.array([-0.75, 1.5, 0.003], np.float32), np.array([100.25, -3.5, 0.1], np.float32))
# the edges of binary16, chosen with the model above (tests/test_float_sink_cpu.py holds the set to these statements):
#   channel 0, 2^-25 u: every result is a binary16 subnormal (below 2^-14) or zero, the subnormals step by 2^-24, so every odd u is an
#              exact tie between two of them and goes to the even one
#   channel 1, u + 1800: from 2048 on binary16 steps by 2, so u = 249, 251, 253, 255 (2049, 2051, 2053, 2055) are exact ties
#   channel 2, 300 u - 100: negative at u = 0, beyond binary16's largest finite value from u = 219 on (65 600 >= 65 520): +inf
TIES = (np.array([2.0 ** -25, 1.0, 300.0], np.float32), np.array([0.0, 1800.0, -100.0], np.float32))
