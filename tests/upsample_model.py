"""The numpy model of the upsampling policy "fancy" (include/jpgpu.h, "Chroma upsampling") that the upsampling tests share: libjpeg's triangle
filter for h2v1, h2v2 and h1v2 chroma, in integers, with the taps clamped to the plane that is handed in.

    upsample(C, hs, vs, W, H)   a native chroma plane uint8[ch, cw] -> uint8[H, W]; the taps clamp to C's own extent, so the caller decides
                                whether that is the REAL extent ceil(W / hs) x ceil(H / vs) (what libjpeg does) or a padded plane
    replicate(C, hs, vs, W, H)  the same plane by sample replication
    filtered(I, hs, vs)         the INTERLEAVED_U8 decode uint8[H, W, 3] of a file -> the (Y, Cb', Cr') the policy defines, uint8[H, W, 3]:
                                the native samples are I[j * vs][i * hs]; an image the rule does not filter comes back as it is
                                (RGB and the format variants come from color_model.model("ycbcr") and color_model.as_format)
    sof_sampling(f)             (W, H, precision, [(h, v)]) of a file's frame header; qualifies(f) the rule on it (a YCbCr file assumed)
    fetch_span / fetch_rect     the rectangle of the stored frame the taps of a window touch, as jpeglibrary_amd/csrc/k3u_taps.h states it

Only numpy and Pillow are imported here."""
import struct

import numpy as np

RATIOS = ((2, 1), (2, 2), (1, 2))


def chroma_extent(size, step):
    return (size + step - 1) // step


def ratio_filtered(hs, vs, width):
    """the ratio is one of the three, and for hs == 2 the chroma plane is more than two samples wide"""
    return (hs, vs) in RATIOS and (hs != 2 or chroma_extent(width, 2) > 2)


def taps(p, extent):
    """pixel coordinates p of an axis subsampled by two -> (near, far, even): far = near - 1 for even p, near + 1 for odd p, clamped"""
    p = np.asarray(p, dtype=np.int64)
    near = p >> 1
    even = (p & 1) == 0
    far = np.clip(np.where(even, near - 1, near + 1), 0, extent - 1)
    return near, far, even


def upsample(C, hs, vs, W, H):
    C = np.asarray(C).astype(np.int64)
    ch, cw = C.shape
    x, y = np.arange(W), np.arange(H)
    if vs == 2:
        j, jf, y_even = taps(y, ch)
        s = 3 * C[j] + C[jf]  # [H, cw], unrounded
        rb = np.where(y_even, 1, 2)[:, None]
    else:
        s = C[y]
    if hs == 2:
        i, i_far, x_even = taps(x, cw)
        if vs == 2:
            out = (3 * s[:, i] + s[:, i_far] + np.where(x_even, 8, 7)[None, :]) >> 4
        else:
            out = (3 * s[:, i] + s[:, i_far] + np.where(x_even, 1, 2)[None, :]) >> 2
    else:
        out = (s[:, x] + rb) >> 2 if vs == 2 else s[:, x]
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def replicate(C, hs, vs, W, H):
    C = np.asarray(C)
    return np.ascontiguousarray(C[np.arange(H) // vs][:, np.arange(W) // hs])


def filtered(I, hs, vs):
    I = np.asarray(I)
    H, W = I.shape[:2]
    if I.ndim != 3 or I.shape[2] != 3 or not ratio_filtered(hs, vs, W):
        return I.copy()
    out = I.copy()
    for c in (1, 2):
        out[..., c] = upsample(I[::vs, ::hs, c], hs, vs, W, H)  # (the slice has the real extent: ceil(H / vs) x ceil(W / hs))
    return out


def sof(f):
    """offset of the frame header's marker in f"""
    pos = 2
    while True:
        assert f[pos] == 0xFF, pos
        m = f[pos + 1]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return pos
        pos += 2 + struct.unpack(">H", f[pos + 2:pos + 4])[0]


def sof_sampling(f):
    a = sof(f)
    precision, H, W, n = f[a + 4], struct.unpack(">H", f[a + 5:a + 7])[0], struct.unpack(">H", f[a + 7:a + 9])[0], f[a + 9]
    return W, H, precision, [(f[a + 11 + 3 * c] >> 4, f[a + 11 + 3 * c] & 15) for c in range(n)]


def ratio(f):
    """(hs, vs) of a three-component file whose component 0 carries the maximal factors and whose components 1 and 2 agree, else None"""
    _, _, _, hv = sof_sampling(f)
    if len(hv) != 3 or hv[1] != hv[2]:
        return None
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    if hv[0] != (hmax, vmax) or hmax % hv[1][0] or vmax % hv[1][1]:
        return None
    return hmax // hv[1][0], vmax // hv[1][1]


def qualifies(f):
    """is a file whose three components are YCbCr filtered under the policy"""
    W, _, precision, _ = sof_sampling(f)
    r = ratio(f)
    return r is not None and precision == 8 and ratio_filtered(r[0], r[1], W)


def patch_sof(f, width=None, height=None, luma=None):
    """the frame header's size and component 0's factors byte, the rest of the file as it is"""
    a = sof(f)
    out = bytearray(f)
    if height is not None:
        out[a + 5:a + 7] = struct.pack(">H", height)
    if width is not None:
        out[a + 7:a + 9] = struct.pack(">H", width)
    if luma is not None:
        out[a + 11] = luma
    return bytes(out)


def fetch_span(p0, p1, size, step):
    """the pixels [p0, p1) of an axis subsampled by step, widened to whole native samples plus one per side, clipped to the frame"""
    if step == 1:
        return p0, p1
    return max(0, (p0 // step - 1) * step), min(size, ((p1 - 1) // step + 2) * step)


def fetch_rect(x, y, w, h, W, H, hs, vs):
    x0, x1 = fetch_span(x, x + w, W, hs)
    y0, y1 = fetch_span(y, y + h, H, vs)
    return x0, y0, x1 - x0, y1 - y0
