"""The numpy model of the scaled decode (include/jpgpu.h, "Scaled decode") that the scaled tests share: libjpeg's reduced transforms
(jidctred.c) in integers that wrap like int32, jdmaster.c's choice of a transform size per component, and the assembly of the reduced
picture.  It stands on islow_model (the 8 x 8 transform, the headers, the colour constants) and upsample_model (the triangle filter).

    block_size(m, h, v, hmax, vmax)     samples per block side of a component, m = 8 // denom: the per-component rule
    component_sizes(m, hv)              [(s, rh, rv)] for the frame's [(h, v)]: the size and the replication that is left
    reduced(coefs, quant, s)            int16[n, 64] zig-zag coefficients, uint16[64] or [n, 64] quantisers -> uint8[n, s, s]; s = 8 is islow
    asserts_in_range(coefs, quant, s)   the same samples, asserting that dequantised and workspace values fit int16 and pass sums int32
    out_size(W, H, denom)               (W', H') = ceil(W * m / 8), ceil(H * m / 8)
    samples(f, denom, blocks=None)      the reduced picture as INTERLEAVED_U8 would hold it, uint8[H', W', C], sub-sampled components replicated
    residual_ratio(f, denom)            (rh, rv) of a three-component file's chroma in the reduced picture, or None (upsample_model.ratio's rule)
    filters(f, denom)                   does upsampling="fancy" filter the reduced picture
    ycc(f, denom, upsampling)           samples -> upsample_model.filtered where the policy filters
    decode(f, denom, upsampling, kind)  ... -> islow_model.rgb: uint8[H', W', 3], what decode_to_tensors(arithmetic="libjpeg", scale=denom) delivers
    pillow_draft(f, denom, mode)        Pillow's draft() decode at that scale in "L", "YCbCr" or "RGB", or None without Pillow

Only numpy, Pillow and the sibling models are imported at module level."""
import io

import numpy as np

import islow_model as im
import upsample_model as um

DENOMS = (2, 4, 8)


def block_size(m, h, v, hmax, vmax):
    s = m
    while s < 8 and (hmax * m) % (h * s * 2) == 0 and (vmax * m) % (v * s * 2) == 0:
        s *= 2
    return s


def component_sizes(m, hv):
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    out = []
    for h, v in hv:
        s = block_size(m, h, v, hmax, vmax)
        out.append((s, hmax * m // (h * s), vmax * m // (v * s)))
    return out


def out_size(W, H, denom):
    m = 8 // denom
    return -(-W * m // 8), -(-H * m // 8)


# ------------------------------------------------------------------------------------------------ the transforms

def _descale(sums, shift, check):
    if check:
        for v in sums:
            assert np.abs(v).max(initial=0) + (1 << (shift - 1)) < (1 << 31), "a pass sum leaves int32"
    return [im.wrap32(im.wrap32(v) + (1 << (shift - 1))) >> shift for v in sums]


def _pass4(d, shift, check):
    """jpeg_idct_4x4's pass: d[k] = input k (k = 4 is never read) -> the four descaled outputs"""
    t0 = d[0] << 14
    t2 = d[2] * 15137 - d[6] * 6270
    t10, t12 = t0 + t2, t0 - t2
    a = -d[7] * 1730 + d[5] * 11893 - d[3] * 17799 + d[1] * 8697
    b = -d[7] * 4176 - d[5] * 4926 + d[3] * 7373 + d[1] * 20995
    if check:
        for v in (t2, a, b):
            assert np.abs(v).max(initial=0) < (1 << 31), "a pass sum leaves int32"
    return _descale([t10 + b, t12 + a, t12 - a, t10 - b], shift, check)


def _pass2(d, shift, check):
    """jpeg_idct_2x2's pass: inputs 0, 1, 3, 5, 7 -> the two descaled outputs"""
    t10 = d[0] << 15
    t0 = -d[7] * 5906 + d[5] * 6967 - d[3] * 10426 + d[1] * 29692
    if check:
        assert np.abs(t0).max(initial=0) < (1 << 31), "a pass sum leaves int32"
    return _descale([t10 + t0, t10 - t0], shift, check)


def _reduced(coefs, quant, s, check):
    if s == 8:
        return im._islow(coefs, quant, check)
    coefs = np.asarray(coefs, dtype=np.int16).reshape(-1, 64).astype(np.int64)
    quant = np.broadcast_to(np.asarray(quant).astype(np.int64).reshape(-1, 64), coefs.shape)
    d = np.zeros(coefs.shape, np.int64)
    d[:, im.NAT_OF_ZIG] = coefs * quant
    if check:
        assert np.abs(d).max(initial=0) < (1 << 15), "a dequantised coefficient leaves int16"
    d = d.reshape(-1, 8, 8)  # [n, row, column]
    if s == 1:
        out = (im.wrap32(d[:, 0, 0] + 4) >> 3).reshape(-1, 1, 1)
    else:
        one, s1, s2 = (_pass4, 12, 19) if s == 4 else (_pass2, 13, 20)
        ws = np.stack(one([d[:, k, :] for k in range(8)], s1, check), axis=1)  # columns: [n, s, 8]
        if check:
            used = [0, 1, 2, 3, 5, 6, 7] if s == 4 else [0, 1, 3, 5, 7]
            assert np.abs(ws[:, :, used]).max(initial=0) < (1 << 15), "a workspace value leaves int16"
        out = np.stack(one([ws[:, :, k] for k in range(8)], s2, check), axis=2)  # rows: [n, s, s]
    return np.clip(im.wrap32(out + 128), 0, 255).astype(np.uint8)


def reduced(coefs, quant, s):
    return _reduced(coefs, quant, s, False)


def asserts_in_range(coefs, quant, s):
    return _reduced(coefs, quant, s, True)


# ------------------------------------------------------------------------------------------------ the reduced picture

def samples(f, denom, check=False, blocks=None):
    """every block through its component's transform, at its place times m / 8, replicated by what is left, clipped to W' x H'.
    blocks: a baseline file's int16[n, 64] in the order of Batch.coefficients, in place of the oracle's"""
    from oracle import pyoracle

    m = 8 // denom
    W, H, progressive, comps = im.frame(f)
    hv = [(c[1], c[2]) for c in comps]
    sizes = component_sizes(m, hv)
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    canvas = np.zeros((my * vmax * m + 4 * m, mx * hmax * m + 4 * m, len(comps)), np.uint8)
    per = {c: ([], []) for c in range(len(comps))}  # component -> (blocks, [(x, y)] in the reduced picture)
    if not progressive:
        blocks = np.asarray(pyoracle.decode_coefficients(f)[0] if blocks is None else blocks).reshape(-1, 64)
        k = 0
        for sc in im.scans(f):
            for mcu in range(mx * my):
                for c in sc:
                    h, v = hv[c]
                    for by in range(v):
                        for bx in range(h):
                            per[c][0].append(blocks[k])
                            per[c][1].append((((mcu % mx) * hmax + bx) * m, ((mcu // mx) * vmax + by) * m))
                            k += 1
        assert k == len(blocks), (k, len(blocks))
        q = im.tables(f)
        quant = {c: q[comps[c][3]] for c in range(len(comps))}
    else:
        _, store, quant = pyoracle.decode_progressive_store(f)
        for c, blocks in store.items():
            s, rh, rv = sizes[c]
            for (bx, by), b in blocks.items():
                if bx * s * rh < canvas.shape[1] - 4 * m and by * s * rv < canvas.shape[0] - 4 * m:
                    per[c][0].append(b)
                    per[c][1].append((bx * s * rh, by * s * rv))
    for c, (blocks, places) in per.items():
        if not blocks:
            continue
        s, rh, rv = sizes[c]
        px = _reduced(np.stack(blocks), quant[c], s, check)
        for (x, y), b in zip(places, px):
            rep = np.repeat(np.repeat(b, rv, axis=0), rh, axis=1)
            canvas[y:y + s * rv, x:x + s * rh, c] = rep[:canvas.shape[0] - y, :canvas.shape[1] - x]
    Wr, Hr = out_size(W, H, denom)
    return np.ascontiguousarray(canvas[:Hr, :Wr])


def residual_ratio(f, denom):
    if len(im.frame(f)[3]) != 3 or um.ratio(f) is None:
        return None
    _, _, _, hv = um.sof_sampling(f)
    _, rh, rv = component_sizes(8 // denom, hv)[1]
    return rh, rv


def filters(f, denom):
    """libjpeg: do_fancy_upsampling && min_DCT_scaled_size > 1, then upsample_model's rule on the reduced picture"""
    W, H, precision, _ = um.sof_sampling(f)
    r = residual_ratio(f, denom)
    return r is not None and precision == 8 and denom < 8 and um.ratio_filtered(r[0], r[1], out_size(W, H, denom)[0])


def ycc(f, denom, upsampling="replicate", check=False):
    s = samples(f, denom, check)
    if upsampling == "fancy" and filters(f, denom):
        s = um.filtered(s, *residual_ratio(f, denom))
    return s


def decode(f, denom, upsampling="replicate", kind=None, check=False):
    s = samples(f, denom, check)
    if kind is None:
        kind = "gray" if s.shape[2] == 1 else "ycbcr"
    if upsampling == "fancy" and kind == "ycbcr" and filters(f, denom):
        s = um.filtered(s, *residual_ratio(f, denom))
    return im.rgb(kind, s)


def pillow_draft(f, denom, mode="RGB", strict=True):
    """Pillow's decode at 1 / denom: draft() asked for (w * m // 8, h * m // 8) -- the ceiling would make it pick the next larger scale.
    Pillow picks a scale by min(w // asked w, h // asked h): a frame with a side below denom pixels does not get 1 / denom from it, which is
    an AssertionError, or None under strict=False"""
    try:
        from PIL import Image
    except ImportError:
        return None
    img = Image.open(io.BytesIO(f))
    m = 8 // denom
    w, h = img.size
    native = "L" if img.mode == "L" else ("YCbCr" if mode == "YCbCr" else "RGB")
    if img.mode == "CMYK":
        native = "CMYK"
    img.draft(native, (max(1, w * m // 8), max(1, h * m // 8)))
    if not strict and img.size != out_size(w, h, denom):
        return None
    assert img.size == out_size(w, h, denom), (img.size, (w, h), denom)
    return np.asarray(img if img.mode == mode else img.convert(mode))
