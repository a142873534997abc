"""Encoding from pixels that are on the device already (jpgpu_encoder_upload_device / _upload_described_device, EncodeBatch.upload_tensors /
upload_described_tensors / output_tensor, encode_tensors): interleaved (H, W, C) and planar (C, H, W) torch tensors, read where they are.

Every expectation is byte equality: coefficients and streams against the oracle's encoder (po.encode_8bit), described arrangements against
the host upload of the same pixels (test_encoder_components_gpu.py pins that one to the model).  The shapes are test_gpu_parity's
FUSED_SHAPES -- the branches fdct_fused_kernel picks between -- and, because the alignment of a caller's pointer is the caller's, the same
images at addresses that are multiples of 1, 4 and 8 only."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import encoder_arrangements as ea
import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from oracle import pyoracle as po
from test_gpu_parity import FUSED_SHAPES, _enc_image, _rgba
from tools import jpegsynth

pytestmark = pytest.mark.gpu
_lib = _capi.lib
ERR_ARGUMENT = _capi.ERR_ARGUMENT
INTERLEAVED, PLANAR = _capi.PIXELS_INTERLEAVED, _capi.PIXELS_PLANAR
LUMAS = [(2, 2), (2, 1), (1, 1)]


def _device():
    return torch.device("cuda", jl.default_context().device)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_device())


def _planes(a):
    """(H, W, C) -> (C, H, W), (H, W) -> (1, H, W)"""
    return np.ascontiguousarray(a.transpose(2, 0, 1)) if a.ndim == 3 else a[None]


def _as(a, layout):
    return _dev(_planes(a) if layout == "chw" else a)


@functools.lru_cache(maxsize=None)
def _case(w, h, luma, opt=False, q=77, ri=0):
    """(rgb, ycc, oracle stream, oracle coefficients) of one image, computed once"""
    rgb = _enc_image(w, h, 3 * w + h)
    ycc = po.rgb_to_ycbcr8(rgb)
    ref, coefs = po.encode_8bit(ycc, luma[0], luma[1], q, want_coefficients=True, optimize_coding=opt, restart_interval=ri)
    return rgb, ycc, ref, coefs


def _encoded(tensors, luma, q, rgb, opt, layout, ri=0):
    b = jl.EncodeBatch().upload_tensors(tensors, luma, q, rgb, opt, ri, layout).encode()
    out = [(b.output(i), b.coefficients(i)) for i in range(len(b))]
    b.close()
    return out


# ------------------------------------------------------------------------------------------------ the fused instances

@pytest.mark.parametrize("w,h", FUSED_SHAPES)
@pytest.mark.parametrize("opt", [False, True])
@pytest.mark.parametrize("luma", LUMAS)
def test_fused_shapes_from_chw_and_hwc_tensors(w, h, opt, luma):
    """fdct_fused_kernel<H, V, 3> over the caller's memory and its planar instances: rows that start on 16 bytes (16, 48, 272, 1600), on 4 (100,
    20, 12), an image narrower than an MCU, one row high, more than 16 MCUs per line; YCbCr and RGB pixels, standard and built tables."""
    rgb, ycc, ref, ref_coefs = _case(w, h, luma, opt)
    for layout in ("chw", "hwc"):
        for px, is_rgb in ((ycc, False), (rgb, True)):
            (got, coefs), = _encoded([_as(px, layout)], luma, 77, is_rgb, opt, layout)
            assert np.array_equal(coefs, ref_coefs), (layout, is_rgb)
            assert got == ref, (layout, is_rgb)
    # Rgba32 pixels have an interleaved form only
    (got, coefs), = _encoded([_dev(_rgba(rgb, w))], luma, 77, True, opt, "hwc")
    assert np.array_equal(coefs, ref_coefs) and got == ref


def test_rgba_planes_are_refused():
    rgb = _case(20, 16, (2, 2))[0]
    rgba = _dev(_planes(_rgba(rgb, 1)))
    with pytest.raises(ValueError, match="samples per pixel"):
        jl.EncodeBatch().upload_tensors([rgba], (2, 2), 77, rgb=True, layout="chw")
    b = jl.EncodeBatch()
    ptrs = (C.c_void_p * 1)(rgba.data_ptr())
    params = (_capi.EncodeParams * 1)(_capi.EncodeParams(20, 16, 3, 2, 2, 77, 2, 0, 0))
    assert _lib.jpgpu_encoder_upload_device(b._h, ptrs, params, (C.c_int32 * 1)(PLANAR), 1) == ERR_ARGUMENT
    assert b"Rgba32" in _lib.jpgpu_last_error(b.ctx._h)
    assert _lib.jpgpu_encoder_upload_device(b._h, ptrs, params, (C.c_int32 * 1)(INTERLEAVED), 1) == 0  # (the same bytes as pixels of four)
    b.close()


# ------------------------------------------------------------------------------------------------ addresses the caller chose

def _at_offset(a, offset):
    """the array's bytes `offset` bytes into a larger device buffer (torch allocations start on 512 bytes)"""
    flat = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.zeros(flat.numel() + 64, dtype=torch.uint8, device=_device())
    assert buf.data_ptr() % 256 == 0
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    view = view.view(a.shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + offset
    return view


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("luma", LUMAS)
@pytest.mark.parametrize("w,h", [(16, 16), (272, 33), (100, 80)])
def test_misaligned_bases_give_the_aligned_bytes(w, h, luma, layout):
    """The image 1, 4 and 8 bytes into a buffer: no wide load on an address that is not a multiple of its size -- the slower variants,
    the same bytes.  (Widths 16 and 272 take the look-ahead fetch when aligned, 100 the dword rows.)"""
    rgb, _, ref, ref_coefs = _case(w, h, luma)
    a = _planes(rgb) if layout == "chw" else rgb
    tensors = [_dev(a)] + [_at_offset(a, off) for off in (1, 4, 8)]
    assert [t.data_ptr() % 16 for t in tensors] == [0, 1, 4, 8]
    for k, (got, coefs) in enumerate(_encoded(tensors, luma, 77, True, False, layout)):
        assert np.array_equal(coefs, ref_coefs), k
        assert got == ref, k


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("luma", LUMAS)
def test_an_image_of_a_batch_tensor_whose_size_is_no_multiple_of_16(luma, layout):
    """(2, 3, 81, 100): image 1 starts 24 300 bytes in (a multiple of 4, not of 8), and a plane is 8 100 bytes"""
    w, h = 100, 81
    rgbs = [_case(w, h, luma)[0], _case(w, h, luma)[0][::-1, ::-1].copy()]
    batch = _dev(np.stack([_planes(r) if layout == "chw" else r for r in rgbs]))
    assert batch[1].data_ptr() % 16 == 12 and batch[1].is_contiguous()
    out = _encoded([batch[0], batch[1]], luma, 77, True, False, layout)
    for k, rgb in enumerate(rgbs):
        ref, ref_coefs = po.encode_8bit(po.rgb_to_ycbcr8(rgb), luma[0], luma[1], 77, want_coefficients=True)
        assert np.array_equal(out[k][1], ref_coefs) and out[k][0] == ref, k


# ------------------------------------------------------------------------------------------------ the two-kernel path

@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_two_kernel_shapes(layout):
    """E1a + E1b: gray as (1, H, W) / (H, W), and colour at luma 4 x 1 and 1 x 2, through the per-sample readers"""
    for (w, h) in ((31, 65), (75, 50)):
        gray = np.ascontiguousarray(_case(w, h, (1, 1))[1][..., 0])
        for luma in ((1, 1), (2, 2)):
            ref, ref_coefs = po.encode_8bit(gray, luma[0], luma[1], 60, want_coefficients=True)
            (got, coefs), = _encoded([_as(gray, layout)], luma, 60, False, False, layout)
            assert np.array_equal(coefs, ref_coefs) and got == ref, (w, h, luma)
        for luma in ((4, 1), (1, 2)):
            rgb, ycc, ref, ref_coefs = _case(w, h, luma, False, 70)
            for px, is_rgb in ((ycc, False), (rgb, True)):
                (got, coefs), = _encoded([_as(px, layout)], luma, 70, is_rgb, False, layout)
                assert np.array_equal(coefs, ref_coefs) and got == ref, (w, h, luma, is_rgb)
    if layout == "hwc":  # the four-byte reader of the two-kernel path over the caller's memory
        rgb, _, ref, _ = _case(75, 50, (4, 1), False, 70)
        assert _encoded([_dev(_rgba(rgb, 3))], (4, 1), 70, True, False, "hwc")[0][0] == ref


# ------------------------------------------------------------------------------------------------ described arrangements

DESCRIBED = [("A", (37, 29), False), ("A", (37, 29), True), ("E", (24, 24), False), ("E", (264, 136), True)]


@pytest.mark.parametrize("name,size,built", DESCRIBED, ids=["%s-%dx%d-%s" % (n, s[0], s[1], "built" if b else "given") for n, s, b in DESCRIBED])
def test_described_arrangements_equal_the_host_upload(name, size, built):
    """A: four components (CMYK-like) as [4, H, W]; E: a sub-sampled FIRST component.  Both layouts against upload_described."""
    px = ea.pixels(size[0], size[1], len(ea.SAMPLING[name]), 21)
    desc = ea.to_description(ea.arrangement(name, built), size[0], size[1])
    host = jl.EncodeBatch().upload_described([px], [desc]).encode()
    want, want_coefs = host.output(0), host.coefficients(0)
    host.close()
    for layout in ("chw", "hwc"):
        b = jl.EncodeBatch().upload_described_tensors([_as(px, layout)], [desc], layout).encode()
        assert np.array_equal(b.coefficients(0), want_coefs), layout
        assert b.output(0) == want, layout
        b.close()


def test_a_refused_arrangement_is_that_image_alone():
    f, a = ea.pixels(40, 24, 2, 13), ea.pixels(37, 29, 4, 11)
    descs = [ea.to_description(ea.arrangement("A"), 37, 29), ea.to_description(ea.arrangement("F"), 40, 24), ea.to_description(ea.arrangement("A"), 37, 29)]
    host = jl.EncodeBatch().upload_described([a, f, a], descs).encode()
    b = jl.EncodeBatch().upload_described_tensors([_as(p, "chw") for p in (a, f, a)], descs)
    assert [b.image_status(i) for i in range(3)] == [0, 3, 0]
    b.encode()
    assert b.output(0) == host.output(0) and b.output(2) == host.output(2)
    with pytest.raises(jl.NotSupportedException, match="maximum sampling factors"):
        b.output(1)
    with pytest.raises(jl.NotSupportedException):
        b.output_tensor(1)
    b.close()
    host.close()


# ------------------------------------------------------------------------------------------------ one upload, both layouts

def _raw_batch(entries, device):
    """entries: (array (H, W, C) or (H, W), luma, quality, rgb mode, optimize_coding, restart_interval, pixel layout).  device=True: one
    jpgpu_encoder_upload_device with per-image layouts; False: jpgpu_encoder_upload of the interleaved arrays."""
    n = len(entries)
    params, keep, blocks = (_capi.EncodeParams * n)(), [], []
    ptrs, layouts = (C.c_void_p * n)(), (C.c_int32 * n)()
    for i, (a, luma, q, mode, opt, ri, layout) in enumerate(entries):
        h, w = a.shape[:2]
        comps = 1 if a.ndim == 2 else 3
        params[i] = _capi.EncodeParams(w, h, comps, luma[0], luma[1], q, mode, opt, ri)
        blocks.append((-(-w // (8 * luma[0]))) * (-(-h // (8 * luma[1]))) * (luma[0] * luma[1] + (2 if comps == 3 else 0)))
        if device:
            t = _dev(_planes(a) if layout == PLANAR else a)
            ptrs[i], layouts[i] = t.data_ptr(), layout
        else:
            t = np.ascontiguousarray(a)
            ptrs[i] = t.ctypes.data
        keep.append(t)
    b = jl.EncodeBatch()
    if device:
        torch.cuda.synchronize()
        b._check(_lib.jpgpu_encoder_upload_device(b._h, ptrs, params, layouts, n))
    else:
        b._check(_lib.jpgpu_encoder_upload(b._h, ptrs, params, n))
    b._n, b._blocks, b._keep = n, blocks, keep
    return b


@pytest.mark.parametrize("ri", [0, 3], ids=["one_pass", "restart_3"])
def test_planar_and_interleaved_images_in_one_upload(ri):
    """Fused and two-kernel shapes, both layouts, Rgba32, gray, built tables (and restart intervals) in ONE upload: every instance of E1
    leaves the others' images alone, and the entropy stage runs as it does behind the host upload of the same images."""
    shapes = [(160, 96, (2, 2)), (33, 47, (2, 2)), (64, 64, (1, 1)), (75, 50, (4, 1)), (50, 70, (1, 2)), (100, 80, (2, 1)), (272, 33, (1, 1)), (48, 40, (2, 2))]
    entries, want = [], []
    for k, (w, h, luma) in enumerate(shapes):
        opt = 1 if k in (1, 4, 6) else 0
        rgb, ycc, ref, _ = _case(w, h, luma, bool(opt), 70, ri)
        layout = PLANAR if k % 2 == 0 else INTERLEAVED
        if k == 2:  # gray, as one plane
            gray = np.ascontiguousarray(ycc[..., 0])
            entries.append((gray, luma, 70, 0, opt, ri, PLANAR))
            want.append(po.encode_8bit(gray, luma[0], luma[1], 70, optimize_coding=opt, restart_interval=ri))
            continue
        if k == 5:  # Rgba32: interleaved only
            entries.append((_rgba(rgb, k), luma, 70, 2, opt, ri, INTERLEAVED))
        elif k == 7:  # samples that are Y, Cb, Cr already
            entries.append((ycc, luma, 70, 0, opt, ri, layout))
        else:
            entries.append((rgb, luma, 70, 1, opt, ri, layout))
        want.append(ref)
    dev, host = _raw_batch(entries, True), _raw_batch(entries, False)
    for rep in range(2):
        dev.encode()
        host.encode()
        assert dev.emit_passes() == host.emit_passes() == ((rep + 1, 0) if ri == 0 else (0, 0))
        for k, ref in enumerate(want):
            assert dev.output(k) == ref, (rep, k)
    assert set(dev.stage_ms()) == set(host.stage_ms())
    # SetQuantizationTable behind a device upload, as behind a host upload
    table = np.arange(1, 65, dtype=np.uint16)
    for b in (dev, host):
        b.set_quantization_table(0, 0, table).encode()
    assert dev.output(0) == host.output(0) != want[0]
    assert np.array_equal(dev.coefficients(0), host.coefficients(0))
    dev.close()
    host.close()


# ------------------------------------------------------------------------------------------------ refusals

def _hip(name, *argtypes):
    for lib in (None, "libamdhip64.so.7", "libamdhip64.so"):
        try:
            fn = getattr(C.CDLL(lib), name)
            break
        except (OSError, AttributeError):
            continue
    fn.restype, fn.argtypes = C.c_int, list(argtypes)
    return fn


def test_refusals_beside_a_batch_that_encodes():
    rgb, _, ref, _ = _case(16, 16, (2, 2))
    good = jl.EncodeBatch().upload_tensors([_dev(rgb)], (2, 2), 77, rgb=True, layout="hwc")
    bad = jl.EncodeBatch()
    params = (_capi.EncodeParams * 1)(_capi.EncodeParams(16, 16, 3, 2, 2, 77, 1, 0, 0))
    nbytes = rgb.size

    def upload(ptr, layout=INTERLEAVED):
        rc = _lib.jpgpu_encoder_upload_device(bad._h, (C.c_void_p * 1)(ptr), params, (C.c_int32 * 1)(layout), 1)
        return rc, _lib.jpgpu_last_error(bad.ctx._h)

    # host memory
    host = np.ascontiguousarray(rgb)
    rc, msg = upload(host.ctypes.data)
    assert rc == ERR_ARGUMENT and b"device memory" in msg, (rc, msg)
    # a layout that does not exist
    t = _dev(rgb)
    rc, msg = upload(t.data_ptr(), 2)
    assert rc == ERR_ARGUMENT and b"pixel layout" in msg, (rc, msg)
    # null arguments
    assert _lib.jpgpu_encoder_upload_device(bad._h, (C.c_void_p * 1)(None), params, None, 1) == ERR_ARGUMENT
    assert _lib.jpgpu_encoder_upload_device(bad._h, None, params, None, 1) == ERR_ARGUMENT
    assert _lib.jpgpu_encoder_upload_device(bad._h, (C.c_void_p * 1)(t.data_ptr()), None, None, 1) == ERR_ARGUMENT
    assert _lib.jpgpu_encoder_upload_device(None, (C.c_void_p * 1)(t.data_ptr()), params, None, 1) == ERR_ARGUMENT
    # the last bytes of an allocation whose size is known: one byte further and the image leaves it
    size = 2 << 20
    base = C.c_void_p()
    assert _hip("hipMalloc", C.POINTER(C.c_void_p), C.c_size_t)(C.byref(base), size) == 0
    try:
        last = base.value + size - nbytes
        assert _hip("hipMemcpy", C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)(last, host.ctypes.data, nbytes, 1) == 0  # hipMemcpyHostToDevice
        for layout in (INTERLEAVED, PLANAR):
            rc, msg = upload(last + 1, layout)
            assert rc == ERR_ARGUMENT and b"inside one device allocation" in msg, (rc, msg)
        # a refused upload leaves nothing to encode
        assert len(bad) == 0 and bad.image_status(0) == ERR_ARGUMENT
        # ... and the image that ends exactly where the allocation does is taken
        rc, msg = upload(last)
        assert rc == 0, (rc, msg)
        bad._n = 1
        assert bad.encode().output(0) == ref
    finally:
        bad.close()
        assert _hip("hipFree", C.c_void_p)(base) == 0
    assert good.encode().output(0) == ref
    good.close()


def test_upload_tensors_refuses_what_it_would_have_to_copy():
    rgb = _case(20, 16, (2, 2))[0]
    b = jl.EncodeBatch()
    t = _dev(rgb)
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        b.upload_tensors([t.permute(2, 0, 1)], layout="chw")
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        b.upload_tensors([_dev(_planes(rgb))[:, :, ::2]], layout="chw")
    with pytest.raises(ValueError, match="uint8"):
        b.upload_tensors([t.to(torch.int16)], layout="hwc")
    with pytest.raises(ValueError, match="context's device"):
        b.upload_tensors([t.cpu()], layout="hwc")
    with pytest.raises(ValueError, match="samples per pixel"):
        b.upload_tensors([t], layout="chw")  # (16, 20, 3) read as 16 planes
    with pytest.raises(ValueError, match="samples per pixel"):
        b.upload_tensors([_dev(_rgba(rgb, 1))], rgb=False, layout="hwc")
    b.close()


# ------------------------------------------------------------------------------------------------ decode -> encode on the device

def test_decode_to_tensors_straight_into_encode_tensors():
    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=60 + k)) for k, (w, h, sub, dri) in enumerate([(80, 48, "420", 4), (61, 37, "444", 0), (40, 24, "gray", 0)])]
    tensors, results = jl.decode_to_tensors(files)
    assert all(r.status == 0 for r in results) and all(tuple(t.shape)[0] == 3 for t in tensors)
    pixels, _ = jl.decode_batch(files, jl.FMT_RGB_U8)
    for luma in ((2, 2), (1, 1)):
        assert jl.encode_tensors(tensors, luma, 80) == jl.encode_batch(pixels, luma, 80, rgb=True), luma
    hwc, _ = jl.decode_to_tensors(files, jl.FMT_RGB_U8)
    assert jl.encode_tensors(hwc, (2, 1), 80, layout="hwc") == jl.encode_batch(pixels, (2, 1), 80, rgb=True)


def test_output_tensor_aliases_the_encoded_stream():
    rgbs = [_case(w, h, (2, 2))[0] for (w, h) in ((100, 80), (20, 16), (272, 33))]
    b = jl.EncodeBatch().upload_tensors([_dev(_planes(r)) for r in rgbs], (2, 2), 77, rgb=True).encode()
    tensors, hosts = [], []
    for i, rgb in enumerate(rgbs):
        t = b.output_tensor(i)
        size = C.c_size_t()
        ptr = _lib.jpgpu_encoder_output_device(b._h, i, C.byref(size))
        assert t.data_ptr() == ptr and tuple(t.shape) == (size.value,) and t.dtype == torch.uint8
        assert t.device.type == "cuda" and t.device.index == b.ctx.device
        host = b.output(i)
        assert host == _case(rgb.shape[1], rgb.shape[0], (2, 2))[2]
        assert bytes(t.cpu().numpy()) == host
        assert int(t[:2].to(torch.int32).sum().item()) == 0xFF + 0xD8  # torch computes on it, on the device: SOI
        tensors.append(t)
        hosts.append(host)
    del b, t
    gc.collect()
    for t, host in zip(tensors, hosts):  # the holder keeps the batch, and so the memory, alive
        assert bytes(t.cpu().numpy()) == host
    fresh = jl.EncodeBatch().upload_tensors([_dev(_planes(rgbs[0]))], (2, 2), 77, rgb=True)
    with pytest.raises((ValueError, jl.JpegError)):
        fresh.output_tensor(0)  # (no encode() yet)
    fresh.close()
