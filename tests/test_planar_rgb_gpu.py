"""RGB_PLANAR_U8: RGB_U8's bytes as three tight planes uint8[3, H, W], written by K3 itself (a fused store path for the four fast
layout classes, the scratch image + converter for everything else), and Batch.output_tensor / decode_to_tensors, which hand the batch's
output buffer to torch without a copy.

Expected values: the oracle's block transform through test_idct_stage_gpu's writer model and po.ycbcr8_to_rgb (the reference's
converter), transposed; whole files also against the RGB_U8 sink of the same process.  Every byte of every image is compared, and
Batch.plan_stats()["idct_work"] proves which layout class each frame reached."""
import ctypes as C
import gc
import io

import numpy as np
import pytest

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from jpeglibrary_amd import decoder as jd
from oracle import pyoracle as po
from test_idct_stage_gpu import (BIG, DETAIL_UNSUPPORTED_FRAME, GENERIC, GEOMETRIES, GRAY, H1V1, H2V1, H2V2, NOT_SUPPORTED, S420, S422, S444, TILE_ROWS,
                                 _assert_same, _cases, _expected, _expected_class, _file_case, _frame, _planes, _run_frames)
from test_split_handoff_gpu import SMALL
from tools import jpegsynth

pytestmark = pytest.mark.gpu
FMT = jl.FMT_RGB_PLANAR_U8


def _rgb_only(cases):
    return [c for c in cases if len(c[0]["components"]) in (1, 3)]


def _want(frame, qt, blocks):
    """RGB_U8's expectation (the converter over the interleaved samples), as planes"""
    return np.ascontiguousarray(_expected(jl.FMT_RGB_U8, frame, _planes(frame, qt, blocks)).transpose(2, 0, 1))


@pytest.fixture(scope="module")
def matrix():
    """(cases, expected planes) of the whole geometry matrix, computed once"""
    cases = _rgb_only(_cases(2, GEOMETRIES + TILE_ROWS + BIG))
    return cases, [_want(*c) for c in cases]


# ------------------------------------------------------------------------------------------------ 1, 2: the frame hand-off

def test_every_layout_class_alone():
    for i, (frame, qt, blocks) in enumerate(_rgb_only(_cases(1, GEOMETRIES))):
        sampling = [(c[1], c[2]) for c in frame["components"]]
        b = _run_frames([frame], [qt], [blocks], FMT)
        work = b.plan_stats()["idct_work"]
        cls = _expected_class(frame["width"], frame["height"], sampling)
        assert work[cls] > 0 and sum(work) == work[cls], (i, frame["width"], frame["height"], sampling, work)
        _assert_same(b.output(0), _want(frame, qt, blocks), i)


def test_all_classes_in_one_batch_in_two_orders(matrix):
    cases, want = matrix
    for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
        b = _run_frames([cases[i][0] for i in order], [cases[i][1] for i in order], [cases[i][2] for i in order], FMT)
        for k, i in enumerate(order):
            _assert_same(b.output(k), want[i], i)
            info, (w, h) = b.image_info(k), (cases[i][0]["width"], cases[i][0]["height"])
            assert info.out_bytes == 3 * w * h
            for c in range(3):
                p = info.plane[c]
                assert (p.offset, p.width, p.height, p.pitch) == (c * w * h, w, h, w), (i, c)
        work = b.plan_stats()["idct_work"]
        assert all(work[c] > 0 for c in (GENERIC, H1V1, H2V1, H2V2, GRAY)) and work[5] == 0, work


# ------------------------------------------------------------------------------------------------ 3: against the existing sink

def _progressive_file():
    from PIL import Image

    yy, xx = np.mgrid[0:56, 0:88]
    rgb = np.stack([(xx * 3) % 256, (yy * 5) % 256, (xx + yy) % 256], axis=-1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=85, progressive=True)
    assert b"\xff\xc2" in buf.getvalue()
    return buf.getvalue()


def _same_as_rgb_u8(files):
    a = jl.Batch().upload(files, jl.FMT_RGB_U8).decode().sync()
    b = jl.Batch().upload(files, FMT).decode().sync()
    for i in range(len(files)):
        assert (a.result(i).status, b.result(i).status) == (0, 0), i
        _assert_same(b.output(i), np.ascontiguousarray(a.output(i).transpose(2, 0, 1)), i)
    return b


@pytest.mark.parametrize("dri", [0, 3])
def test_whole_files_equal_the_rgb_u8_sink(dri):
    # widths that are and are not multiples of 16 (and of 8), heights that are and are not whole MCUs
    shapes = [(64, 48), (80, 33), (72, 40), (61, 37)]
    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=10 * k + j)) for k, (w, h) in enumerate(shapes) for j, sub in enumerate(("420", "422", "444", "gray"))]
    if dri == 0:
        files.append(_progressive_file())
    b = _same_as_rgb_u8(files)
    work = b.plan_stats()["idct_work"]
    assert all(work[c] > 0 for c in (GENERIC, H1V1, H2V1, H2V2, GRAY)), work


@pytest.mark.parametrize("dense", ["0", "1"], ids=["split", "dense"])
def test_the_split_handoff_shapes_equal_the_rgb_u8_sink(dense, monkeypatch):
    """JPGPU_DENSE_HANDOFF=0: every scan K3 has a split form for is handed over as half-line planes -- all four fast classes of this sink"""
    monkeypatch.setenv("JPGPU_DENSE_HANDOFF", dense)
    files = [bytes(jpegsynth.encode(w, h, sub, q, dri, seed=s)) for (w, h, sub, dri) in SMALL for q, s in ((75, 11), (97, 12))]
    b = _same_as_rgb_u8(files)
    total = C.c_uint64()
    assert _capi.lib.jpgpu_batch_coefficients_device(b._h, C.byref(total))
    blocks = sum(b.image_info(i).total_blocks for i in range(len(files)))
    assert (total.value > blocks) == (dense == "0"), (total.value, blocks)  # (the split scans' padding: the layout really differs)


# ------------------------------------------------------------------------------------------------ 4: every chroma pair

@pytest.mark.parametrize("sub,cls", [(0, H1V1), (1, H2V1), (2, H2V2)], ids=["444", "422", "420"])
def test_every_chroma_pair_on_every_fused_class(sub, cls):
    """test_independent_evidence's frame: Cb x Cr sweep all 65 536 pairs at a few luma levels (quality 100).  Under 4:2:2 / 4:2:0 the
    chroma planes are the same 256 x 256 and every chroma sample covers 2 x 1 / 2 x 2 equal pixels."""
    from PIL import Image

    fx, fy = (1, 1) if sub == 0 else ((2, 1) if sub == 1 else (2, 2))
    cbg, crg = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    cbg, crg = (np.repeat(np.repeat(g, fy, axis=0), fx, axis=1) for g in (cbg, crg))
    files = []
    for y in (0, 37, 128, 201, 255):
        ycc = np.stack([np.full(cbg.shape, y), cbg, crg], axis=-1).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(ycc, mode="YCbCr").save(buf, format="JPEG", quality=100, subsampling=sub)
        files.append(buf.getvalue())
    ycc_out, res = jl.decode_batch(files, jl.FMT_INTERLEAVED_U8)
    b = jl.Batch().upload(files, FMT).decode().sync()
    work = b.plan_stats()["idct_work"]
    assert work[cls] > 0 and sum(work) == work[cls], work
    pairs = set()
    for i, a in enumerate(ycc_out):
        assert res[i].status == 0 and b.result(i).status == 0
        _assert_same(b.output(i), np.ascontiguousarray(po.ycbcr8_to_rgb(a).transpose(2, 0, 1)), i)
        pairs.update(np.unique(a[..., 1].astype(np.int64) * 256 + a[..., 2]).tolist())
    print("distinct (Cb, Cr) pairs decoded:", len(pairs))
    assert len(pairs) > 60000  # (the decoded samples still cover the range: 65 536 went in)


# ------------------------------------------------------------------------------------------------ 5: refusals and edges

def test_refusals_beside_images_that_decode():
    rng = np.random.default_rng(5)
    good = [_frame(rng, 64, 32, S420), _frame(rng, 40, 24, [(1, 1)])]
    bad = [_frame(rng, 40, 24, [(1, 1), (1, 1)]), _frame(rng, 33, 17, [(2, 2), (1, 1), (1, 1), (2, 2)]), _frame(rng, 32, 16, S444, precision=12)]
    cases = [good[0], bad[0], bad[1], good[1], bad[2]]
    b = jl.Batch().upload_frames([c[0] for c in cases], np.stack([c[1] for c in cases]), FMT)
    for i in (1, 2, 4):  # straight after the upload
        assert (b.image_info(i).status, b.image_info(i).detail) == (NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME), i
    for i in (0, 3):
        assert b.image_info(i).status == 0
        b.set_coefficients(i, cases[i][2])
    b.run_idct().sync()
    for i in (1, 2, 4):
        assert (b.result(i).status, b.result(i).detail) == (NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME), i
        with pytest.raises(jl.NotSupportedException):
            b.output(i)
    for i in (0, 3):
        assert b.result(i).status == 0
        _assert_same(b.output(i), _want(*cases[i]), i)
    # the same messages as RGB_U8
    msgs = {}
    for fmt in (jl.FMT_RGB_U8, FMT):
        for k, c in enumerate((bad[0], bad[2])):
            bb = jl.Batch().upload_frames([c[0]], np.stack([c[1]]), fmt)
            with pytest.raises(jl.NotSupportedException) as ei:
                bb.output(0)
            msgs[(fmt, k)] = str(ei.value)
    assert msgs[(FMT, 0)] == msgs[(jl.FMT_RGB_U8, 0)] and msgs[(FMT, 1)] == msgs[(jl.FMT_RGB_U8, 1)], msgs


def test_a_frame_without_any_scan_is_the_converter_over_zeros():
    good = bytes(jpegsynth.encode(64, 48, "420", 75, 2, seed=3))
    gray = bytes(jpegsynth.encode(40, 24, "gray", 75, 0, seed=4))
    files = [f[:f.index(b"\xff\xda")] + b"\xff\xd9" for f in (good, gray)] + [good]
    b = jl.Batch().upload(files, FMT).decode().sync()
    for i, (w, h, nc) in enumerate([(64, 48, 3), (40, 24, 1)]):
        assert b.result(i).status == 0
        want = po.ycbcr8_to_rgb(np.zeros((h, w, nc), np.uint8), gray=nc == 1).transpose(2, 0, 1)
        assert len(np.unique(want[0])) == 1  # (one value per plane)
        _assert_same(b.output(i), np.ascontiguousarray(want), i)
    _assert_same(b.output(2), np.ascontiguousarray(po.ycbcr8_to_rgb(po.decode_8bit(good)[0]).transpose(2, 0, 1)), "neighbour")


def test_one_pixel_and_one_block_images():
    cases = _cases(7, [(1, 1, [(1, 1)]), (8, 8, [(1, 1)]), (1, 1, S444), (8, 8, S444), (1, 1, S420), (8, 8, S420), (16, 16, S420), (16, 8, S422)])
    b = _run_frames([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], FMT)
    for i, c in enumerate(cases):
        _assert_same(b.output(i), _want(*c), i)


# ------------------------------------------------------------------------------------------------ 6: per-scan entries

def test_one_decode_scan_call_on_a_420_scan():
    from test_per_scan_gpu import Walk

    frame, qt, blocks, data = _file_case(2200, 48, 32, S420, 8, 3)
    w, st = Walk(data), {}

    def on_scan(entropy, sh):
        st.update(entropy=bytes(entropy), sh=sh, dri=w.dri, quant=w.quantization_tables(), huff=w.huffman_tables())
        return 0

    w.run(lambda marker, fh: st.update(fh=fh, sof=marker), on_scan)
    f, sc = st["fh"]._c(st["sof"]), st["sh"]._c()
    qtc, present, dht = jd._tables_c(st["quant"], st["huff"], sc, jd._frame_tq_slots(f))
    ctx = jl.default_context()
    ebuf = np.frombuffer(st["entropy"], np.uint8)
    outs = {}
    for fmt in (jl.FMT_RGB_U8, FMT):
        out = np.zeros(48 * 32 * 3, np.uint8)
        res, consumed = _capi.ImageResult(), C.c_size_t()
        rc = _capi.lib.jpgpu_decode_scan(ctx._h, C.byref(f), C.byref(sc), qtc.ctypes.data, present.ctypes.data, C.cast(dht, C.c_void_p), st["dri"],
                                         ebuf.ctypes.data, ebuf.size, fmt, out.ctypes.data, out.size, C.byref(res), C.byref(consumed))
        assert rc == 0 and res.status == 0, ctx.last_error()
        assert consumed.value == len(st["entropy"]) - 2
        outs[fmt] = out
    want = np.ascontiguousarray(outs[jl.FMT_RGB_U8].reshape(32, 48, 3).transpose(2, 0, 1))
    _assert_same(outs[FMT].reshape(3, 32, 48), want, "decode_scan")
    _assert_same(want, _want(frame, qt, blocks), "model")


def test_one_progressive_session():
    from golden_util import read_jpeg
    from test_per_scan_gpu import _decode_progressive_scan_by_scan

    data = read_jpeg("progress.jpg")
    sizes = {}

    def deliver(fmt):
        def f(dec, fh):
            sizes[fmt] = dec.output_size(fmt)
            return dec.Dispose(fmt=fmt)
        return f

    rgb, state = _decode_progressive_scan_by_scan(data, deliver(jl.FMT_RGB_U8))
    planar, _ = _decode_progressive_scan_by_scan(data, deliver(FMT))
    w, h = state["fh"].SamplesPerLine, state["fh"].NumberOfLines
    assert sizes[FMT] == 3 * w * h == sizes[jl.FMT_RGB_U8]
    want = np.ascontiguousarray(rgb.reshape(h, w, 3).transpose(2, 0, 1))
    _assert_same(planar.reshape(3, h, w), want, "dispose")
    _assert_same(want, np.ascontiguousarray(po.ycbcr8_to_rgb(po.decode_8bit(data)[0]).transpose(2, 0, 1)), "oracle")


# ------------------------------------------------------------------------------------------------ 7: torch hand-over

TENSOR_FILES = [(80, 48, "420", 4), (61, 37, "444", 0), (40, 24, "gray", 0)]


@pytest.mark.parametrize("fmt", [FMT, jl.FMT_RGB_U8], ids=["rgb_planar", "rgb"])
def test_output_tensor_aliases_the_output_buffer(fmt):
    import torch

    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=20 + k)) for k, (w, h, sub, dri) in enumerate(TENSOR_FILES)]
    b = jl.Batch().upload(files, fmt).decode()  # (no sync: output_tensor does it)
    base = None
    tensors, hosts = [], []
    for i, (w, h, _, _) in enumerate(TENSOR_FILES):
        t = b.output_tensor(i)
        base = b.output_device_ptr()[0]
        assert tuple(t.shape) == ((3, h, w) if fmt == FMT else (h, w, 3)) and t.dtype == torch.uint8
        assert t.device.type == "cuda" and t.device.index == b.ctx.device
        assert t.data_ptr() == base + b.image_info(i).out_offset
        host = b.output(i)
        assert torch.equal(t.cpu(), torch.from_numpy(host))
        m = t.float().mean()  # torch computes on it, on the device
        assert m.device == t.device and abs(m.item() - host.astype(np.float64).mean()) < 1e-2
        tensors.append(t)
        hosts.append(host)
    del b, t
    gc.collect()
    for t, host in zip(tensors, hosts):  # the holder keeps the batch, and so the memory, alive
        assert torch.equal(t.cpu(), torch.from_numpy(host))


def test_output_tensor_refuses_padded_planes_and_failed_images():
    files = [bytes(jpegsynth.encode(48, 32, "420", 75, 0, seed=30))]
    for fmt in (jl.FMT_PLANAR_U8, jl.FMT_PLANAR_I16, jl.FMT_EXTENDED_U16):
        b = jl.Batch().upload(files, fmt).decode().sync()
        with pytest.raises(ValueError):
            b.output_tensor(0)
    b = jl.Batch().upload([files[0][:20]], FMT).decode().sync()
    with pytest.raises(jl.JpegError):
        b.output_tensor(0)


def test_decode_to_tensors():
    import torch

    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=40 + k)) for k, (w, h, sub, dri) in enumerate(TENSOR_FILES)]
    files[1] = files[1][:20]  # cut inside its headers
    tensors, results = jl.decode_to_tensors(files)
    outs, want_results = jl.decode_batch(files, FMT)
    assert [t is None for t in tensors] == [False, True, False] == [o is None for o in outs]
    for i, (t, r, wr) in enumerate(zip(tensors, results, want_results)):
        assert (r.status, r.detail) == (wr.status, wr.detail), i
        if t is not None:
            w, h = TENSOR_FILES[i][:2]
            assert tuple(t.shape) == (3, h, w) and t.dtype == torch.uint8 and t.is_cuda
            assert torch.equal(t.cpu(), torch.from_numpy(outs[i]))
    assert results[1].status != 0
    gc.collect()
    assert torch.equal(tensors[2].cpu(), torch.from_numpy(outs[2]))
    hwc, _ = jl.decode_to_tensors(files[:1], jl.FMT_RGB_U8)
    assert torch.equal(hwc[0].permute(2, 0, 1), tensors[0])
