"""RGB_PLANAR_F16 / RGB_PLANAR_F32: RGB_PLANAR_U8's planes with every byte u of channel c written by K3 as the float
(float32)u * scale[c] + bias[c] -- a fused store for the four fast layout classes (dense and split form), the scratch image and a float
converter for everything else -- and the constants (Batch.set_output_affine), which are launch state.

A float sample is a fixed IEEE function of the byte RGB_PLANAR_U8 holds at its place, so every comparison here is on the bit pattern
(.view(np.uint16) / .view(np.uint32)) of every sample of every image.  The expected value is always float_sink_model.model -- numpy's
(u.astype(float32) * float32(scale[c]) + float32(bias[c])).astype(dtype) -- over bytes that existing, pinned code produces: the RGB_U8
writer model of test_idct_stage_gpu, transposed, or the RGB_PLANAR_U8 sink of the same files in the same process."""
import gc
import io

import numpy as np
import pytest

import jpeglibrary_amd as jl
from float_sink_model import IMAGENET, NEGATIVE, TIES, DEFAULT, model
from test_idct_stage_gpu import (BIG, DETAIL_UNSUPPORTED_FRAME, GENERIC, GEOMETRIES, GRAY, H1V1, H2V1, H2V2, NOT_SUPPORTED, S420, S444, TILE_ROWS,
                                 _cases, _expected, _expected_class, _frame, _planes, _run_frames)
from test_split_handoff_gpu import SMALL
from tools import jpegsynth

pytestmark = pytest.mark.gpu

FORMATS = [(jl.FMT_RGB_PLANAR_F16, np.float16), (jl.FMT_RGB_PLANAR_F32, np.float32)]
FMT_IDS = ["f16", "f32"]
# the layout classes K3 has a split form for under these two formats (kernels.h: idct_split_supported): all four fast classes
SPLIT_CLASSES = {H1V1, H2V1, H2V2, GRAY}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _assert_bits(got, want, what):
    """every sample, bit for bit (so -0.0 != 0.0 and an infinity must be that infinity)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = _bits(got), _bits(want)
    assert np.array_equal(g, w), (what, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def _rgb_only(cases):
    return [c for c in cases if len(c[0]["components"]) in (1, 3)]


def _u8_planes(frame, qt, blocks):
    """RGB_U8's expectation (the converter over the interleaved samples), as planes: the bytes RGB_PLANAR_U8 holds"""
    return np.ascontiguousarray(_expected(jl.FMT_RGB_U8, frame, _planes(frame, qt, blocks)).transpose(2, 0, 1))


def _run(frames, qts, blocks, fmt, consts):
    b = jl.Batch().set_output_affine(*consts).upload_frames(frames, np.stack(qts), fmt)
    for i in range(len(frames)):
        assert b.image_info(i).status == 0, (i, b.image_info(i).status)
        b.set_coefficients(i, blocks[i])
    return b.run_idct().sync()


@pytest.fixture(scope="module")
def alone():
    """(cases, the bytes of their RGB planes), computed once for both sample types"""
    cases = _rgb_only(_cases(1, GEOMETRIES))
    return cases, [_u8_planes(*c) for c in cases]


@pytest.fixture(scope="module")
def matrix():
    cases = _rgb_only(_cases(2, GEOMETRIES + TILE_ROWS + BIG))
    return cases, [_u8_planes(*c) for c in cases]


# ------------------------------------------------------------------------------------------------ 1, 2: the frame hand-off

@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_every_layout_class_alone(fmt, dt, alone):
    cases, u8 = alone
    for i, (frame, qt, blocks) in enumerate(cases):
        sampling = [(c[1], c[2]) for c in frame["components"]]
        b = _run([frame], [qt], [blocks], fmt, IMAGENET)
        work = b.plan_stats()["idct_work"]
        cls = _expected_class(frame["width"], frame["height"], sampling)
        assert work[cls] > 0 and sum(work) == work[cls], (i, frame["width"], frame["height"], sampling, work)
        _assert_bits(b.output(0), model(u8[i], *IMAGENET, dt), i)


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_all_classes_in_one_batch_in_two_orders(fmt, dt, matrix):
    cases, u8 = matrix
    size = np.dtype(dt).itemsize
    for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
        b = _run([cases[i][0] for i in order], [cases[i][1] for i in order], [cases[i][2] for i in order], fmt, NEGATIVE)
        for k, i in enumerate(order):
            _assert_bits(b.output(k), model(u8[i], *NEGATIVE, dt), i)
            info, (w, h) = b.image_info(k), (cases[i][0]["width"], cases[i][0]["height"])
            assert info.out_bytes == 3 * w * h * size
            for c in range(3):
                p = info.plane[c]
                assert (p.offset, p.width, p.height, p.pitch) == (c * w * h * size, w, h, w), (i, c)
        work = b.plan_stats()["idct_work"]
        assert all(work[c] > 0 for c in (GENERIC, H1V1, H2V1, H2V2, GRAY)) and work[5] == 0, work


# ------------------------------------------------------------------------------------------------ 3: whole files

def _progressive_file():
    from PIL import Image

    yy, xx = np.mgrid[0:56, 0:88]
    rgb = np.stack([(xx * 3) % 256, (yy * 5) % 256, (xx + yy) % 256], axis=-1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=85, progressive=True)
    assert b"\xff\xc2" in buf.getvalue()
    return buf.getvalue()


def _same_as_the_u8_sink(files, fmt, dt, consts):
    a = jl.Batch().upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    b = jl.Batch().set_output_affine(*consts).upload(files, fmt).decode().sync()
    for i in range(len(files)):
        assert (a.result(i).status, b.result(i).status) == (0, 0), i
        _assert_bits(b.output(i), model(a.output(i), *consts, dt), i)
    return b


@pytest.mark.parametrize("dri", [0, 3])
@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_whole_files_equal_the_model_over_the_u8_sink(fmt, dt, dri):
    # widths that are and are not multiples of 16 (and of 8), heights that are and are not whole MCUs
    shapes = [(64, 48), (80, 33), (72, 40), (61, 37)]
    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=10 * k + j)) for k, (w, h) in enumerate(shapes) for j, sub in enumerate(("420", "422", "444", "gray"))]
    if dri == 0:
        files.append(_progressive_file())
    b = _same_as_the_u8_sink(files, fmt, dt, IMAGENET)
    work = b.plan_stats()["idct_work"]
    assert all(work[c] > 0 for c in (GENERIC, H1V1, H2V1, H2V2, GRAY)), work


# ------------------------------------------------------------------------------------------------ 4: the split hand-off

@pytest.mark.parametrize("dense", ["0", "1"], ids=["split", "dense"])
@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_the_split_handoff_shapes(fmt, dt, dense, monkeypatch):
    """JPGPU_DENSE_HANDOFF=0: every scan K3 has a split form for is handed over as half-line planes; =1: none is"""
    monkeypatch.setenv("JPGPU_DENSE_HANDOFF", dense)
    files = [bytes(jpegsynth.encode(w, h, sub, q, dri, seed=s)) for (w, h, sub, dri) in SMALL for q, s in ((75, 11), (97, 12))]
    b = _same_as_the_u8_sink(files, fmt, dt, NEGATIVE)
    stats = b.plan_stats()
    work, split = stats["idct_work"], stats["idct_split_work"]
    assert {c for c in range(6) if work[c] > 0} == {H1V1, H2V1, H2V2, GRAY}, work  # (SMALL's widths are whole MCUs)
    if dense == "1":
        assert sum(split) == 0, split
    else:  # every scan of SMALL has restart intervals and is its image's only scan: all of a supported class's work is split work
        assert {c for c in range(6) if split[c] > 0} == SPLIT_CLASSES and all(split[c] == work[c] for c in SPLIT_CLASSES), (work, split)


# ------------------------------------------------------------------------------------------------ 5: every byte value

def _flat_frames():
    """A gray frame of 256 flat blocks and a 4:4:4 frame of 512 flat MCUs, quantisation tables of ones: a DC of 8 * (v - 128) alone is the
    sample v in the whole block (the transform of a lone DC is exact).  Gray: v = 0..255.  4:4:4: Y = v with neutral chroma (R = G = B = v),
    then Y = v under chroma that moves with v."""
    qt = np.ones((4, 64), np.uint16)
    dc = lambda v: np.concatenate([[8 * (int(v) - 128)], np.zeros(63, np.int64)]).astype(np.int16)
    gray = ({"width": 128, "height": 128, "precision": 8, "components": [(1, 1, 1, 0)]}, qt, np.stack([dc(v) for v in range(256)]))
    mcus = [(v, 128, 128) for v in range(256)] + [(v, (37 * v) % 256, (91 * v + 5) % 256) for v in range(256)]
    ycc = ({"width": 256, "height": 128, "precision": 8, "components": [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 2)]}, qt,
           np.stack([dc(s) for m in mcus for s in m]))
    return [gray, ycc]


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_every_byte_value(fmt, dt):
    """DEFAULT: the sample is exactly float(u).  TIES (float_sink_model): as F16, channel 0 (scale 2^-25) is subnormal for every byte and an
    exact tie between two subnormals for every odd one; channel 1 (u + 1800) is an exact tie for u = 249, 251, 253, 255 (2049 .. 2055, where
    binary16 steps by 2); channel 2 (300 u - 100) overflows to +inf from u = 219 on and is negative for u = 0."""
    cases = _flat_frames()
    u8 = _run_frames([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], jl.FMT_RGB_PLANAR_U8)
    bytes_out = [u8.output(i) for i in range(2)]
    for i, planes in enumerate(bytes_out):  # a condition on the input, not on the code under test
        assert planes.shape[0] == 3 and all(len(np.unique(planes[c])) == 256 for c in range(3)), i
    assert [u8.plan_stats()["idct_work"][c] > 0 for c in (H1V1, GRAY)] == [True, True]
    for consts in (DEFAULT, TIES):
        b = _run([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], fmt, consts)
        for i in range(2):
            got = b.output(i)
            _assert_bits(got, model(bytes_out[i], *consts, dt), (i, consts is TIES))
            if consts is DEFAULT:
                assert np.array_equal(got.astype(np.float64), bytes_out[i].astype(np.float64)), i
    if dt == np.float16:  # (the set does what the docstring says, on the GPU's own output)
        assert np.isinf(got[2]).any() and (got[0][got[0] != 0] < 2.0 ** -14).all() and (got[2] < 0).any()


# ------------------------------------------------------------------------------------------------ 6: the constants are launch state

@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_the_constants_take_effect_at_the_next_launch_of_the_same_upload(fmt, dt):
    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=70 + k)) for k, (w, h, sub, dri) in enumerate([(80, 48, "420", 4), (61, 37, "444", 0), (40, 24, "gray", 2)])]
    u8 = jl.Batch().upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    want = [u8.output(i) for i in range(len(files))]
    b = jl.Batch().upload(files, fmt).decode().sync()
    for i, u in enumerate(want):
        _assert_bits(b.output(i), model(u, *DEFAULT, dt), ("default", i))
    b.set_output_affine(*IMAGENET).run_idct().sync()  # no upload in between
    for i, u in enumerate(want):
        _assert_bits(b.output(i), model(u, *IMAGENET, dt), ("run_idct", i))
    b.set_output_affine(*NEGATIVE).decode().sync()
    for i, u in enumerate(want):
        _assert_bits(b.output(i), model(u, *NEGATIVE, dt), ("decode", i))


def test_the_constants_do_not_touch_the_u8_sink():
    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=80 + k)) for k, (w, h, sub, dri) in enumerate([(64, 48, "420", 2), (61, 37, "422", 0), (40, 24, "gray", 0)])]
    a = jl.Batch().upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    b = jl.Batch().set_output_affine(*NEGATIVE).upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    for i in range(len(files)):
        assert b.output(i).dtype == np.uint8 and np.array_equal(a.output(i), b.output(i)), i


# ------------------------------------------------------------------------------------------------ 7: refusals

@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_constants_that_are_not_finite_are_refused_and_the_old_ones_stay(fmt, dt):
    files = [bytes(jpegsynth.encode(64, 48, "420", 75, 2, seed=90))]
    u = jl.Batch().upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync().output(0)
    b = jl.Batch().set_output_affine(*IMAGENET).upload(files, fmt)
    for scale, bias in (([1, np.nan, 1], [0, 0, 0]), ([1, 1, 1], [0, 0, np.inf]), ([-np.inf, 1, 1], [0, 0, 0]), ([1, 1, 1], [np.nan, 0, 0])):
        with pytest.raises(jl.ArgumentException):
            b.set_output_affine(scale, bias)
    _assert_bits(b.decode().sync().output(0), model(u, *IMAGENET, dt), "after the refusals")


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_frames_rgb_u8_refuses_fail_by_themselves(fmt, dt):
    rng = np.random.default_rng(5)
    good = [_frame(rng, 64, 32, S420), _frame(rng, 40, 24, [(1, 1)])]
    bad = [_frame(rng, 33, 17, [(2, 2), (1, 1), (1, 1), (2, 2)]), _frame(rng, 32, 16, S444, precision=12)]
    cases = [good[0], bad[0], good[1], bad[1]]
    b = jl.Batch().set_output_affine(*IMAGENET).upload_frames([c[0] for c in cases], np.stack([c[1] for c in cases]), fmt)
    for i in (1, 3):  # straight after the upload
        assert (b.image_info(i).status, b.image_info(i).detail) == (NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME), i
    for i in (0, 2):
        assert b.image_info(i).status == 0
        b.set_coefficients(i, cases[i][2])
    b.run_idct().sync()
    for i in (1, 3):
        assert (b.result(i).status, b.result(i).detail) == (NOT_SUPPORTED, DETAIL_UNSUPPORTED_FRAME), i
        with pytest.raises(jl.NotSupportedException):
            b.output(i)
    for i in (0, 2):
        assert b.result(i).status == 0
        _assert_bits(b.output(i), model(_u8_planes(*cases[i]), *IMAGENET, dt), i)
    for k, c in enumerate(bad):  # the class, the detail and the message RGB_U8 gives them
        seen = []
        for f in (jl.FMT_RGB_U8, fmt):
            bb = jl.Batch().upload_frames([c[0]], np.stack([c[1]]), f)
            with pytest.raises(jl.NotSupportedException) as ei:
                bb.output(0)
            seen.append((bb.image_info(0).status, bb.image_info(0).detail, str(ei.value)))
        assert seen[0] == seen[1], (k, seen)


# ------------------------------------------------------------------------------------------------ 8: the torch hand-over

TENSOR_FILES = [(80, 48, "420", 4), (61, 37, "444", 0), (40, 24, "gray", 0)]


def _torch_bits(t):
    import torch

    return t.cpu().view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy()


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_output_tensor_aliases_the_output_buffer(fmt, dt):
    import torch

    tdt = torch.float16 if dt == np.float16 else torch.float32
    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=20 + k)) for k, (w, h, sub, dri) in enumerate(TENSOR_FILES)]
    u8 = jl.Batch().upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    b = jl.Batch().set_output_affine(*IMAGENET).upload(files, fmt).decode()  # (no sync: output_tensor does it)
    tensors, wants = [], []
    for i, (w, h, _, _) in enumerate(TENSOR_FILES):
        t = b.output_tensor(i)
        assert tuple(t.shape) == (3, h, w) and t.dtype == tdt
        assert t.device.type == "cuda" and t.device.index == b.ctx.device
        assert t.data_ptr() == b.output_device_ptr()[0] + b.image_info(i).out_offset
        want = model(u8.output(i), *IMAGENET, dt)
        assert np.array_equal(_torch_bits(t), _bits(want).view(_torch_bits(t).dtype)), i
        assert (t * 2).device == t.device  # torch computes on it, on the device
        tensors.append(t)
        wants.append(want)
    del b, t
    gc.collect()
    for t, want in zip(tensors, wants):  # the holder keeps the batch, and so the memory, alive
        assert np.array_equal(_torch_bits(t), _bits(want).view(_torch_bits(t).dtype))


@pytest.mark.parametrize("fmt,dt", FORMATS, ids=FMT_IDS)
def test_decode_to_tensors_with_mean_and_std(fmt, dt):
    import torch

    tdt = torch.float16 if dt == np.float16 else torch.float32
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    files = [bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=40 + k)) for k, (w, h, sub, dri) in enumerate(TENSOR_FILES)]
    files.insert(2, files[0][:20])  # cut inside its headers
    u8, want_results = jl.decode_batch(files, jl.FMT_RGB_PLANAR_U8)
    tensors, results = jl.decode_to_tensors(files, dtype=tdt, mean=mean, std=std)
    assert [t is None for t in tensors] == [o is None for o in u8] and tensors[2] is None
    consts = jl.affine_from_mean_std(mean, std)
    for i, (t, r, wr) in enumerate(zip(tensors, results, want_results)):
        assert (r.status, r.detail) == (wr.status, wr.detail), i
        if t is not None:
            assert t.dtype == tdt and t.is_cuda and tuple(t.shape) == u8[i].shape
            want = model(u8[i], *consts, dt)
            assert np.array_equal(_torch_bits(t), _bits(want).view(_torch_bits(t).dtype)), i
    assert [r.status == 0 for r in results] == [True, True, False, True]
    plain, _ = jl.decode_to_tensors(files[:1], dtype=tdt)  # without mean / std: the byte as a float
    assert torch.equal(plain[0].cpu(), torch.from_numpy(u8[0]).to(tdt))
    with pytest.raises(ValueError):
        jl.decode_to_tensors(files[:1], dtype=tdt, mean=mean)
    with pytest.raises(ValueError):
        jl.decode_to_tensors(files[:1], mean=mean, std=std)


def test_encode_tensors_to_float_tensors_on_the_device():
    import torch

    rng = np.random.default_rng(11)
    imgs = [torch.from_numpy(rng.integers(0, 256, (3, 48, 64), dtype=np.uint8)).to("cuda:0"),
            torch.from_numpy(rng.integers(0, 256, (3, 17, 33), dtype=np.uint8)).to("cuda:0")]
    eb = jl.EncodeBatch().upload_tensors(imgs, (2, 2), 80, rgb=True, restart_interval=2).encode()
    streams = [eb.output_tensor(i) for i in range(len(eb))]  # the streams where they are, in device memory
    u8, _ = jl.decode_to_tensors(streams)
    for tdt, dt in ((torch.float16, np.float16), (torch.float32, np.float32)):
        tensors, results = jl.decode_to_tensors(streams, dtype=tdt, mean=[0.5, 0.4, 0.3], std=[0.2, 0.25, 0.3])
        consts = jl.affine_from_mean_std([0.5, 0.4, 0.3], [0.2, 0.25, 0.3])
        for i, (t, r) in enumerate(zip(tensors, results)):
            assert r.status == 0 and t.dtype == tdt and tuple(t.shape) == tuple(imgs[i].shape)
            want = model(u8[i].cpu().numpy(), *consts, dt)
            assert np.array_equal(_torch_bits(t), _bits(want).view(_torch_bits(t).dtype)), (tdt, i)
