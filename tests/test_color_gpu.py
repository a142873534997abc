"""The colour policy "file" on the GPU: CMYK, YCCK and Adobe-RGB files under the five RGB formats.

Every expected value is, bit for bit, the model (tests/color_model.py) applied to Batch.output(i) of the same file uploaded as
FMT_INTERLEAVED_U8 -- K3's sample bytes are pinned elsewhere.  Covered: the six kinds of file of the rule table at 1x1, 8x8, 17x33 and 45x67
under every RGB format, the float forms with the default and the ImageNet constants; a 2x2-subsampled YCCK file; a progressive CMYK file;
every (s0, s3) pair of the CMYK product from a 2048 x 2048 frame of DC-only blocks; one upload that mixes a fast-class YCbCr file, two CMYK
files, a grey file and a truncated one (the scratch slot of a CMYK image is larger than its output: the neighbour case); windows; the resize
stage; a device file whose Adobe marker lies behind 80 KB of APP1; Batch.color; the policy as state of the batch; and the default, which
decodes and refuses exactly as before."""
import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from float_sink_model import DEFAULT, IMAGENET
from tools import jpegsynth
import color_model as cm
import resize_model as rm

pytestmark = pytest.mark.gpu

VARIANTS = [("rgb_u8", jl.FMT_RGB_U8, None), ("rgba_u8", jl.FMT_RGBA_U8, None), ("planar_u8", jl.FMT_RGB_PLANAR_U8, None),
            ("planar_f16", jl.FMT_RGB_PLANAR_F16, DEFAULT), ("planar_f32", jl.FMT_RGB_PLANAR_F32, DEFAULT),
            ("planar_f16_imagenet", jl.FMT_RGB_PLANAR_F16, IMAGENET), ("planar_f32_imagenet", jl.FMT_RGB_PLANAR_F32, IMAGENET)]
V_IDS = [v[0] for v in VARIANTS]
SIZES = [(1, 1), (8, 8), (17, 33), (45, 67)]
NOT_SUPPORTED = 3

_SAMPLES = {}


def _samples(key, files):
    """the INTERLEAVED_U8 output of every file, decoded once per key and shared"""
    if key not in _SAMPLES:
        outs, results = jl.decode_batch(files, jl.FMT_INTERLEAVED_U8)
        assert all(r.status == 0 for r in results), [r.status for r in results]
        _SAMPLES[key] = outs
    return _SAMPLES[key]


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(-1), want.reshape(-1)
        bad = np.flatnonzero(g.view(np.dtype("u%d" % g.itemsize)) != w.view(np.dtype("u%d" % w.itemsize)))
        raise AssertionError("%s: %d of %d samples differ, the first at %d: %r, not %r" % (what, len(bad), g.size, bad[0], g[bad[0]], w[bad[0]]))


def _decode_file_policy(files, fmt, consts=None, windows=None):
    b = jl.Batch().set_color_policy("file")
    if consts is not None:
        b.set_output_affine(*consts)
    if windows is not None:
        b.set_windows(windows)
    return b.upload(files, fmt).decode().sync()


# ------------------------------------------------------------------------------------------------ 1: kinds x sizes x formats

@pytest.mark.parametrize("variant", VARIANTS, ids=V_IDS)
@pytest.mark.parametrize("name", cm.KIND_FILES)
def test_every_kind_at_every_size_in_every_format(name, variant):
    _, fmt, consts = variant
    files = [cm.kind_file(name, w, h)[0] for w, h in SIZES]
    kind = cm.kind_file(name)[1]
    samples = _samples(name, files)
    b = _decode_file_policy(files, fmt, consts)
    for i, (w, h) in enumerate(SIZES):
        assert b.image_info(i).status == 0 and b.result(i).status == 0, (i, b.image_info(i).status, b.result(i).status)
        assert b.color(i) == kind == jl.identify_color(files[i])
        assert samples[i].shape == (h, w, 4 if kind in ("cmyk", "ycck") else 3)
        _assert_bits(b.output(i), cm.as_format(cm.model(kind, samples[i]), fmt, consts), "%s %dx%d" % (name, w, h))
    b.close()


@pytest.mark.parametrize("variant", VARIANTS[:4], ids=V_IDS[:4])
def test_subsampled_ycck_and_progressive_cmyk(variant):
    _, fmt, consts = variant
    files = [cm.subsampled_ycck(), cm.pillow_jpeg(45, 67, "CMYK", progressive=True), cm.patch_adobe_transform(cm.pillow_jpeg(40, 24, "CMYK", progressive=True), 2)]
    assert b"\xff\xc2" in files[1]
    kinds = ["ycck", "cmyk", "ycck"]
    samples = _samples("sub+prog", files)
    b = _decode_file_policy(files, fmt, consts)
    for i, kind in enumerate(kinds):
        assert b.result(i).status == 0 and b.color(i) == kind
        _assert_bits(b.output(i), cm.as_format(cm.model(kind, samples[i]), fmt, consts), "file %d" % i)
    b.close()


# ------------------------------------------------------------------------------------------------ 2: every (s0, s3) pair

def test_every_pair_of_the_cmyk_product():
    """2048 x 2048, four 1x1 components, DC-only blocks under unit quantisation tables: component 0 steps by block column, component 3 by
    block row, so the 256 x 256 blocks hold every (s0, s3) pair; components 1 and 2 run against them."""
    n = 256
    frame = {"width": 8 * n, "height": 8 * n, "precision": 8, "components": [(ord(c), 1, 1, 0) for c in "CMYK"]}
    qt = np.ones((1, 4, 64), np.uint16)
    row, col = np.mgrid[0:n, 0:n]
    values = np.stack([col, (col + row) % 256, (255 - col + 3 * row) % 256, row], axis=-1)  # [block row, block column, component]
    coefs = np.zeros((n * n * 4, 64), np.int16)
    coefs[:, 0] = ((values.reshape(-1).astype(np.int32) - 128) * 8).astype(np.int16)  # sample = DC / 8 + 128

    def run(fmt):
        b = jl.Batch().set_color_policy("file").upload_frames([frame], qt, fmt)
        b.set_coefficients(0, coefs)
        b.run_idct().sync()
        assert b.color(0) == ("cmyk" if fmt != jl.FMT_INTERLEAVED_U8 else "ycbcr")
        out = b.output(0)
        b.close()
        return out

    samples = run(jl.FMT_INTERLEAVED_U8)
    assert samples.shape == (8 * n, 8 * n, 4)
    blocks = samples[::8, ::8]
    pairs = np.unique(blocks[..., 0].astype(np.int64) * 256 + blocks[..., 3])
    assert len(pairs) == 65536  # the output really holds all of them
    _assert_bits(run(jl.FMT_RGB_U8), cm.model("cmyk", samples), "all pairs")


# ------------------------------------------------------------------------------------------------ 3: the mixed upload (scratch-slot neighbours)

def test_mixed_upload_keeps_fast_classes_and_neighbours_intact():
    ycc = bytes(jpegsynth.encode(64, 48, "420", 75, 2, seed=3))
    grey = bytes(jpegsynth.encode(43, 37, "gray", 75, 0, seed=4))  # (odd width: the generic class, whose samples pass through the scratch image too)
    cmyk1, cmyk2 = cm.kind_file("cmyk")[0], cm.kind_file("ycck", 17, 33)[0]
    broken = cmyk1[:len(cmyk1) * 2 // 3]
    files = [ycc, cmyk1, grey, cmyk2, broken]
    kinds = ["ycbcr", "cmyk", "gray", "ycck", "cmyk"]
    ref_b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8).decode().sync()
    ref_status = [ref_b.result(i).status for i in range(5)]
    assert ref_status[:4] == [0, 0, 0, 0] and ref_status[4] != 0
    samples = [ref_b.output(i) for i in range(4)]
    ref_b.close()
    b = _decode_file_policy(files, jl.FMT_RGB_PLANAR_U8)
    work = b.plan_stats()["idct_work"]
    assert work[3] > 0 and work[0] > 0, work  # the 4:2:0 file keeps its fast class; the CMYK files take the generic one
    infos = [b.image_info(i) for i in range(5)]
    # a CMYK image's slot is 4 bytes per pixel although its output is 3: out_bytes stays, the next image moves
    assert infos[1].out_bytes == 3 * 45 * 67 and infos[2].out_offset - infos[1].out_offset >= 4 * 45 * 67
    for i in range(4):
        assert b.result(i).status == 0 and b.color(i) == kinds[i]
        _assert_bits(b.output(i), cm.as_format(cm.model(kinds[i], samples[i]), jl.FMT_RGB_PLANAR_U8), "image %d" % i)
    assert b.result(4).status == ref_status[4]  # the truncated file reports what it reports under the sample format
    b.close()


# ------------------------------------------------------------------------------------------------ 4: windows and the resize stage

WINDOWS = [(0, 0, 0, 0), (8, 16, 16, 24), (5, 3, 30, 29), (44, 66, 1, 1), (0, 7, 45, 1)]


@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[1], VARIANTS[2], VARIANTS[5]], ids=[V_IDS[0], V_IDS[1], V_IDS[2], V_IDS[5]])
@pytest.mark.parametrize("name", ["cmyk", "ycck", "rgb_adobe"])
def test_windows_equal_slices_of_the_whole_decode(name, variant):
    _, fmt, consts = variant
    f, kind = cm.kind_file(name)
    b = _decode_file_policy([f] * len(WINDOWS), fmt, consts, WINDOWS)
    whole = b.output(0)
    _assert_bits(whole, cm.as_format(cm.model(kind, _samples(name + "45", [f])[0]), fmt, consts), name)
    for i, (x, y, w, h) in enumerate(WINDOWS[1:], 1):
        assert b.result(i).status == 0 and b.color(i) == kind and b.window(i) == (x, y, w, h)
        want = whole[:, y:y + h, x:x + w] if whole.shape[0] == 3 else whole[y:y + h, x:x + w]
        _assert_bits(b.output(i), np.ascontiguousarray(want), "%s window %r" % (name, WINDOWS[i]))
    b.close()


@pytest.mark.parametrize("dtype,consts", [(torch.uint8, None), (torch.float16, IMAGENET), (torch.float32, None)], ids=["u8", "f16_imagenet", "f32"])
def test_decode_resized_follows(dtype, consts):
    names = ["cmyk", "rgb_adobe", "ycck"]
    files = [cm.kind_file(n)[0] for n in names]
    samples = _samples("resized", files)
    mean_std = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]) if consts is not None else (None, None)
    out, results = jl.decode_resized(files, (20, 14), dtype, *mean_std, color="file")
    assert [r.status for r in results] == [0, 0, 0] and tuple(out.shape) == (3, 3, 20, 14)
    np_dtype = {torch.uint8: np.uint8, torch.float16: np.float16, torch.float32: np.float32}[dtype]
    got = out.cpu().numpy()
    for i, n in enumerate(names):
        planes = cm.as_format(cm.model(cm.kind_file(n)[1], samples[i]), jl.FMT_RGB_PLANAR_U8)
        _assert_bits(got[i], rm.model(planes, 20, 14, np_dtype, *(consts or ())), n)
    # without the policy the CMYK and YCCK files fail and their slabs read zero
    out, results = jl.decode_resized(files, (20, 14), dtype)
    assert [r.status for r in results] == [NOT_SUPPORTED, 0, NOT_SUPPORTED] and not out[0].cpu().numpy().view(np.uint8).any()


# ------------------------------------------------------------------------------------------------ 5: ingest sources

def test_a_device_file_with_80_kb_in_front_of_its_adobe_marker():
    f = cm.with_app1_padding(cm.kind_file("ycck")[0])
    assert f.index(b"Adobe") > 80000
    plain = cm.kind_file("cmyk", 17, 33)[0]
    samples = _samples("padded", [f, plain])
    tensors = [torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda() for x in (f, plain)]
    b = jl.Batch().set_color_policy("file").upload_tensors(tensors, jl.FMT_RGB_U8).decode().sync()
    assert [b.color(0), b.color(1)] == ["ycck", "cmyk"]
    _assert_bits(b.output(0), cm.model("ycck", samples[0]), "padded")
    _assert_bits(b.output(1), cm.model("cmyk", samples[1]), "plain")
    b.close()
    # ... and as segments cut in front of the marker (the header-only plan sees the first 64 KB of a multi-segment file)
    b = jl.Batch().set_color_policy("file").upload_segments([[f[:1000], f[1000:70000], f[70000:]], [plain]], jl.FMT_RGBA_U8).decode().sync()
    assert [b.color(0), b.color(1)] == ["ycck", "cmyk"]
    _assert_bits(b.output(0), cm.as_format(cm.model("ycck", samples[0]), jl.FMT_RGBA_U8), "padded, segments")
    b.close()
    tensors, results = jl.decode_to_tensors([f, plain], color="file")
    assert [r.status for r in results] == [0, 0]
    _assert_bits(tensors[0].cpu().numpy(), cm.as_format(cm.model("ycck", samples[0]), jl.FMT_RGB_PLANAR_U8), "decode_to_tensors")


# ------------------------------------------------------------------------------------------------ 6: the policy is batch state; the default is unchanged

def test_the_policy_persists_over_uploads_and_can_be_set_back():
    from oracle import pyoracle

    cmyk, rgb = cm.kind_file("cmyk")[0], cm.kind_file("rgb_adobe")[0]
    samples = _samples("state", [cmyk, rgb])
    b = jl.Batch()
    b.upload([cmyk, rgb], jl.FMT_RGB_U8).decode().sync()  # the default: refused, and YCbCr's matrix
    assert b.image_info(0).status == NOT_SUPPORTED and [b.color(0), b.color(1)] == ["ycbcr", "ycbcr"]
    today = b.output(1)
    assert np.array_equal(today, pyoracle.ycbcr8_to_rgb(samples[1])) and not np.array_equal(today, samples[1])
    b.set_color_policy("file")
    for _ in range(2):  # not consumed by an upload
        b.upload([cmyk, rgb], jl.FMT_RGB_U8).decode().sync()
        assert [b.color(0), b.color(1)] == ["cmyk", "rgb"]
        _assert_bits(b.output(0), cm.model("cmyk", samples[0]), "cmyk")
        _assert_bits(b.output(1), samples[1], "rgb")
    b.upload([cmyk, rgb], jl.FMT_INTERLEAVED_U8).decode().sync()  # the sample formats do not read it
    assert [b.color(0), b.color(1)] == ["ycbcr", "ycbcr"] and np.array_equal(b.output(0), samples[0])
    b.set_color_policy("ycc").upload([cmyk, rgb], jl.FMT_RGB_U8).decode().sync()
    assert b.image_info(0).status == NOT_SUPPORTED and np.array_equal(b.output(1), today)
    with pytest.raises(ValueError):
        b.set_color_policy("cmyk")
    assert jl._capi.lib.jpgpu_batch_set_color_policy(b._h, 2) == jl._capi.ERR_ARGUMENT
    b.close()
    outs, results = jl.decode_batch([cmyk, rgb], jl.FMT_RGBA_U8)
    assert outs[0] is None and results[0].status == NOT_SUPPORTED
    outs, results = jl.decode_batch([cmyk, rgb], jl.FMT_RGBA_U8, color="file")
    _assert_bits(outs[0], cm.as_format(cm.model("cmyk", samples[0]), jl.FMT_RGBA_U8), "decode_batch")
