"""Orientation on the GPU: the Exif orientation of a file (policy "file") or a caller-given value, applied by K3O behind K3's generic class.

Every expected value is, bit for bit, the model (tests/orient_model.py: the header's table as numpy indexing) applied to Batch.output(i) of the
SAME upload decoded as stored, in the same format and with the same constants.  Covered: all 8 values under the 7 format variants of the colour
suite at sizes one below, at and one above a tile edge (4:2:0, 4:4:4 and grey files, Exif blocks in both byte orders); the explicit list; the
colour kinds under color="file"; one mixed upload whose unoriented 4:2:0 file keeps its fast class and whose slots' surroundings stay
untouched; windows in oriented coordinates; decode_resized; failing baseline and progressive files; the four ingest sources; the defaults."""
import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from tools import jpegsynth
import color_model as cm
import orient_model as om
import policy_model as pm
import resize_model as rm
from test_color_gpu import VARIANTS, V_IDS, _assert_bits
from test_planar_rgb_gpu import _progressive_file

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 9), (9, 1), (31, 33), (64, 64), (65, 130), (130, 67)]  # (w, h): none a multiple of 4 but the tile itself
SUBS = ["420", "444", "gray"]
ERR_ARGUMENT = jl._capi.ERR_ARGUMENT
_FILES = {}


def _file(w, h, sub, seed=0, dri=0):
    key = (w, h, sub, seed, dri)
    if key not in _FILES:
        _FILES[key] = bytes(jpegsynth.encode(w, h, sub, 85, dri, seed=seed))
    return _FILES[key]


def _decode(files, fmt, consts=None, policy="stored", orientations=None, windows=None, color="ycc"):
    b = jl.Batch().set_color_policy(color).set_orientation_policy(policy)
    if consts is not None:
        b.set_output_affine(*consts)
    if orientations is not None:
        b.set_orientations(orientations)
    if windows is not None:
        b.set_windows(windows)
    return b.upload(files, fmt).decode().sync()


def _stored_size(b, i):
    info = b.image_info(i)
    return info.height, info.width


# ------------------------------------------------------------------------------------------------ 1: values x formats x sizes

def _tagged(o):
    files = []
    for k, (w, h) in enumerate(SIZES):
        for s, sub in enumerate(SUBS):
            files.append(om.with_orientation(_file(w, h, sub, seed=k), o, "MM" if (k + s) & 1 else "II"))
    return files


@pytest.mark.parametrize("variant", VARIANTS, ids=V_IDS)
@pytest.mark.parametrize("o", om.ORIENTATIONS)
def test_every_value_in_every_format_at_every_size(o, variant):
    _, fmt, consts = variant
    files = _tagged(o)
    ref = _decode(files, fmt, consts)  # as stored: the policy's default
    b = _decode(files, fmt, consts, "file")
    for i, f in enumerate(files):
        w, h = SIZES[i // len(SUBS)]
        assert ref.result(i).status == 0 == b.result(i).status, (i, ref.result(i).status, b.result(i).status)
        assert ref.orientation(i) == 1 and b.orientation(i) == o == jl.identify_orientation(f)
        info, stored = b.image_info(i), ref.image_info(i)
        assert (info.width, info.height, info.out_bytes) == (w, h, stored.out_bytes)  # the stored frame's size stays
        oh, ow = om.oriented_size(o, h, w)
        assert b.window(i) == (0, 0, ow, oh) and ref.window(i) == (0, 0, w, h)
        if fmt not in (jl.FMT_RGB_U8, jl.FMT_RGBA_U8):
            assert all((info.plane[c].width, info.plane[c].height, info.plane[c].pitch) == (ow, oh, ow) for c in range(3))
        _assert_bits(b.output(i), om.orient_output(o, ref.output(i), fmt), "orientation %d, %dx%d %s" % (o, w, h, SUBS[i % len(SUBS)]))
    ref.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2: the explicit list

def test_an_explicit_list_overrides_the_file_and_is_consumed_by_one_upload():
    fmt = jl.FMT_RGB_PLANAR_U8
    files = [om.with_orientation(_file(65, 130, "420", seed=k), 6, "II") for k in range(4)] + [_file(31, 33, "444")]
    ref = _decode(files, fmt)
    stored = [ref.output(i) for i in range(5)]
    ref.close()
    given = [0, 3, 1, 8, 2]
    for policy, by_policy in (("file", [6, 3, 1, 8, 2]), ("stored", [1, 3, 1, 8, 2])):
        b = _decode(files, fmt, None, policy, given)
        assert [b.orientation(i) for i in range(5)] == by_policy
        for i, o in enumerate(by_policy):
            _assert_bits(b.output(i), om.orient(o, stored[i], (1, 2)), "%s, image %d" % (policy, i))
        b.upload(files, fmt).decode().sync()  # the list is gone: the policy alone
        after = [6, 6, 6, 6, 1] if policy == "file" else [1] * 5
        assert [b.orientation(i) for i in range(5)] == after
        _assert_bits(b.output(1), om.orient(after[1], stored[1], (1, 2)), "the upload after")
        b.close()
    tensors, results = jl.decode_to_tensors(files, orientation="file", orientations=given)
    assert [r.status for r in results] == [0] * 5 and tuple(tensors[0].shape) == (3, 65, 130) and tuple(tensors[1].shape) == (3, 130, 65)
    _assert_bits(tensors[3].cpu().numpy(), om.orient(8, stored[3], (1, 2)), "decode_to_tensors")
    outs, results = jl.decode_batch(files, jl.FMT_RGB_PLANAR_U8, orientations=[2] * 5)
    _assert_bits(outs[4], om.orient(2, stored[4], (1, 2)), "decode_batch: the horizontal flip")


def test_the_refusals():
    lib, C = jl._capi.lib, jl._capi.C
    f = _file(31, 33, "420")
    b = jl.Batch()
    assert lib.jpgpu_batch_set_orientations(b._h, (C.c_uint8 * 2)(1, 9), 2) == ERR_ARGUMENT  # a value above 8
    assert lib.jpgpu_batch_set_orientations(b._h, None, 1) == ERR_ARGUMENT
    assert lib.jpgpu_batch_set_orientation_policy(b._h, 2) == ERR_ARGUMENT
    with pytest.raises(ValueError):
        b.set_orientation_policy("exif")
    b.upload([f, f], jl.FMT_RGB_U8)  # (the refused list is not pending)
    assert len(b) == 2
    b.set_orientations([6])
    with pytest.raises(jl.ArgumentException):  # n differs: refused, and the batch is left empty
        b.upload([f, f], jl.FMT_RGB_U8)
    assert len(b) == 0
    b.upload([f, f], jl.FMT_RGB_U8).decode().sync()  # ... and the list was consumed by the refusal
    assert [b.orientation(0), b.orientation(1)] == [1, 1]
    b.set_orientations([6, 6]).set_orientations(None)  # withdrawn
    b.upload([f, f], jl.FMT_RGB_U8)
    assert b.orientation(0) == 1
    b.set_orientations([6, 6])
    with pytest.raises(jl.ArgumentException):  # a format that does not read orientation, like windows under PLANAR_U8
        b.upload([f, f], jl.FMT_INTERLEAVED_U8)
    assert len(b) == 0
    b.set_orientations([6])
    frame = {"width": 8, "height": 8, "precision": 8, "components": [(1, 1, 1, 0)]}
    with pytest.raises(jl.ArgumentException):
        b.upload_frames([frame], np.ones((1, 4, 64), np.uint16), jl.FMT_RGB_U8)
    assert len(b) == 0
    o = C.c_int()
    assert lib.jpgpu_batch_image_orientation(b._h, 0, C.byref(o)) == ERR_ARGUMENT  # no such image
    b.close()


# ------------------------------------------------------------------------------------------------ 3: colour kinds

@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[2], VARIANTS[5]], ids=[V_IDS[0], V_IDS[2], V_IDS[5]])
def test_colour_kinds_under_orientations_6_and_7(variant):
    _, fmt, consts = variant
    files = [cm.kind_file("cmyk")[0], cm.subsampled_ycck(), cm.kind_file("rgb_adobe", 17, 33)[0], cm.kind_file("ycck", 70, 66)[0]]
    kinds = ["cmyk", "ycck", "rgb", "ycck"]
    ref = _decode(files, fmt, consts, color="file")
    for o in (6, 7):
        b = _decode([om.with_orientation(f, o) for f in files], fmt, consts, "file", color="file")
        for i, kind in enumerate(kinds):
            assert b.result(i).status == 0 and b.color(i) == kind and b.orientation(i) == o
            _assert_bits(b.output(i), om.orient_output(o, ref.output(i), fmt), "%s under %d" % (kind, o))
            _assert_bits(b.output(i), pm.expected(files[i], arithmetic="reference", scale=1, upsampling="replicate", color="file", mode="rgb", orientation=o, window=None, fmt=fmt, consts=consts, resize=None).output, "%s under %d, the composed model" % (kind, o))
        b.close()
    ref.close()


def test_an_image_whose_window_is_refused_reports_orientation_1_and_ycbcr_as_a_failed_image_does():
    """include/jpgpu.h: jpgpu_batch_image_orientation gives 1 and jpgpu_batch_image_color YCBCR for an image that failed at upload; a window
    outside the oriented frame fails its image at upload.  (The accessors used to hand out what the plan had reached when the window was refused.)"""
    g = _file(31, 33, "gray")
    b = _decode([g, g], jl.FMT_RGB_PLANAR_U8, orientations=[6, 6], windows=[(0, 0, 0, 0), (32, 0, 1, 1)], color="file")  # the oriented frame is 33 x 31: its last column
    assert b.image_info(1).status == 0 and (b.orientation(1), b.color(1)) == (6, "gray")
    b.close()
    b = _decode([g, g], jl.FMT_RGB_PLANAR_U8, orientations=[6, 6], windows=[(0, 0, 0, 0), (33, 0, 1, 1)], color="file")
    assert b.image_info(0).status == 0 and (b.orientation(0), b.color(0)) == (6, "gray")
    assert b.image_info(1).status == ERR_ARGUMENT and b.image_info(1).out_bytes == 0 and (b.orientation(1), b.color(1)) == (1, "ycbcr")
    assert (b.scale(1), b.arithmetic(1), b.upsampling(1), b.channels(1)) == (1, 0, 0, 3)
    b.close()


# ------------------------------------------------------------------------------------------------ 4: one mixed upload

def test_a_mixed_upload_keeps_the_fast_class_and_leaves_the_gaps_alone():
    fmt = jl.FMT_RGB_PLANAR_U8
    ycc = _file(64, 48, "420", seed=3, dri=2)
    cmyk = cm.kind_file("cmyk")[0]
    whole = _file(130, 67, "420", seed=6)
    files = [om.with_orientation(_file(65, 130, "420", seed=5), 6), ycc, om.with_orientation(_file(31, 33, "gray"), 3, "II"), om.with_orientation(cmyk, 5),
             om.with_orientation(whole[:len(whole) * 6 // 10] + b"\xff\xd9", 8)]
    want_o = [6, 1, 3, 5, 8]
    ref = _decode(files, fmt, color="file")
    alone = _decode([ycc], fmt, color="file")
    b = jl.Batch().set_color_policy("file").set_orientation_policy("file").upload(files, fmt)
    base, total = b.output_device_ptr()
    canvas = torch.as_tensor(jl.batch._DeviceView(None, base, (total,)), device="cuda:0")
    canvas.fill_(0xA5)
    torch.cuda.synchronize()
    b.decode().sync()
    work, work_alone = b.plan_stats()["idct_work"], alone.plan_stats()["idct_work"]
    assert work_alone[0] == 0 and work_alone[3] > 0 and work[3] == work_alone[3] and work[0] > 0, (work, work_alone)  # the unoriented file keeps its class
    assert ref.result(4).status != 0 and b.result(4).status == ref.result(4).status
    after = canvas.cpu().numpy()
    end = 0
    for i, o in enumerate(want_o):
        info = b.image_info(i)
        assert b.orientation(i) == o and info.status == 0 and b.result(i).status == ref.result(i).status
        _assert_bits(b.output(i), om.orient(o, ref.output(i), (1, 2)), "image %d" % i)
        assert (after[end:info.out_offset] == 0xA5).all(), "the bytes in front of image %d" % i
        end = info.out_offset + info.out_bytes
    assert (after[end:] == 0xA5).all()
    infos = [b.image_info(i) for i in range(5)]
    assert infos[3].out_bytes == 3 * 45 * 67 and infos[4].out_offset - infos[3].out_offset >= 4 * 45 * 67  # the slot of the CMYK image
    for x in (ref, alone, b):
        x.close()


# ------------------------------------------------------------------------------------------------ 5: windows, in oriented coordinates

@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[1], VARIANTS[2], VARIANTS[6]], ids=[V_IDS[0], V_IDS[1], V_IDS[2], V_IDS[6]])
@pytest.mark.parametrize("o", [3, 6, 8])
def test_windows_are_slices_of_the_oriented_whole_decode(o, variant):
    _, fmt, consts = variant
    w, h = 130, 67
    f = om.with_orientation(_file(w, h, "420", seed=8), o)
    oh, ow = om.oriented_size(o, h, w)
    windows = [(0, 0, 0, 0), (16, 32, 32, 16), (5, 3, 41, 57), (ow - 1, oh - 1, 1, 1), (0, 7, ow, 1), (3, 0, 1, oh), (0, 0, ow, oh),
               # the last: under 6 and 8 inside the stored frame but outside the oriented one; under 3 the two frames coincide: outside both
               (w - 8, 0, 8, 8) if o >= 5 else (0, h + 54, 8, 8)]
    b = _decode([f] * len(windows), fmt, consts, "file", windows=windows)
    whole = b.output(0)
    ref = _decode([f], fmt, consts)
    _assert_bits(whole, om.orient_output(o, ref.output(0), fmt), "whole")
    ref.close()
    planes = fmt not in (jl.FMT_RGB_U8, jl.FMT_RGBA_U8)
    for i, (x, y, ww, hh) in enumerate(windows[1:-1], 1):
        assert b.result(i).status == 0 and b.orientation(i) == o and b.window(i) == (x, y, ww, hh), (i, b.window(i))
        want = whole[:, y:y + hh, x:x + ww] if planes else whole[y:y + hh, x:x + ww]
        _assert_bits(b.output(i), np.ascontiguousarray(want), "window %r under %d" % (windows[i], o))
        if planes:
            info = b.image_info(i)
            assert (info.plane[1].width, info.plane[1].height) == (ww, hh) and (info.width, info.height) == (w, h)
    last = len(windows) - 1
    assert b.image_info(last).status == ERR_ARGUMENT and b.image_info(last - 1).status == 0  # fails alone
    b.close()


# ------------------------------------------------------------------------------------------------ 6: the resize stage

@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16], ids=["u8", "f16"])
def test_decode_resized_reads_the_oriented_image(dtype):
    sizes = [(65, 130), (130, 67), (31, 33), (9, 1)]
    given = [6, 5, 2, 8]
    files = [_file(w, h, "420", seed=k) for k, (w, h) in enumerate(sizes)]
    outs, results = jl.decode_batch(files, jl.FMT_RGB_PLANAR_U8, orientations=given)
    assert [r.status for r in results] == [0] * 4 and outs[0].shape == (3, 65, 130)
    tagged = [om.with_orientation(f, o) for f, o in zip(files, given)]
    np_dtype = {torch.uint8: np.uint8, torch.float16: np.float16}[dtype]
    for kw, fs in (({"orientations": given}, files), ({"orientation": "file"}, tagged)):
        out, results = jl.decode_resized(fs, (20, 14), dtype, **kw)
        assert [r.status for r in results] == [0] * 4 and tuple(out.shape) == (4, 3, 20, 14)
        got = out.cpu().numpy()
        for i in range(4):
            _assert_bits(got[i], rm.model(outs[i], 20, 14, np_dtype), "image %d" % i)


# ------------------------------------------------------------------------------------------------ 7: failing files

@pytest.mark.parametrize("fmt", [jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_U8], ids=["planar_u8", "rgb"])
def test_failing_files_give_the_transform_of_their_partial_picture(fmt):
    base = _file(130, 67, "420", seed=11, dri=3)
    prog = bytearray(_progressive_file())
    sos = [k for k in range(len(prog) - 1) if prog[k] == 0xFF and prog[k + 1] == 0xDA]
    prog[sos[2] + 40] ^= 0x10  # a flipped bit inside the third scan's entropy data
    cut = _progressive_file()
    files = [base[:len(base) * 6 // 10] + b"\xff\xd9", bytes(prog), cut[:len(cut) * 6 // 10] + b"\xff\xd9", _progressive_file()]
    ref = _decode(files, fmt)
    statuses = [ref.result(i).status for i in range(4)]
    assert statuses[0] != 0 and statuses[2] != 0 and statuses[3] == 0, statuses
    stored = [ref.output(i) for i in range(4)]
    assert all(s.any() for s in stored)
    for o in (2, 5, 6):
        b = _decode(files, fmt, orientations=[o] * 4)
        assert [b.result(i).status for i in range(4)] == statuses
        assert b.progressive_replays() == ref.progressive_replays()
        for i in range(4):
            _assert_bits(b.output(i), om.orient_output(o, stored[i], fmt), "file %d under %d" % (i, o))
        b.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 8: ingest sources

def test_every_ingest_source_sees_the_block():
    fmt = jl.FMT_RGB_U8
    plain = _file(65, 130, "420", seed=5)
    files = [om.with_orientation(plain, 6, "II"), cm.insert_after_soi(plain, cm.segment(0xE2, b"\x11" * 40000), cm.segment(0xED, b"\x22" * 40000), om.exif_segment(8)),
             _file(31, 33, "gray")]
    assert files[1].index(b"Exif") > 80000
    ref = _decode([plain, plain, files[2]], fmt)
    want = [om.orient(o, ref.output(i)) for i, o in enumerate([6, 8, 1])]
    ref.close()

    def check(b, what):
        assert [b.orientation(i) for i in range(3)] == [6, 8, 1], what
        for i in range(3):
            _assert_bits(b.output(i), want[i], "%s, file %d" % (what, i))
        b.close()

    check(_decode(files, fmt, None, "file"), "upload")
    check(jl.Batch().set_orientation_policy("file").upload_segments([[f[:700], f[700:50000], f[50000:]] for f in files], fmt).decode().sync(), "segments")
    ctx = jl.default_context()
    arena = ctx.host_alloc(sum(len(f) + 64 for f in files))
    views, pos = [], 0
    for f in files:
        arena[pos:pos + len(f)] = np.frombuffer(f, np.uint8)
        views.append(arena[pos:pos + len(f)])
        pos += (len(f) + 63) // 64 * 64
    check(jl.Batch(ctx).set_orientation_policy("file").upload_segments(views, fmt, pinned=True).decode().sync(), "page-locked")
    tensors = [torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda() for f in files]
    check(jl.Batch().set_orientation_policy("file").upload_tensors(tensors, fmt).decode().sync(), "device files")


# ------------------------------------------------------------------------------------------------ 9: the defaults

def test_the_default_policy_and_the_other_formats_decode_as_stored():
    plain = _file(65, 130, "420", seed=5)
    tagged = om.with_orientation(plain, 6)
    for fmt in (jl.FMT_RGB_U8, jl.FMT_RGB_PLANAR_F16, jl.FMT_INTERLEAVED_U8, jl.FMT_PLANAR_U8):
        a = jl.Batch().upload([plain], fmt).decode().sync()
        variants = [jl.Batch().upload([tagged], fmt)]  # the default policy
        if fmt in (jl.FMT_INTERLEAVED_U8, jl.FMT_PLANAR_U8):
            variants.append(jl.Batch().set_orientation_policy("file").upload([tagged], fmt))  # a format that does not read it
        for b in variants:
            b.decode().sync()
            ia, ib = a.image_info(0), b.image_info(0)
            assert b.orientation(0) == 1 and b.window(0) == a.window(0) == (0, 0, 65, 130)
            assert (ia.width, ia.height, ia.out_bytes, ia.out_offset) == (ib.width, ib.height, ib.out_bytes, ib.out_offset)
            assert [(p.offset, p.width, p.height, p.pitch) for p in ia.plane] == [(p.offset, p.width, p.height, p.pitch) for p in ib.plane]
            assert a.plan_stats()["idct_work"] == b.plan_stats()["idct_work"]
            oa, ob = a.output(0), b.output(0)
            if isinstance(oa, list):
                assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
            else:
                _assert_bits(ob, oa, "format %d" % fmt)
            b.close()
        a.close()
