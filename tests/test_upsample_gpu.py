"""The upsampling policy "fancy" on the GPU: libjpeg's triangle filter for 4:2:0, 4:2:2 and 4:4:0 chroma, applied by K3U behind K3's generic class
(include/jpgpu.h, "Chroma upsampling").

Every expected value is, bit for bit, the model (tests/upsample_model.py, shown to be libjpeg's upsampler by tests/test_upsample_cpu.py) applied
to Batch.output(i) of the same files uploaded as FMT_INTERLEAVED_U8 under the default policies, converted by the reference callers' converter
(color_model.model) and laid out by color_model.as_format.  Covered: the three ratios at sizes one below, at and one above an MCU and a K3U tile
edge under the 7 format variants of the colour suite, with and without restart intervals, a non-interleaved and a progressive file; what stays
replicated; windows; the 8 orientations, given and from Exif; decode_resized; failing files with and without the partial flush; one mixed upload;
the policy's lifetime and the refusals."""
import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from tools import jpegsynth
import color_model as cm
import orient_model as om
import resize_model as rm
import upsample_model as um
from test_color_gpu import VARIANTS, V_IDS, _assert_bits
from test_planar_rgb_gpu import _progressive_file

pytestmark = pytest.mark.gpu

SAMPLING = {"420": ((2, 2), (1, 1), (1, 1)), "422": ((2, 1), (1, 1), (1, 1)), "440": ((1, 2), (1, 1), (1, 1))}
# (w, h): one below, at and one above an MCU edge and a tile's height (16), the first width that filters, odd tails on both axes; the last three
# lie around the tile's width (128)
SIZES = [(5, 1), (5, 2), (6, 5), (9, 9), (15, 17), (16, 16), (17, 31), (33, 17), (64, 64), (65, 130), (130, 67), (127, 15), (128, 16), (129, 33)]
ERR_ARGUMENT = jl._capi.ERR_ARGUMENT
_FILES, _SAMPLES = {}, {}


def _file(w, h, sub, seed=0, dri=0, **kw):
    key = (w, h, sub, seed, dri, tuple(sorted(kw.items())))
    if key not in _FILES:
        _FILES[key] = bytes(jpegsynth.encode(w, h, "444", 85, dri, seed=seed, sampling=SAMPLING[sub], **kw))
    return _FILES[key]


def _samples(files, partial_flush=True):
    """the INTERLEAVED_U8 output of every file under the default policies (None where the upload refused the file), decoded once per file"""
    missing = [f for f in dict.fromkeys(files) if (f, partial_flush) not in _SAMPLES]
    if missing:
        b = jl.Batch()
        b.set_partial_flush(partial_flush)
        b.upload(missing, jl.FMT_INTERLEAVED_U8).decode().sync()
        for i, f in enumerate(missing):
            b.result(i)
            _SAMPLES[(f, partial_flush)] = b.output(i) if b.image_info(i).status == 0 else None
        b.close()
    return [_SAMPLES[(f, partial_flush)] for f in files]


def _filtered_rgb(f, I):
    """uint8[H, W, 3]: the RGB pixels of the filtered stored decode of file f, whose INTERLEAVED_U8 decode is I"""
    r = um.ratio(f)
    assert r is not None and um.qualifies(f)
    return cm.model("ycbcr", um.filtered(I, *r))


def _decode(files, fmt, consts=None, upsampling="fancy", windows=None, orientation="stored", orientations=None, color="ycc", partial_flush=True):
    b = jl.Batch().set_color_policy(color).set_orientation_policy(orientation).set_upsampling_policy(upsampling)
    b.set_partial_flush(partial_flush)
    if consts is not None:
        b.set_output_affine(*consts)
    if orientations is not None:
        b.set_orientations(orientations)
    if windows is not None:
        b.set_windows(windows)
    return b.upload(files, fmt).decode().sync()


def _same_geometry(a, b, i):
    ia, ib = a.image_info(i), b.image_info(i)
    assert (ia.status, ia.width, ia.height, ia.out_bytes) == (ib.status, ib.width, ib.height, ib.out_bytes), i
    assert [(p.offset, p.width, p.height, p.pitch) for p in ia.plane] == [(p.offset, p.width, p.height, p.pitch) for p in ib.plane], i


# ------------------------------------------------------------------------------------------------ 1: values x formats x sizes x ratios

def _value_files():
    files, what = [], []
    for k, (w, h) in enumerate(SIZES):
        for s, sub in enumerate(SAMPLING):
            files.append(_file(w, h, sub, seed=k, dri=4 if (k + s) & 1 else 0))
            what.append("%dx%d %s dri %d" % (w, h, sub, 4 if (k + s) & 1 else 0))
    for sub in SAMPLING:
        files.append(_file(65, 67, sub, seed=40, noninterleaved=True))
        what.append("65x67 %s, three scans" % sub)
        files.append(_file(65, 67, sub, seed=41, progressive=True))
        what.append("65x67 %s, progressive" % sub)
    files.append(_progressive_file())
    what.append("a progressive 4:2:0 file from Pillow")
    return files, what


@pytest.mark.parametrize("variant", VARIANTS, ids=V_IDS)
def test_every_ratio_in_every_format_at_every_size(variant):
    _, fmt, consts = variant
    files, what = _value_files()
    samples = _samples(files)
    ref = _decode(files, fmt, consts, "replicate")
    b = _decode(files, fmt, consts)
    differs = 0
    for i, f in enumerate(files):
        assert b.result(i).status == 0 == ref.result(i).status, (what[i], b.result(i).status)
        assert b.upsampling(i) == 1 and ref.upsampling(i) == 0, what[i]
        _same_geometry(ref, b, i)
        _assert_bits(ref.output(i), cm.as_format(cm.model("ycbcr", samples[i]), fmt, consts), "replicated: " + what[i])
        want = cm.as_format(_filtered_rgb(f, samples[i]), fmt, consts)
        _assert_bits(b.output(i), want, what[i])
        differs += ref.output(i).tobytes() != want.tobytes()
    assert differs > len(files) // 2  # (the filter is another picture than the replication, on most files: the comparison above is not vacuous)
    ref.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2: what stays replicated

def test_what_the_rule_does_not_name_stays_replicated():
    fmt = jl.FMT_RGB_U8
    plain = [bytes(jpegsynth.encode(45, 67, "444", 85, 0, seed=1)), bytes(jpegsynth.encode(45, 67, "gray", 85, 0, seed=2)),
             bytes(jpegsynth.encode(70, 33, "444", 85, 0, seed=3, sampling=((4, 1), (1, 1), (1, 1)))),
             bytes(jpegsynth.encode(70, 33, "444", 85, 0, seed=4, sampling=((2, 2), (2, 1), (1, 1))))]
    narrow = [_file(w, 19, sub, seed=w) for sub in ("420", "422") for w in (1, 2, 3, 4)]
    kinds = [cm.kind_file("cmyk")[0], cm.subsampled_ycck()]
    twelve = cm.patch_precision(_file(33, 17, "420", seed=7), 12)
    files = plain + narrow + kinds + [twelve, _file(5, 19, "420", seed=5)]
    assert [um.qualifies(f) for f in plain[2:] + narrow] == [False] * 10 and um.qualifies(files[-1])
    ref = _decode(files, fmt, None, "replicate", color="file")
    b = _decode(files, fmt, color="file")
    last = len(files) - 1
    for i in range(last):
        assert b.upsampling(i) == 0 == ref.upsampling(i), i
        _same_geometry(ref, b, i)
        assert b.image_info(i).out_offset == ref.image_info(i).out_offset
        if i == last - 1:
            assert b.image_info(i).status != 0  # the 12-bit frame: refused as ever
            continue
        assert b.result(i).status == 0 == ref.result(i).status, i
        assert b.color(i) == ref.color(i)
        _assert_bits(b.output(i), ref.output(i), "file %d" % i)
    assert b.upsampling(last) == 1 and b.output(last).tobytes() != ref.output(last).tobytes()  # (the same upload does filter the file the rule names)
    assert b.plan_stats()["idct_work"][1:] == ref.plan_stats()["idct_work"][1:]  # the others keep their classes
    ref.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 3: windows

@pytest.mark.parametrize("variant", [VARIANTS[0], VARIANTS[5]], ids=[V_IDS[0], V_IDS[5]])
@pytest.mark.parametrize("sub", list(SAMPLING))
def test_windows_are_slices_of_the_filtered_whole_decode(sub, variant):
    _, fmt, consts = variant
    assert fmt in (jl.FMT_RGB_U8, jl.FMT_RGB_PLANAR_F16)
    w, h = 149, 51
    windows = [(0, 0, 0, 0), (5, 3, 41, 37), (0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1), (73, 25, 1, 1), (16, 16, 32, 32),
               (w - 29, h - 21, 29, 21), (1, 1, w - 1, h - 1), (127, 15, 3, 3), (7, 0, 141, 17), (w, 0, 1, 1)]
    # one scan with restart intervals; a progressive frame (the store holds samples); three scans (K3 walks the whole MCU grid for the window)
    for kind, f in (("baseline", _file(w, h, sub, seed=9, dri=3)), ("progressive", _file(w, h, sub, seed=10, progressive=True)),
                    ("three scans", _file(w, h, sub, seed=11, noninterleaved=True))):
        b = _decode([f] * len(windows), fmt, consts, windows=windows)
        whole = b.output(0)
        _assert_bits(whole, cm.as_format(_filtered_rgb(f, _samples([f])[0]), fmt, consts), "whole, " + kind)
        planes = fmt not in (jl.FMT_RGB_U8, jl.FMT_RGBA_U8)
        for i, (x, y, ww, hh) in enumerate(windows[1:-1], 1):
            assert b.result(i).status == 0 and b.upsampling(i) == 1 and b.window(i) == (x, y, ww, hh), (i, b.window(i))
            want = whole[:, y:y + hh, x:x + ww] if planes else whole[y:y + hh, x:x + ww]
            _assert_bits(b.output(i), np.ascontiguousarray(want), "window %r of %s, %s" % (windows[i], sub, kind))
        last = len(windows) - 1
        assert b.image_info(last).status == ERR_ARGUMENT and b.upsampling(last) == 0 and b.image_info(last - 1).status == 0  # fails alone
        b.close()


# ------------------------------------------------------------------------------------------------ 4: orientation

@pytest.mark.parametrize("source", ["given", "exif"])
@pytest.mark.parametrize("o", om.ORIENTATIONS)
def test_orientation_turns_the_filtered_picture(o, source):
    plain = [_file(w, h, sub, seed=20 + k) for k, (w, h) in enumerate([(31, 33), (65, 130)]) for sub in SAMPLING]
    samples = _samples(plain)
    files = [om.with_orientation(f, o, "MM" if k & 1 else "II") for k, f in enumerate(plain)] if source == "exif" else plain
    for _, fmt, consts in (VARIANTS[0], VARIANTS[5]):
        kw = {"orientation": "file"} if source == "exif" else {"orientations": [o] * len(files)}
        b = _decode(files, fmt, consts, **kw)
        for i, f in enumerate(plain):
            assert b.result(i).status == 0 and b.orientation(i) == o and b.upsampling(i) == 1, i
            stored = cm.as_format(_filtered_rgb(f, samples[i]), fmt, consts)
            _assert_bits(b.output(i), om.orient_output(o, stored, fmt), "file %d under %d" % (i, o))
        b.close()


@pytest.mark.parametrize("o", [3, 6, 8])
def test_a_window_of_an_oriented_filtered_image_is_given_in_oriented_coordinates(o):
    fmt = jl.FMT_RGB_PLANAR_U8
    w, h = 130, 67
    for sub in SAMPLING:
        f = _file(w, h, sub, seed=8)
        oh, ow = om.oriented_size(o, h, w)
        windows = [(0, 0, 0, 0), (5, 3, 41, 57), (ow - 1, oh - 1, 1, 1), (16, 32, 32, 16)]
        b = _decode([f] * len(windows), fmt, windows=windows, orientations=[o] * len(windows))
        whole = om.orient_output(o, cm.as_format(_filtered_rgb(f, _samples([f])[0]), fmt), fmt)
        _assert_bits(b.output(0), whole, "whole")
        for i, (x, y, ww, hh) in enumerate(windows[1:], 1):
            assert b.result(i).status == 0 and b.upsampling(i) == 1 and b.window(i) == (x, y, ww, hh)
            _assert_bits(b.output(i), np.ascontiguousarray(whole[:, y:y + hh, x:x + ww]), "window %r of %s under %d" % (windows[i], sub, o))
        b.close()


# ------------------------------------------------------------------------------------------------ 5: the resize stage

@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16], ids=["u8", "f16"])
def test_decode_resized_resamples_the_filtered_picture(dtype):
    files = [_file(65, 130, "420", seed=1), _file(130, 67, "422", seed=2), _file(31, 33, "440", seed=3), _file(4, 9, "420", seed=4)]
    samples = _samples(files)
    planes = [cm.as_format(_filtered_rgb(f, s) if um.qualifies(f) else cm.model("ycbcr", s), jl.FMT_RGB_PLANAR_U8) for f, s in zip(files, samples)]
    np_dtype = {torch.uint8: np.uint8, torch.float16: np.float16}[dtype]
    out, results = jl.decode_resized(files, (20, 14), dtype, upsampling="fancy", windows=[(0, 0, 0, 0), (3, 5, 100, 40), (0, 0, 0, 0), (0, 0, 0, 0)])
    assert [r.status for r in results] == [0] * 4 and tuple(out.shape) == (4, 3, 20, 14)
    planes[1] = np.ascontiguousarray(planes[1][:, 5:45, 3:103])
    got = out.cpu().numpy()
    for i in range(4):
        _assert_bits(got[i], rm.model(planes[i], 20, 14, np_dtype), "image %d" % i)
    plain, _ = jl.decode_resized(files, (20, 14), dtype)
    assert plain.cpu().numpy()[0].tobytes() != got[0].tobytes()
    tensors, results = jl.decode_to_tensors(files[:1], upsampling="fancy")
    _assert_bits(tensors[0].cpu().numpy(), planes[0], "decode_to_tensors")
    outs, results = jl.decode_batch(files[:1], jl.FMT_RGB_PLANAR_U8, upsampling="fancy")
    _assert_bits(outs[0], planes[0], "decode_batch")


# ------------------------------------------------------------------------------------------------ 6: failing files

@pytest.mark.parametrize("partial_flush", [True, False], ids=["partial_flush", "no_partial_flush"])
@pytest.mark.parametrize("fmt", [jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_U8], ids=["planar_u8", "rgb"])
def test_failing_files_give_the_filter_of_their_partial_picture(fmt, partial_flush):
    base = _file(130, 67, "420", seed=11, dri=3)
    base422 = _file(130, 67, "422", seed=12, dri=0)
    prog = bytearray(_progressive_file())
    sos = [k for k in range(len(prog) - 1) if prog[k] == 0xFF and prog[k + 1] == 0xDA]
    prog[sos[2] + 40] ^= 0x10  # a flipped bit inside the third scan's entropy data
    cut = _progressive_file()
    files = [base[:len(base) * 6 // 10] + b"\xff\xd9", bytes(prog), cut[:len(cut) * 6 // 10] + b"\xff\xd9", _progressive_file(),
             base422[:len(base422) * 6 // 10] + b"\xff\xd9"]
    samples = _samples(files, partial_flush)
    ref = _decode(files, fmt, None, "replicate", partial_flush=partial_flush)
    statuses = [ref.result(i).status for i in range(len(files))]
    assert statuses[0] != 0 and statuses[2] != 0 and statuses[3] == 0 and statuses[4] != 0, statuses
    b = _decode(files, fmt, partial_flush=partial_flush)
    assert [b.result(i).status for i in range(len(files))] == statuses
    assert b.progressive_replays() == ref.progressive_replays()
    for i, f in enumerate(files):
        assert b.upsampling(i) == 1 and samples[i].any()
        _assert_bits(ref.output(i), cm.as_format(cm.model("ycbcr", samples[i]), fmt), "replicated, file %d" % i)
        _assert_bits(b.output(i), cm.as_format(_filtered_rgb(f, samples[i]), fmt), "file %d" % i)
    # ... and turned as well: K3O behind K3U, on the second issue too
    t = _decode(files, fmt, orientations=[6] * len(files), partial_flush=partial_flush)
    assert [t.result(i).status for i in range(len(files))] == statuses
    for i, f in enumerate(files):
        _assert_bits(t.output(i), om.orient_output(6, cm.as_format(_filtered_rgb(f, samples[i]), fmt), fmt), "file %d, turned" % i)
    for x in (ref, b, t):
        x.close()


# ------------------------------------------------------------------------------------------------ 7: one mixed upload

def test_a_mixed_upload_keeps_the_neighbours_classes_and_leaves_the_gaps_alone():
    fmt = jl.FMT_RGB_PLANAR_U8
    f444 = bytes(jpegsynth.encode(64, 48, "444", 85, 2, seed=3))
    gray = bytes(jpegsynth.encode(64, 40, "gray", 85, 0, seed=4))  # (both neighbours of sizes their fast classes take: whole blocks per line)
    f444b = bytes(jpegsynth.encode(24, 9, "444", 85, 0, seed=8))
    filtered = [_file(65, 130, "420", seed=5), _file(33, 17, "422", seed=6, dri=4), _file(130, 67, "440", seed=7)]
    files = [f444, filtered[0], gray, filtered[1], f444b, filtered[2]]
    turned = [1, 1, 1, 6, 1, 1]
    samples = _samples(files)
    without = _decode([f444, gray, f444b], fmt)
    b = jl.Batch().set_upsampling_policy("fancy")
    b.set_orientations(turned)
    b.upload(files, fmt)
    base, total = b.output_device_ptr()
    canvas = torch.as_tensor(jl.batch._DeviceView(None, base, (total,)), device="cuda:0")
    canvas.fill_(0xA5)
    torch.cuda.synchronize()
    b.decode().sync()
    work, work_without = b.plan_stats()["idct_work"], without.plan_stats()["idct_work"]
    assert work_without[0] == 0 and sum(work_without[1:]) > 0 and work[1:] == work_without[1:] and work[0] > 0, (work, work_without)
    after = canvas.cpu().numpy()
    end = 0
    for i, f in enumerate(files):
        info = b.image_info(i)
        assert info.status == 0 and b.result(i).status == 0 and b.upsampling(i) == (1 if f in filtered else 0), i
        rgb = _filtered_rgb(f, samples[i]) if f in filtered else cm.model("gray" if f is gray else "ycbcr", samples[i])
        _assert_bits(b.output(i), om.orient_output(turned[i], cm.as_format(rgb, fmt), fmt), "image %d" % i)
        assert (after[end:info.out_offset] == 0xA5).all(), "the bytes in front of image %d" % i
        end = info.out_offset + info.out_bytes
    assert (after[end:] == 0xA5).all()
    without.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 8: the policy's lifetime, the defaults, the refusals

def test_the_policy_holds_until_it_is_set_again():
    fmt = jl.FMT_RGB_U8
    f = _file(65, 130, "420", seed=5)
    want = {1: cm.as_format(_filtered_rgb(f, _samples([f])[0]), fmt), 0: cm.as_format(cm.model("ycbcr", _samples([f])[0]), fmt)}
    assert want[0].tobytes() != want[1].tobytes()
    b = jl.Batch()
    for policy, applied in ((None, 0), ("fancy", 1), (None, 1), (None, 1), ("replicate", 0), (None, 0)):
        if policy is not None:
            b.set_upsampling_policy(policy)
        b.upload([f], fmt).decode().sync()
        assert b.upsampling(0) == applied
        _assert_bits(b.output(0), want[applied], "policy %r" % (policy,))
    b.close()


def test_the_default_policy_and_the_other_formats_never_heard_of_it():
    f = _file(65, 130, "420", seed=5)
    for fmt in (jl.FMT_RGB_U8, jl.FMT_RGB_PLANAR_F16, jl.FMT_INTERLEAVED_U8, jl.FMT_PLANAR_U8, jl.FMT_PLANAR_I16, jl.FMT_INTERLEAVED_U8_SCALED):
        a = jl.Batch().upload([f], fmt).decode().sync()
        variants = [jl.Batch().set_upsampling_policy("replicate").upload([f], fmt)]
        if fmt not in (jl.FMT_RGB_U8, jl.FMT_RGB_PLANAR_F16):
            variants.append(jl.Batch().set_upsampling_policy("fancy").upload([f], fmt))  # a format that does not read it
        for b in variants:
            b.decode().sync()
            assert b.upsampling(0) == 0 == a.upsampling(0)
            _same_geometry(a, b, 0)
            assert a.image_info(0).out_offset == b.image_info(0).out_offset
            assert a.plan_stats()["idct_work"] == b.plan_stats()["idct_work"]
            oa, ob = a.output(0), b.output(0)
            if isinstance(oa, list):
                assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
            else:
                _assert_bits(ob, oa, "format %d" % fmt)
            b.close()
        a.close()


def test_the_event_pair_around_k3u_is_recorded_on_request_only(monkeypatch):
    f = _file(65, 130, "420", seed=5)
    b = jl.Batch().set_upsampling_policy("fancy").upload([f], jl.FMT_RGB_U8).decode().sync()
    with pytest.raises(jl.InvalidOperationException):
        b.upsampling_ms()
    monkeypatch.setenv("JPGPU_TIME_UPSAMPLE", "1")
    b.upload([f], jl.FMT_RGB_U8)
    with pytest.raises(jl.InvalidOperationException):  # not decoded yet
        b.upsampling_ms()
    b.decode().sync()
    assert b.upsampling_ms() > 0
    b.set_upsampling_policy("replicate").upload([f], jl.FMT_RGB_U8).decode().sync()
    with pytest.raises(jl.InvalidOperationException):  # no filtered image
        b.upsampling_ms()
    assert jl._capi.lib.jpgpu_batch_upsampling_ms(b._h, None) == ERR_ARGUMENT
    b.close()


def test_the_refusals():
    lib, C = jl._capi.lib, jl._capi.C
    b = jl.Batch()
    for bad in (2, -1, 7):
        assert lib.jpgpu_batch_set_upsampling_policy(b._h, bad) == ERR_ARGUMENT
    with pytest.raises(ValueError):
        b.set_upsampling_policy("triangle")
    f = _file(33, 17, "420", seed=7)
    b.upload([f], jl.FMT_RGB_U8).decode().sync()
    assert b.upsampling(0) == 0  # (a refused value changes nothing)
    applied = C.c_int()
    assert lib.jpgpu_batch_image_upsampling(b._h, 1, C.byref(applied)) == ERR_ARGUMENT  # no such image
    assert lib.jpgpu_batch_image_upsampling(b._h, 0, None) == ERR_ARGUMENT
    b.close()
