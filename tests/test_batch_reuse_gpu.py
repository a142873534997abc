"""One Batch, and one JpegDecoder, used for upload after upload of differing content -- what a data loader does with them.

A DeviceBatch carries grow-only device buffers (output, scratch image, coefficient store and its dense copy, split planes and flag words,
the K2S arrays, the progressive store, staging, the resize buffer, the ticket counters) and some fifty host fields from one upload to the
next.  Every other suite decodes each upload in a fresh, exactly sized Batch.  Here one Batch goes through sequences whose every upload
lands in what another road left behind: LOUD files (tests/reuse_cases.py: no zero sample, no zero last coefficient) in front of QUIET
ones that leave part of their slot unwritten, and in front of every quiet decode the bytes of the coming slots are read from the device
and are still the loud image's, all nonzero -- a missing clear cannot hide behind a buffer that happened to be zero.

Expected values come from the oracle (po.decode_8bit_partial, po.decode_coefficients, po.decode_16bit), from policy_model.expected and
resize_model, and -- as a second witness only -- from a fresh Batch of the same upload; never from the reused batch.  Every comparison is
exact.  test_batch_reuse_inputs_cpu.py proves the inputs, test_decoder_reuse_cpu.py the host-only half of the decoder mirror."""
import numpy as np
import pytest
import torch

import islow_model as im
import jpeglibrary_amd as jl
import policy_model as pm
import reuse_cases as rc
import test_policy_matrix_gpu as matrix
from oracle import pyoracle as po
from test_color_gpu import _assert_bits

pytestmark = pytest.mark.gpu
NAMES = {0: "OK", 1: "InvalidDataException", 2: "InvalidOperationException", 3: "NotSupportedException", 4: "ArgumentException"}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("JPGPU_DENSE_HANDOFF", "JPGPU_SUBSEQ_SHIFT", "JPGPU_SUBSEQ_TWO_PER_LANE_FROM", "JPGPU_SUBSEQ_BUDGET", "JPGPU_OVERLAP", "JPGPU_NO_PARTIAL_FLUSH",
                 "JPGPU_PROG_NO_PIPELINE", "JPGPU_PROG_SPIN_BUDGET", "JPGPU_K1_SPIN_BUDGET", "JPGPU_PROG_FORCE_PIPELINE"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture
def every_scan_split(monkeypatch):
    """The planner splits a scan's hand-off by itself only up to eight bytes of entropy data a block, which leaves quality 100 out;
    JPGPU_DENSE_HANDOFF=0 (read per upload) splits every scan K3 has the split form for, so the loud files take that road too."""
    monkeypatch.setenv("JPGPU_DENSE_HANDOFF", "0")


def _device_bytes(b, off=0, n=None):
    """a copy of the batch's output buffer as it is now"""
    base, total = b.output_device_ptr()
    n = total - off if n is None else n
    assert base and off + n <= total
    return torch.as_tensor(jl.batch._DeviceView(None, base + off, (n,)), device="cuda:0").cpu().numpy()


def _single_scan(f):
    return len(rc._sos_offsets(f)) == 1


def _check_u8(b, files, what):
    """every image of an INTERLEAVED_U8 upload against the oracle: status class, bytes, coefficients where the file decodes cleanly"""
    assert len(b) == len(files), what
    for i, f in enumerate(files):
        kind, px, coefs = rc.reference(f)
        res = b.result(i)
        assert NAMES[res.status] == kind, (what, i, kind, res.status, res.detail)
        if px is None:
            continue
        assert b.image_info(i).status == 0, (what, i)
        _assert_bits(b.output(i), px, "%s, image %d (%s)" % (what, i, kind))
        if coefs is not None and _single_scan(f):  # (the oracle taps a multi-scan file scan by scan, the batch keeps MCU order)
            _assert_bits(b.coefficients(i), coefs, "%s, coefficients of image %d" % (what, i))
        if f == rc.band_1_5():  # (what the writer was given: the band no scan writes is zero in the store, not the loud upload's)
            assert not rc.band_store()[:, 6:].any() and rc.band_store()[:, 1:6].any()
            _assert_bits(b.coefficients(i), rc.band_store(), "%s, the store of image %d" % (what, i))
        if f in _progressive_three():  # (whole MCUs: the oracle's store, block for block)
            _assert_bits(b.coefficients(i), rc.progressive_store(f), "%s, the store of image %d" % (what, i))


def _road(b, road, n, split=True):
    """split: the upload's format has the split form of K3 (INTERLEAVED_U8 has it for every class)"""
    st = b.plan_stats()
    if road == "k2":  # the five 4:2:0 files are one pooled run, the grey one another; single-scan DRI != 0 files are handed over split
        assert st["k2_pools"] == 2 and st["k2_pooled_chunks"] == 5 * 2 + 6 and st["k2s_subs"] == 0 and (sum(st["idct_split_work"]) > 0 or not split), st
    elif road == "quiet":
        assert st["k2_plain_work"] + st["k2_pooled_chunks"] > 0 and st["k2s_subs"] == 0, st
    elif road == "k2s":
        assert st["k2s_scans"] == n and st["k2s_subs"] > n and st["k2_plain_work"] + st["k2_pools"] == 0, st
    elif road == "progressive":
        assert b.progressive_plan()["scans"] >= 2 * n and st["k2s_subs"] == 0 and st["k2_plain_work"] + st["k2_pools"] == 0, (st, b.progressive_plan())
    elif road == "empty":
        assert st["k2_plain_work"] + st["k2_pools"] + st["k2s_scans"] + sum(st["idct_work"]) == 0 and b.progressive_plan()["scans"] == 0, st


def _k2s_pair():
    return [rc.loud_k2s(0), rc.loud_k2s(1)]


def _progressive_three():
    return [rc.loud_progressive(k) for k in range(3)]


# (name, files, road, does it land in a loud upload's bytes)
SEQUENCE = [("loud K2", rc.loud_k2_upload, "k2", False), ("quiet: truncated DRI 4, missing scan, black", rc.quiet_upload, "quiet", True),
            ("loud K2S", _k2s_pair, "k2s", False), ("quiet: truncated DRI 0", lambda: [rc.truncated(0)], "k2s", True),
            ("loud progressive", _progressive_three, "progressive", False), ("quiet: band 1..5, and cut", rc.band_upload, "progressive", True),
            ("empty", list, "empty", False), ("loud K2 again", rc.loud_k2_upload, "k2", False)]


def _check_empty(b):
    """jpgpu_batch_upload with n == 0 (include/jpgpu.h): a usable batch of no images"""
    assert len(b) == 0 and b.totals() == {"compressed_bytes": 0, "blocks": 0, "pixels": 0, "output_bytes": 0}
    assert b.output_device_ptr()[1] == 0
    b.decode().sync()
    b.run_entropy().run_idct().sync()
    for call in (b.image_info, b.result, b.output, b.window, b.scale):
        with pytest.raises(jl.JpegError):
            call(0)
    st = b.ingest_stats()
    assert st["n_header_only"] + st["n_full_walk"] == 0, st


# ------------------------------------------------------------------------------------------------ a. the roads of the entropy stage

def test_the_roads_of_the_entropy_stage_by_turns_interleaved_u8(every_scan_split):
    b = jl.Batch()
    loud = first = None
    for name, make, road, lands_in_loud in SEQUENCE:
        files = make()
        b.upload(files, jl.FMT_INTERLEAVED_U8)
        _road(b, road, len(files))
        if road == "empty":
            _check_empty(b)
            continue
        if lands_in_loud:  # the precondition, on the device: the coming slots still hold the loud upload's bytes, none of them zero
            for i in range(len(files)):
                info = b.image_info(i)
                assert info.status == 0 and info.out_bytes > 0 and info.out_offset + info.out_bytes <= len(loud), (name, i, info.out_offset, info.out_bytes, len(loud))
                now = _device_bytes(b, info.out_offset, info.out_bytes)
                assert now.all() and np.array_equal(now, loud[info.out_offset:info.out_offset + info.out_bytes]), (name, i, int((now == 0).sum()))
        b.decode().sync()
        _check_u8(b, files, name)
        if road == "progressive":
            assert b.progressive_plan()["launch_form"] != "none", name
        if road == "k2s":
            assert b.subseq_rounds() > 0, name
        outs = [b.output(i).tobytes() for i in range(len(files))]
        b.decode().sync()
        assert [b.output(i).tobytes() for i in range(len(files))] == outs, "the second decode of " + name
        if not lands_in_loud:
            loud = _device_bytes(b)
            assert loud.all(), (name, int((loud == 0).sum()))  # (whole MCUs, whole multiples of 256 bytes: the slots lie back to back)
        if first is None:
            first = outs
        elif name == "loud K2 again":
            assert outs == first
    b.close()


FORMATS = [jl.FMT_PLANAR_U8, jl.FMT_PLANAR_I16, jl.FMT_EXTENDED_U16, jl.FMT_RGB_U8, jl.FMT_RGBA_U8, jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_PLANAR_F16]


def _has_holes(f):
    """files whose decode leaves samples unwritten.  For the two that are no truncated sequential scan (a component without a scan, the partial
    flush of a progressive frame) the oracle decides the pixels it reached in the RGB formats and the fresh batch witnesses the rest"""
    return f in (rc.truncated(4), rc.truncated(0), rc.missing_last_scan(), rc.band_1_5_cut())


def _reached_rows(f):
    """a truncated file: (lines every sample of which the reference wrote, the line from which on it wrote none) -- the MCU row of the
    block it threw in lies between them; None for any other file"""
    if f not in (rc.truncated(4), rc.truncated(0)):
        return None
    W, H, _, comps = im.frame(f)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    row = rc.blocks_before_the_error(f)[0] // sum(c[1] * c[2] for c in comps) // -(-W // (8 * hmax))
    return row * 8 * vmax, (row + 1) * 8 * vmax


def _as_list(out):
    return [np.asarray(p) for p in out] if isinstance(out, list) else [out]


def _check_format(b, i, f, fmt, witness, what):
    kind, px, _ = rc.reference(f)
    assert NAMES[b.result(i).status] == kind == NAMES[witness.result(i).status], (what, kind)
    if px is None:
        return
    got = b.output(i)
    for g, w in zip(_as_list(got), _as_list(witness.output(i))):
        _assert_bits(g, w, what + ": the fresh batch")
    H, W, C = px.shape
    whole = kind == "OK" and not _has_holes(f)
    if fmt in (jl.FMT_PLANAR_U8, jl.FMT_PLANAR_I16):
        comps = im.frame(f)[3]
        hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
        for c in range(C):
            p = np.asarray(got[c])
            p = np.clip(p, 0, 255).astype(np.uint8) if fmt == jl.FMT_PLANAR_I16 else p
            up = np.repeat(np.repeat(p, vmax // comps[c][2], axis=0), hmax // comps[c][1], axis=1)[:H, :W]
            _assert_bits(np.ascontiguousarray(up), np.ascontiguousarray(px[..., c]), "%s: plane %d" % (what, c))
        return
    rows = _reached_rows(f)
    if fmt == jl.FMT_EXTENDED_U16:
        if whole:
            _assert_bits(got, po.decode_16bit(f, 4)[0], what)
        elif rows is not None:  # (a sample the 8-bit writer clamped to 0 may be negative, which this writer clamps to the maximum: those are left out)
            top = px[:rows[0]]
            assert np.array_equal(got[:rows[0], :, :C][top != 0], top[top != 0].astype(np.uint16) * 257) and not got[rows[1]:].any(), what
        return
    rgb = po.ycbcr8_to_rgb(px, rgba=fmt == jl.FMT_RGBA_U8, gray=C == 1)
    if fmt in (jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_PLANAR_F16):
        rgb = np.ascontiguousarray(rgb.transpose(2, 0, 1))
        if fmt == jl.FMT_RGB_PLANAR_F16:  # (the default constants: the byte as a float)
            as_bytes = got.astype(np.uint8)
            _assert_bits(got, as_bytes.astype(np.float16), what + ": whole bytes as float16")
            got = as_bytes
        reached = px.all(axis=2)[None].repeat(3, axis=0)
    else:
        reached = px.all(axis=2)[..., None].repeat(rgb.shape[2], axis=2)
    # (a sequential scan that fails: K3 sends the blocks the reference never reached through the same output code with zero SAMPLES, so the
    # pixels there are the conversion of zeros, as they are for the reference's caller who converts the whole buffer -- the oracle decides
    # every byte, and a stale byte under the hole cannot pass)
    if whole or rows is not None:
        _assert_bits(got, rgb, what)
    else:
        assert np.array_equal(got[reached], rgb[reached]), what


def test_the_same_sequence_with_the_format_changing_at_every_upload(every_scan_split):
    """the planes buffer, the extend descriptors and the scratch image reused by formats of other widths.  (That a quiet image lands inside
    nonzero bytes of the upload before it is proven by the INTERLEAVED_U8 run alone: the slots and plane paddings of these formats differ, so
    here a stale byte may or may not lie under a hole.  What this run adds is the buffers' reuse across sample widths.)"""
    b = jl.Batch()
    step = 0
    for name, make, road, _ in SEQUENCE:
        files = make()
        fmt = FORMATS[step % len(FORMATS)]
        b.upload(files, fmt)
        _road(b, road, len(files), split=False)
        if road == "empty":
            _check_empty(b)
            continue
        step += 1
        b.decode().sync()
        witness = jl.Batch().upload(files, fmt).decode().sync()
        for i, f in enumerate(files):
            _check_format(b, i, f, fmt, witness, "%s as format %d, image %d" % (name, fmt, i))
        witness.close()
        outs = [[p.tobytes() for p in _as_list(b.output(i))] for i in range(len(files)) if b.image_info(i).status == 0]
        b.decode().sync()
        assert [[p.tobytes() for p in _as_list(b.output(i))] for i in range(len(files)) if b.image_info(i).status == 0] == outs, "the second decode of " + name
    b.close()


# ------------------------------------------------------------------------------------------------ b. stage calls and the coefficient hand-off

def test_an_entropy_stage_without_its_output_stage_then_another_upload(every_scan_split):
    b = jl.Batch().upload(_progressive_three()).run_entropy()
    b.upload(rc.loud_k2_upload()).run_entropy().sync()
    for i, f in enumerate(rc.loud_k2_upload()):
        _assert_bits(b.coefficients(i), rc.reference(f)[2], "coefficients of image %d behind run_entropy alone" % i)
    b.upload(rc.loud_k2_upload()).decode().sync()
    files = rc.quiet_upload()
    b.upload(files).run_entropy()
    b.upload(files[::-1]).decode().sync()
    _check_u8(b, files[::-1], "decode behind two entropy stages without an output stage")
    b.close()


def _quant_tables(f):
    qt = np.zeros((4, 64), np.uint16)
    for m, a, e in rc.header_segments(f):
        p = f[a + 4:e] if m == 0xDB else b""
        while p:
            n = 128 if p[0] >> 4 else 64
            qt[p[0] & 15] = np.frombuffer(p[1:1 + n], ">u2" if p[0] >> 4 else np.uint8)
            p = p[1 + n:]
    return qt


def _frame(f):
    W, H, _, comps = im.frame(f)
    return {"width": W, "height": H, "precision": 8, "components": comps}


def test_given_coefficients_do_not_outlive_their_upload(every_scan_split):
    """set_coefficients makes the dense copy the output stage's source (dense_override_); the files of the next upload, split scans of
    the same shape in the same places, decode from their own coefficients"""
    from tools import jpegsynth

    a, other, c = rc.mirror_a(), bytes(jpegsynth.encode(112, 80, "420", 75, 4, seed=182)), bytes(jpegsynth.encode(112, 80, "420", 75, 4, seed=183))
    assert rc.table_payloads(a) == rc.table_payloads(other) == rc.table_payloads(c)
    b = jl.Batch().upload([a, rc.mirror_b()]).run_entropy()
    assert sum(b.plan_stats()["idct_split_work"]) > 0
    b.set_coefficients(0, rc.reference(other)[2])
    b.run_idct().sync()
    _assert_bits(b.output(0), rc.reference(other)[1], "the given coefficients")
    _assert_bits(b.output(1), rc.reference(rc.mirror_b())[1], "their neighbour")
    _assert_bits(b.coefficients(0), rc.reference(other)[2], "the given coefficients, read back")
    b.upload([c, rc.mirror_b()]).decode().sync()
    _check_u8(b, [c, rc.mirror_b()], "files behind given coefficients")
    # ... and frames (geometry and tables, no file) between whole files
    frames, qts = [_frame(other), _frame(rc.mirror_b())], np.stack([_quant_tables(other), _quant_tables(rc.mirror_b())])
    for turn in range(2):
        b.upload_frames(frames, qts, jl.FMT_INTERLEAVED_U8)
        b.set_coefficients(0, rc.reference(other)[2])
        b.set_coefficients(1, rc.reference(rc.mirror_b())[2])
        b.run_idct().sync()
        _assert_bits(b.output(0), rc.reference(other)[1], "frame 0, turn %d" % turn)
        _assert_bits(b.output(1), rc.reference(rc.mirror_b())[1], "frame 1, turn %d" % turn)
        b.upload([rc.mirror_b(), a, rc.black_gray()]).decode().sync()
        _check_u8(b, [rc.mirror_b(), a, rc.black_gray()], "files behind frames, turn %d" % turn)
    b.close()


def test_an_upload_of_another_road_and_size_behind_a_decode_that_was_not_waited_for(every_scan_split):
    b = jl.Batch()
    for turn in range(2):
        b.upload(rc.loud_k2_upload()).decode()
        b.upload(_k2s_pair()).decode()
        b.upload(rc.band_upload()).decode()
        b.upload(rc.quiet_upload()).decode().sync()
        _check_u8(b, rc.quiet_upload(), "turn %d" % turn)
    b.upload(_progressive_three()).decode()
    b.upload(rc.loud_k2_upload()).decode().sync()
    _check_u8(b, rc.loud_k2_upload(), "the loud files behind everything")
    b.close()


# ------------------------------------------------------------------------------------------------ c. the ingest kinds by turns

def _paths(st):
    return st["n_header_only"] + st["n_full_walk"]


def test_the_ingest_kinds_by_turns_on_one_batch(every_scan_split):
    ctx = jl.Context(0)
    b = jl.Batch(ctx)
    zero = {k: 0 for k in b.device_ingest_stats()}

    def check(files, what, pinned_dma):
        b.decode().sync()
        _check_u8(b, files, what)
        st = b.ingest_stats()
        assert _paths(st) == len(files) and (st["n_pinned_dma"] > 0) == pinned_dma, (what, st)
        return b.device_ingest_stats()

    files = rc.loud_k2_upload()
    b.upload(files)
    assert check(files, "upload", False) == zero
    files = rc.road_files()
    b.upload_segments([[f[:100], f[100:len(f) // 2], f[len(f) // 2:]] for f in files])
    assert check(files, "upload_segments", False) == zero
    files = rc.quiet_upload() + _k2s_pair()
    arena = ctx.host_alloc(sum(len(f) + 64 for f in files))
    views, pos = [], 0
    for f in files:
        arena[pos:pos + len(f)] = np.frombuffer(f, np.uint8)
        views.append(arena[pos:pos + len(f)])
        pos += (len(f) + 63) // 64 * 64
    b.upload_segments(views, pinned=True)
    assert check(files, "pinned segments", True) == zero
    b.upload_segments(views[::-1][:3], arena=True)
    assert check(files[::-1][:3], "a pinned arena", True) == zero
    files = rc.band_upload() + [rc.black_gray(), rc.loud_k2(0)]
    b.upload_tensors([torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda() for f in files])
    moved = check(files, "upload_tensors", False)
    assert moved["files_gathered"] == len(files) and moved["bytes_gathered"] >= sum(len(f) for f in files), moved
    files = _progressive_three() + [rc.truncated(0)]
    b.upload(files)
    assert check(files, "upload again", False) == zero
    b.close()


# ------------------------------------------------------------------------------------------------ d. the policies: the covering array through ONE batch

def _walk(uploads):
    b = jl.Batch()
    for settings, ks in uploads:
        matrix._upload(settings, matrix._row_images(ks), batch=b)
        matrix._check_uploaded(b, settings, ks)
    b.close()


def test_the_covering_array_through_one_batch_in_array_order():
    """every setter before every upload; each upload checked as test_policy_matrix_gpu.py checks it in a fresh batch"""
    _walk(pm.uploads())


def test_the_covering_array_through_one_batch_in_reverse_order():
    _walk(pm.uploads()[::-1])


# ------------------------------------------------------------------------------------------------ e. settings that are consumed, settings that stay

def _expected(name, fmt=jl.FMT_RGB_U8, orientation=1, window=None, mode="rgb", resize=None, consts=None):
    return pm.expected(pm.file(name), arithmetic="reference", scale=1, upsampling="replicate", color="ycc", mode=mode, orientation=orientation, window=window,
                       fmt=fmt, consts=consts, resize=resize)


def _check_plain(b, names, fmt, what):
    for i, n in enumerate(names):
        want = _expected(n, fmt)
        assert (b.window(i), b.orientation(i)) == (want.window, 1), (what, i, b.window(i), b.orientation(i))
        _assert_bits(b.output(i), want.output, "%s, image %d" % (what, i))


def test_windows_and_orientations_belong_to_one_upload():
    names = ["420", "444"]
    files = [pm.file(n) for n in names]
    b = jl.Batch()
    b.set_windows([(1, 1, 5, 7), (0, 0, 0, 0)]).set_orientations([6, 2])
    b.upload(files, jl.FMT_RGB_U8).decode().sync()
    for i, (n, o, w) in enumerate(zip(names, (6, 2), ((1, 1, 5, 7), None))):
        want = _expected(n, orientation=o, window=w)
        assert (b.window(i), b.orientation(i)) == (want.window, o)
        _assert_bits(b.output(i), want.output, "windowed and turned, image %d" % i)
    b.upload(files, jl.FMT_RGB_U8).decode().sync()
    _check_plain(b, names, jl.FMT_RGB_U8, "the upload behind the windowed one")
    # a list of the wrong length refuses that upload and is gone with it
    for setter, arg in ((b.set_windows, [(0, 0, 4, 4)]), (b.set_orientations, [3]), (b.set_windows, [(0, 0, 4, 4)] * 3)):
        setter(arg)
        with pytest.raises(jl.ArgumentException):
            b.upload(files, jl.FMT_RGB_U8)
        assert len(b) == 0
        b.upload(files, jl.FMT_RGB_U8).decode().sync()
        _check_plain(b, names, jl.FMT_RGB_U8, "the upload behind a refused one")
    # a list in front of upload_frames: consumed and refused, the batch left empty
    frame, qt = _frame(pm.file("444")), _quant_tables(pm.file("444"))[None]
    for setter, arg in ((b.set_windows, [(0, 0, 4, 4)]), (b.set_orientations, [3])):
        setter(arg)
        with pytest.raises(jl.ArgumentException):
            b.upload_frames([frame], qt, jl.FMT_RGB_U8)
        assert len(b) == 0
        b.upload(files[:1], jl.FMT_RGB_U8).decode().sync()
        _check_plain(b, names[:1], jl.FMT_RGB_U8, "a file behind refused frames")
    # a pending list that is withdrawn
    b.set_windows([(0, 0, 4, 4), (0, 0, 4, 4)]).set_orientations([5, 5]).set_windows(None).set_orientations(None)
    b.upload(files, jl.FMT_RGB_U8).decode().sync()
    _check_plain(b, names, jl.FMT_RGB_U8, "behind withdrawn lists")
    b.close()


def test_the_resize_is_withdrawn_and_set_again_smaller():
    names = ["420", "440", "444"]
    b = jl.Batch().set_resize((9, 11), torch.float32)
    b.upload([pm.file(n) for n in names], jl.FMT_RGB_PLANAR_U8).decode().sync()
    got = b.resized()
    assert got.shape == (3, 3, 9, 11) and got.dtype == np.float32
    for i, n in enumerate(names):
        _assert_bits(got[i], _expected(n, jl.FMT_RGB_PLANAR_U8, resize=(9, 11, np.float32)).resized, "resized %s" % n)
    b.set_resize(None)
    with pytest.raises(jl.JpegError):
        b.resized()
    b.upload([pm.file("444")], jl.FMT_RGB_PLANAR_U8).decode().sync()
    with pytest.raises(jl.JpegError):
        b.resized()
    _check_plain(b, ["444"], jl.FMT_RGB_PLANAR_U8, "without a resize")
    b.upload([pm.file("444")], jl.FMT_RGB_U8).decode().sync()  # (a format a set resize would refuse)
    _check_plain(b, ["444"], jl.FMT_RGB_U8, "another format without a resize")
    b.set_resize((3, 4), torch.float16)
    b.upload([pm.file("gray"), pm.file("422")], jl.FMT_RGB_PLANAR_U8).decode().sync()
    got = b.resized()
    assert got.shape == (2, 3, 3, 4) and got.dtype == np.float16
    for i, n in enumerate(("gray", "422")):
        _assert_bits(got[i], _expected(n, jl.FMT_RGB_PLANAR_U8, resize=(3, 4, np.float16)).resized, "resized smaller %s" % n)
    _check_plain(b, ["gray", "422"], jl.FMT_RGB_PLANAR_U8, "beside the smaller resize")
    b.close()


def test_the_partial_flush_setting_stays_and_the_counters_keep_their_scope():
    """include/jpgpu.h: progressive_replays counts for the batch; subseq_rounds is the last decode's (0 = not used); luma_work is the
    upload's.  (The three fallback counters: the next test.)"""
    b = jl.Batch().set_partial_flush(False)
    cut = rc.band_1_5_cut()
    for turn in range(2):  # it holds for the next upload too
        b.upload([cut, rc.band_1_5()]).decode().sync()
        assert NAMES[b.result(0).status] == "InvalidDataException" and b.result(1).status == 0
        _assert_bits(b.output(1), rc.reference(rc.band_1_5())[1], "the clean neighbour, turn %d" % turn)
        assert b.progressive_replays() == 0
    b.set_partial_flush(True)
    # (beside the failing frame, scans handed over as half-line planes: the replay plans the batch again for the failed frame alone, and the
    # coefficients of the images it leaves alone are still read from where, and in the form in which, the first pass left them)
    files = [rc.mirror_a(), cut, rc.band_1_5(), rc.mirror_b(), rc.loud_k2(0)]
    for turn in range(2):
        b.upload(files)
        assert sum(b.plan_stats()["idct_split_work"]) > 0
        b.decode().sync()
        _check_u8(b, files, "partial flush, turn %d" % turn)
        assert b.progressive_replays() == turn + 1  # "issued for this batch so far"
        _check_u8(b, files, "partial flush, turn %d, read again" % turn)
    b.upload(_k2s_pair()).decode().sync()
    assert b.subseq_rounds() > 0 and b.progressive_replays() == 2
    b.upload(rc.loud_k2_upload()).decode().sync()
    assert b.subseq_rounds() == 0  # "the most recent decode (0 = not used)"
    _check_u8(b, rc.loud_k2_upload(), "K2 behind K2S")
    b.set_channels_policy("gray").upload([pm.file("444"), pm.file("420")], jl.FMT_RGB_PLANAR_U8).decode().sync()
    assert sum(b.luma_work()) == 2
    for i, n in enumerate(("444", "420")):
        _assert_bits(b.output(i), _expected(n, jl.FMT_RGB_PLANAR_U8, mode="gray").output, "grey %s" % n)
    b.set_channels_policy("rgb").upload([pm.file("444")], jl.FMT_RGB_PLANAR_U8).decode().sync()
    assert b.luma_work() == (0, 0)
    _check_plain(b, ["444"], jl.FMT_RGB_PLANAR_U8, "three planes again")
    assert (b.progressive_fallbacks(), b.marker_fallbacks(), b.progressive_replays()) == (0, 0, 2)
    b.close()


def test_the_fallback_counters_keep_their_scope_when_the_fallbacks_happen(monkeypatch):
    """include/jpgpu.h: subseq_fallbacks and marker_fallbacks count for the batch, progressive_fallbacks for the upload.  The fallbacks are
    forced the way test_gpu_parity.py forces them: JPGPU_SUBSEQ_BUDGET=2 (read per decode) enqueues fewer rounds than 4:2:0 streams of this
    size need, JPGPU_PROG_SPIN_BUDGET=0 (read per upload) leaves a follower of a long DC scan no poll to spend, JPGPU_K1_SPIN_BUDGET=0 (read
    per decode) makes a marker-index group that would wait count for itself -- whether one had to is the machine's business, so that counter
    is pinned as not reset, whatever it reached.  Every step's bytes are the oracle's."""
    from test_gpu_parity import _pillow_progressive
    from tools import jpegsynth

    k2s = [bytes(jpegsynth.encode(1024, 768, "420", 75, 0, seed=77 + i)) for i in range(3)]
    b = jl.Batch()
    monkeypatch.setenv("JPGPU_SUBSEQ_BUDGET", "2")
    b.upload(k2s).decode().sync()
    _check_u8(b, k2s, "K2S, a budget of two rounds")
    assert b.subseq_fallbacks() == 1 and b.subseq_rounds() > 2, (b.subseq_fallbacks(), b.subseq_rounds())
    monkeypatch.delenv("JPGPU_SUBSEQ_BUDGET")
    fresh = jl.Batch().upload(k2s[::-1]).decode().sync()
    b.upload(k2s[::-1]).decode().sync()
    _check_u8(b, k2s[::-1], "K2S again, the budget unset")
    assert fresh.subseq_fallbacks() == 0 and 2 <= fresh.subseq_rounds() <= 16, (fresh.subseq_fallbacks(), fresh.subseq_rounds())
    assert b.subseq_fallbacks() == 1 and b.subseq_rounds() == fresh.subseq_rounds()  # the batch's count stays, the rounds are this upload's
    fresh.close()
    prog = _progressive_three() + [_pillow_progressive(1024, 768, "4:2:0", 85, 77)]
    monkeypatch.setenv("JPGPU_PROG_SPIN_BUDGET", "0")
    b.upload(prog).decode().sync()
    _check_u8(b, prog, "progressive, no polls to spend")
    assert b.progressive_fallbacks() == 1 and b.subseq_rounds() == 0
    monkeypatch.delenv("JPGPU_PROG_SPIN_BUDGET")
    b.upload(prog[::-1]).decode().sync()
    _check_u8(b, prog[::-1], "progressive again")
    assert b.progressive_fallbacks() == 0 and b.subseq_fallbacks() == 1  # the upload's count starts again, the batch's stays
    monkeypatch.setenv("JPGPU_K1_SPIN_BUDGET", "0")
    b.upload(rc.loud_k2_upload() * 4).decode().sync()
    _check_u8(b, rc.loud_k2_upload() * 4, "the marker index without patience")
    gave_up = b.marker_fallbacks()
    assert 0 <= gave_up <= 1
    monkeypatch.delenv("JPGPU_K1_SPIN_BUDGET")
    b.upload(rc.quiet_upload()).decode().sync()
    _check_u8(b, rc.quiet_upload(), "behind it")
    assert (b.marker_fallbacks(), b.subseq_fallbacks(), b.progressive_fallbacks(), b.progressive_replays()) == (gave_up, 1, 0, 0)
    b.close()


# ------------------------------------------------------------------------------------------------ f. two batches on one context

def test_two_batches_on_one_context_interleaved_without_syncs(every_scan_split):
    ctx = jl.Context(0)
    a, b = jl.Batch(ctx), jl.Batch(ctx)
    a.upload(rc.loud_k2_upload())
    b.upload(_progressive_three() * 2)
    a.decode()
    b.decode()
    files_a = rc.quiet_upload() * 2
    a.upload(files_a)  # (b's decode has not been waited for)
    files_b = _k2s_pair() * 3
    b.upload(files_b)
    a.decode()
    b.decode()
    a.sync()
    b.sync()
    _check_u8(a, files_a, "batch A")
    _check_u8(b, files_b, "batch B")
    _road(b, "k2s", len(files_b))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ the JpegDecoder mirror

def _mirror_decode(d, data):
    d.SetInput(data)
    d.Identify()
    n = d.NumberOfComponents
    out = np.zeros((d.Height, d.Width, n), np.uint8)
    d.SetOutputWriter(jl.JpegBufferOutputWriter8Bit(d.Width, d.Height, n, out.reshape(-1)))
    return out


def test_one_decoder_for_many_inputs_keeps_its_tables_as_the_reference_does():
    """The reference's SetInput clears the frame header and the restart interval (JpegDecoder.cs:56-62), not _huffmanTables /
    _quantizationTables: an abbreviated file decodes with the tables the file before it defined.  Behind ResetTables() (:960-965) the
    scan decoder finds none -- GetHuffmanTable returns null (:869-885) -- and ProcessScan throws InvalidDataException, "Huffman table of
    component 0 is not defined." (JpegHuffmanBaselineScanDecoder.cs:70-76).  Decode() without a writer: InvalidOperationException, "The
    output buffer is not specified." (JpegDecoder.cs:515-518).  Every input has a writer of its own size."""
    a, bfile = rc.mirror_a(), rc.mirror_b()
    short = rc.without_tables(bfile)
    d = jl.JpegDecoder()
    out = _mirror_decode(d, a)
    d.Decode()
    first = out.copy()
    _assert_bits(first, rc.reference(a)[1], "A")
    out = _mirror_decode(d, short)  # (a smaller writer than A's)
    d.Decode()
    _assert_bits(out, rc.reference(bfile)[1], "the abbreviated B with A's tables")
    d.ResetTables()
    out = _mirror_decode(d, short)
    with pytest.raises(jl.InvalidDataException, match="Huffman table of component 0 is not defined"):
        d.Decode()
    assert not out.any()
    out = _mirror_decode(d, rc.loud_progressive(0))
    d.Decode()
    _assert_bits(out, rc.reference(rc.loud_progressive(0))[1], "a progressive file")
    cut = rc.truncated(4)
    out = _mirror_decode(d, cut)  # (a larger writer)
    with pytest.raises(jl.InvalidDataException):
        d.Decode()
    _assert_bits(out, rc.reference(cut)[1], "what the failing decode left in the writer")
    out = _mirror_decode(d, rc.black_gray())
    out[:] = 0xA5
    d.Decode()
    assert not out.any()
    out = _mirror_decode(d, a)
    d.Decode()
    _assert_bits(out, first, "A again")
    d.ResetOutputWriter()
    with pytest.raises(jl.InvalidOperationException, match="The output buffer is not specified"):
        d.Decode()
    d.close()
