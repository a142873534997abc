"""jpgpu_batch_upload_device / Batch.upload_tensors: JPEG files that already lie in device memory are gathered into the batch on the
device; the host sees their heads (and, whole, the files that need the full marker walks); everything behind the upload behaves as
it does behind a host upload of the same bytes.

Every case is checked against the oracle's Identify + Decode on the same bytes (statuses by exception class, as test_ingest_gpu.py
does) and, where it says so, against the host upload; Batch.device_ingest_stats() says what crossed the host link."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from golden_util import read_jpeg
from jpeglibrary_amd import _capi
from oracle import pyoracle as po
from tools import jpegsynth

pytestmark = pytest.mark.gpu

NAMES = {0: "OK", 1: "InvalidDataException", 2: "InvalidOperationException", 3: "NotSupportedException", 4: "ArgumentException"}
U8, PLANAR = jl.FMT_INTERLEAVED_U8, jl.FMT_RGB_PLANAR_U8
HEAD_MAX = 64 << 10
JUNK = b"\xff\xd9\xff\xda\xff\x00\xff\xd0\xff\xff\x00"  # marker look-alikes for the gaps between files (the pinned-arena test's)
_lib = _capi.lib
_ORACLE = {}


def _oracle(data, fmt=U8):
    """(exception class or "OK", samples or None) of the checker for these bytes: computed once per file and format, never changed"""
    key = (bytes(data), fmt)
    if key not in _ORACLE:
        try:
            ref = po.decode_8bit(bytes(data))[0]
            if fmt == PLANAR:
                ref = np.ascontiguousarray(po.ycbcr8_to_rgb(ref, gray=ref.shape[2] == 1).transpose(2, 0, 1))
            ref.setflags(write=False)
            _ORACLE[key] = ("OK", ref)
        except po.OracleError as e:
            _ORACLE[key] = (e.kind, None)
    return _ORACLE[key]


def _dev(data):
    """the file's bytes as a 1-D uint8 tensor on the device"""
    if len(data) == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda:0")
    return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to("cuda:0")


def _check(b, files, fmt=U8, host=None):
    """every image of decoded batch `b` against the oracle (and the statuses of `host`, a host upload of the same files)"""
    problems = []
    for i, f in enumerate(files):
        kind, ref = _oracle(f, fmt)
        res = b.result(i)
        mine = NAMES.get(res.status, str(res.status))
        if mine != kind:
            problems.append((i, kind, mine, res.detail))
        elif ref is not None and not np.array_equal(b.output(i), ref):
            problems.append((i, "samples differ"))
        if host is not None:
            h = host.result(i)
            if (h.status, h.detail) != (res.status, res.detail):
                problems.append((i, "host upload says", h.status, h.detail, "device upload", res.status, res.detail))
    assert not problems, problems


def _good():
    return bytes(jpegsynth.encode(160, 96, "420", 75, 2, seed=42))


def _variety():
    """test_ingest_gpu.py's _variety(), restated: files of every ingest kind -- header-only plans, full walks (progressive, several
    scans, garbage behind the scan, bytes behind EOI), failures, and one whose first scan starts behind the 64 KiB head"""
    good = _good()
    sos = good.index(b"\xff\xda")
    app = b"\xff\xe1" + (65000).to_bytes(2, "big") + bytes(64998)
    big_head = good[:2] + app + app + good[2:]
    return [
        good,
        bytes(jpegsynth.encode(512, 512, "444", 75, 0, seed=3)),
        bytes(jpegsynth.encode(331, 177, "422", 80, 3, seed=9)),
        good + bytes(range(1, 200)),                                     # bytes behind EOI
        good[:-2] + b"\x5a\xff\xd9\xff\xfe\x00\x04ab",                  # one unread byte in front of the terminator + a segment behind EOI
        good[:-2] + b"\xff\xfe\x00\x04ab\xff\xd9",                      # COM behind the scan: full walk
        good[:sos + 14 + 200],                                           # truncated in the scan
        read_jpeg("progress.jpg"),
        read_jpeg("yellowcat_progressive_restart.jpg"),
        read_jpeg("lake.jpg"),
        bytes(jpegsynth.encode(96, 64, "444", 75, 0, seed=5, noninterleaved=True)),
        big_head,
        b"\xff\xd8",
        b"",
    ]


def _entropy_offset(data):
    """offset of the first entropy-coded byte: behind the first SOS header, found by walking the marker segments"""
    pos = 2
    while True:
        assert data[pos] == 0xFF
        seg = int.from_bytes(data[pos + 2:pos + 4], "big")
        if data[pos + 1] == 0xDA:
            return pos + 2 + seg
        pos += 2 + seg


# ------------------------------------------------------------------------------------------------ every ingest kind

@pytest.mark.parametrize("fmt", [U8, PLANAR], ids=["interleaved", "rgb_planar"])
def test_every_ingest_kind_from_device_memory(fmt):
    files = _variety()
    host = jl.Batch().upload(files, fmt).decode().sync()
    b = jl.Batch().upload_tensors([_dev(f) for f in files], fmt).decode().sync()
    _check(b, files, fmt, host)
    st, dst = b.ingest_stats(), b.device_ingest_stats()
    assert st["n_pinned_dma"] == 0 and st["n_linearised"] == 0 and st["total_ms"] > 0, st
    # header-only: the three clean files, lake.jpg, and big_head once it has been fetched whole; full walks: the two files with bytes behind EOI
    # (a head is all the host holds of them: the EOI has to close the file), COM behind the scan, the truncated file, the two progressive files,
    # several scans; FF D8 and the empty file fail in front of either
    assert st["n_header_only"] == 5 and st["n_full_walk"] == 7, st
    assert dst["files_gathered"] == sum(1 for f in files if f) and dst["bytes_gathered"] == sum(len(f) for f in files), dst
    assert dst["files_downloaded"] == 8, (st, dst)  # (the seven full walks, and big_head for its header-only plan)
    # (big_head, whose first scan starts behind the 64 KiB a head may have, is one of the two; the heads' total is the same on every upload of the list)
    assert dst["walker_giveups"] == 2 and dst["head_bytes"] == 72416, dst
    assert host.device_ingest_stats() == dict.fromkeys(dst, 0)  # a host upload moved nothing this way
    host.close()
    b.close()


# ------------------------------------------------------------------------------------------------ alignment and tails

def _laid_out(files, starts):
    """one device tensor that holds the files at start offsets with the residues `starts` (mod 16), marker look-alikes everywhere else;
    returns it and the files' views"""
    places, pos = [], 64
    for f, r in zip(files, starts):
        pos += (r - pos) % 16
        places.append(pos)
        pos += len(f) + 23
    host = np.frombuffer(JUNK * (pos // len(JUNK) + 2), np.uint8)[:pos + 64].copy()
    for f, at in zip(files, places):
        host[at:at + len(f)] = np.frombuffer(f, np.uint8)
    big = torch.from_numpy(host).to("cuda:0")
    assert big.data_ptr() % 256 == 0
    return big, [big[at:at + len(f)] for f, at in zip(files, places)]


def test_any_alignment_and_any_tail_length():
    good = _good()
    tails = [good + bytes([0x30 + k] * k) for k in range(16)]  # 0..15 bytes behind EOI: lengths of all 16 residues mod 16
    files = tails + _variety()
    assert {len(f) % 16 for f in files} == set(range(16))
    starts = [(5 * k + 3) % 16 for k in range(len(files))]
    assert set(starts) == set(range(16))
    big, views = _laid_out(files, starts)
    assert {v.data_ptr() % 16 for v in views if v.numel()} == set(range(16))
    b = jl.Batch().upload_tensors(views, U8).decode().sync()
    _check(b, files)
    # the other residues for the same lengths
    big2, views2 = _laid_out(files, [(s + 7) % 16 for s in starts])
    b.upload_tensors(views2, U8).decode().sync()
    _check(b, files)
    # the same tensor listed three times, beside an overlapping view of it (a file cut short)
    i = 16 + 9  # lake.jpg: several gather pieces from an address that is no multiple of 16
    assert views2[i].data_ptr() % 16 != 0 and len(files[i]) > 3 * (64 << 10)
    cut = views2[i][:len(files[i]) // 2]
    b.upload_tensors([views2[i], views2[i], cut, views2[i]], PLANAR).decode().sync()
    _check(b, [files[i], files[i], files[i][:len(files[i]) // 2], files[i]], PLANAR)
    assert b.device_ingest_stats()["files_gathered"] == 4
    b.close()
    del big, big2


# ------------------------------------------------------------------------------------------------ the verdict bytes

def test_what_follows_the_scan_is_judged_from_the_bytes_the_device_delivers():
    good = _good()
    body = good[:-2]
    sos = good.index(b"\xff\xda")
    rsts = [i for i in range(sos + 14, len(good) - 1) if good[i] == 0xFF and 0xD0 <= good[i + 1] <= 0xD7]
    cases = {  # name: (bytes, a header-only plan whose EOI closes the file)
        "clean": (good, True),
        "second_eoi": (good + b"\xff\xd9", False),
        "early_eoi_at_restart": (good[:rsts[10]] + b"\xff\xd9", True),
        "no_eoi": (body, False),
        "zeros_for_eoi": (body + bytes(2), False),
        "com_behind_scan": (body + b"\xff\xfe\x00\x04ab\xff\xd9", False),
        "dri_behind_scan": (body + b"\xff\xdd\x00\x04\x00\x07\xff\xd9", False),
        "truncated_in_scan": (good[:sos + 14 + 200], False),
        "no_scan_at_all": (good[:sos] + b"\xff\xd9", False),
        "not_a_jpeg": (bytes(range(256)) * 4, False),
    }
    b = jl.Batch()
    for name, (data, header_only) in cases.items():
        b.upload_tensors([_dev(data)], U8).decode().sync()
        _check(b, [data])
        st, dst = b.ingest_stats(), b.device_ingest_stats()
        if header_only:
            assert st["n_header_only"] == 1 and dst["files_downloaded"] == 0, (name, st, dst)
        else:
            assert st["n_header_only"] == 0, (name, st, dst)
    files = [c[0] for c in cases.values()]
    b.upload_tensors([_dev(f) for f in files], U8).decode().sync()
    _check(b, files)
    assert b.ingest_stats()["n_header_only"] == sum(1 for c in cases.values() if c[1])
    b.close()


# ------------------------------------------------------------------------------------------------ only heads cross the link

def test_only_the_heads_of_clean_files_cross_the_host_link():
    files = [bytes(jpegsynth.encode(w, h, ss, q, dri, seed=w + h)) for (w, h, ss, q, dri) in
             [(512, 512, "444", 75, 0), (640, 368, "420", 75, 4), (331, 177, "422", 80, 3), (100, 75, "gray", 60, 1), (17, 9, "420", 75, 1)]]
    files += [read_jpeg("cramps.jpg"), read_jpeg("lake.jpg")]
    b = jl.Batch().upload_tensors([_dev(f) for f in files], U8).decode().sync()
    _check(b, files)
    st, dst = b.ingest_stats(), b.device_ingest_stats()
    assert st["n_header_only"] == len(files) and st["n_full_walk"] == 0, st
    assert dst["files_downloaded"] == 0 and dst["bytes_downloaded"] == 0 and dst["walker_giveups"] == 0, dst
    assert 0 < dst["head_bytes"] <= sum(_entropy_offset(f) + 256 for f in files), dst
    large = [f for f in files if len(f) > _entropy_offset(f) + 256]
    assert len(large) >= 5
    b.upload_tensors([_dev(f) for f in large], U8)
    dst = b.device_ingest_stats()
    assert dst["head_bytes"] < sum(min(len(f), HEAD_MAX) for f in large) and dst["files_downloaded"] == 0, dst

    good = _good()
    # one 20 000-byte APP1 in front of the tables: still planned from its head, which covers the APP1
    app1 = good[:2] + b"\xff\xe1" + (20000).to_bytes(2, "big") + bytes(19998) + good[2:]
    b.upload_tensors([_dev(app1)], U8).decode().sync()
    _check(b, [app1])
    st, dst = b.ingest_stats(), b.device_ingest_stats()
    assert st["n_header_only"] == 1 and dst["files_downloaded"] == 0 and dst["walker_giveups"] == 0, (st, dst)
    assert 20000 < _entropy_offset(app1) <= dst["head_bytes"] <= _entropy_offset(app1) + 256, dst

    # a fill byte in front of a header marker: the walker gives up (its head is min(len, 64 KiB)); planned and decoded all the same
    dqt = good.index(b"\xff\xdb")
    fill = good[:dqt] + b"\xff" + good[dqt:]
    host = jl.Batch().upload([fill], U8).decode().sync()
    b.upload_tensors([_dev(fill)], U8).decode().sync()
    _check(b, [fill], U8, host)
    host.close()
    dst = b.device_ingest_stats()
    assert dst["walker_giveups"] == 1 and dst["head_bytes"] == (min(len(fill), HEAD_MAX) + 15) // 16 * 16, dst

    # the first scan starts behind the 64 KiB head: downloaded whole, and decodes
    big_head = _variety()[11]
    assert _entropy_offset(big_head) > 2 * 65000
    b.upload_tensors([_dev(big_head)], U8).decode().sync()
    _check(b, [big_head])
    assert _oracle(big_head)[0] == "OK"
    dst = b.device_ingest_stats()
    assert dst["files_downloaded"] == 1 and dst["bytes_downloaded"] == len(big_head), dst
    b.close()


# ------------------------------------------------------------------------------------------------ the copy contract

def test_the_batch_owns_a_copy_when_the_upload_returns():
    files = _variety()
    tensors = [_dev(f) for f in files]
    b = jl.Batch().upload_tensors(tensors, U8)
    for t in tensors:
        t.fill_(0xFF)
    torch.cuda.synchronize()
    b.decode().sync()
    _check(b, files)
    del tensors
    # ... and an upload right after an unsynchronised decode waits for it (test_ingest_gpu.py's, from device memory)
    mk = lambda seed0: [bytes(jpegsynth.encode(640, 368, "420", 90, 4, seed=seed0 + i)) for i in range(6)]
    fa, fb = mk(820), mk(840)
    ta, tb = [_dev(f) for f in fa], [_dev(f) for f in fb]
    b.upload_tensors(ta, U8)
    for _ in range(6):
        b.decode()          # not waited for
        b.upload_tensors(tb, U8)
        b.decode()          # not waited for either
        b.upload_tensors(ta, U8)
    b.decode().sync()
    _check(b, fa)
    b.decode()
    b.upload_tensors(tb, U8)
    b.decode().sync()
    _check(b, fb)
    b.close()


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


def test_refusals_are_decided_before_anything_runs_and_leave_the_batch_empty():
    ctx = jl.Context(0)
    good = _good()
    t = _dev(good)
    b = jl.Batch(ctx)

    def upload(ptr, length, fmt=U8):
        rc = _lib.jpgpu_batch_upload_device(b._h, (C.c_void_p * 1)(ptr), (C.c_size_t * 1)(length), 1, fmt)
        return rc, _lib.jpgpu_last_error(ctx._h)

    def refused(ptr, length, fmt=U8, why=b""):
        b.upload_tensors([t], U8)  # a batch that holds something: the refusal empties it
        assert len(b) == 1
        rc, msg = upload(ptr, length, fmt)
        assert rc == _capi.ERR_ARGUMENT and why in msg, (rc, msg)
        assert len(b) == 0
        assert not any(b.device_ingest_stats().values())  # (what the refused upload's predecessor moved is forgotten with it)
        b.upload_tensors([t], U8).decode().sync()  # ... and it still decodes a good upload
        _check(b, [good])

    pageable = np.frombuffer(good, np.uint8).copy()
    refused(pageable.ctypes.data, pageable.size, why=b"not in device memory")
    pinned = ctx.host_alloc(len(good))
    pinned[:] = pageable
    refused(pinned.ctypes.data, pinned.size, why=b"not in device memory")
    ctx.host_free(pinned)
    # a 100-byte tensor that is an allocation of its own, passed as 1 MiB
    base = C.c_void_p()
    assert _hip("hipMalloc", C.POINTER(C.c_void_p), C.c_size_t)(C.byref(base), 100) == 0
    try:
        small = torch.as_tensor(jl.batch._DeviceView(None, base.value, (100,)), device="cuda:0")
        assert small.numel() == 100 and small.data_ptr() == base.value
        refused(small.data_ptr(), 1 << 20, why=b"inside one device allocation")
        del small
    finally:
        assert _hip("hipFree", C.c_void_p)(base) == 0
    refused(None, 5, why=b"null pointer")
    refused(t.data_ptr(), t.numel(), fmt=99, why=b"unknown format")
    refused(t.data_ptr(), t.numel(), fmt=-1, why=b"unknown format")
    # NULL arrays, a NULL batch
    assert _lib.jpgpu_batch_upload_device(b._h, None, (C.c_size_t * 1)(5), 1, U8) == _capi.ERR_ARGUMENT and len(b) == 0
    assert _lib.jpgpu_batch_upload_device(b._h, (C.c_void_p * 1)(t.data_ptr()), None, 1, U8) == _capi.ERR_ARGUMENT
    assert _lib.jpgpu_batch_upload_device(None, (C.c_void_p * 1)(t.data_ptr()), (C.c_size_t * 1)(5), 1, U8) == _capi.ERR_ARGUMENT
    # a NULL pointer with length 0 is the empty file: accepted, with the host path's per-image status
    rc = _lib.jpgpu_batch_upload_device(b._h, (C.c_void_p * 2)(None, t.data_ptr()), (C.c_size_t * 2)(0, t.numel()), 2, U8)
    assert rc == 0 and len(b) == 2, _lib.jpgpu_last_error(ctx._h)
    b.decode().sync()
    _check(b, [b"", good])
    b.close()
    # the Python entry refuses a mixed list, and what it would have to copy
    with pytest.raises(ValueError, match="mix"):
        jl.decode_batch([good, t])
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        jl.Batch(ctx).upload_tensors([t[::2]])
    ctx.close()


# ------------------------------------------------------------------------------------------------ the loop

def test_encode_tensors_to_decode_to_tensors_without_a_download():
    rng = np.random.default_rng(11)
    imgs = [torch.from_numpy(rng.integers(0, 256, (3, 48, 64), dtype=np.uint8)).to("cuda:0"),
            torch.from_numpy(rng.integers(0, 256, (3, 17, 33), dtype=np.uint8)).to("cuda:0")]
    # 4:2:0 with restart_interval = 2 and 4:4:4 without: two batches (a batch has one sampling), each with both images
    for luma, dri in (((2, 2), 2), ((1, 1), 0)):
        files = jl.encode_tensors(imgs, luma, 80, rgb=True, restart_interval=dri)  # the streams as bytes, downloaded
        eb = jl.EncodeBatch().upload_tensors(imgs, luma, 80, rgb=True, restart_interval=dri).encode()
        streams = [eb.output_tensor(i) for i in range(len(eb))]  # the same streams where they are, in HBM
        assert all(t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1 for t in streams)
        assert [bytes(t.cpu().numpy()) for t in streams] == files
        tensors, results = jl.decode_to_tensors(streams)  # from the encoder's buffer into the decoder's, on the device
        via_host, _ = jl.decode_to_tensors(files)
        for i, (img, data) in enumerate(zip(imgs, files)):
            kind, ref = _oracle(data, PLANAR)
            assert kind == "OK" and results[i].status == 0 and tensors[i].shape == img.shape, (luma, i)
            assert np.array_equal(tensors[i].cpu().numpy(), ref), (luma, i)
            assert torch.equal(tensors[i], via_host[i]), (luma, i)
        outs, results = jl.decode_batch(streams, U8)  # decode_batch takes them too
        for i, data in enumerate(files):
            assert results[i].status == 0 and np.array_equal(outs[i], _oracle(data, U8)[1]), (luma, i)
        eb.close()
