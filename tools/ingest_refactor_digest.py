#!/usr/bin/env python3
"""tools/ingest_refactor_digest.py -- everything a caller can see of jpgpu_batch_upload*, one line per upload: what the ingest's
refactor into stages (device_batch_ingest.cpp) was checked with, and what any later change to the ingest can be checked with.

    python tools/ingest_refactor_digest.py --root TREE --raw raw.txt --digest digest.txt

TREE is the checkout whose built jpeglibrary_amd is exercised (default: this one); the files, jpegsynth and the golden images are
this checkout's either way.  Run it on two builds on one machine: the raw logs are to be identical byte for byte.  Each raw line
is `label | ...`: per image the status, detail and error text of result(i), the fields of image_info(i) (out_offset relative to
image 0's) and the sha256 of output(i) where the image decoded; the integer fields of ingest_stats() and device_ingest_stats()
(no milliseconds); for a refused upload the status, the message and the batch's size afterwards.  The digest file holds
`label | sha256[:16] of the raw line`.

The cases: the files of every ingest kind (tests/test_ingest_gpu.py's _variety) through every source -- contiguous, cut into
segments three ways, page-locked segments, two page-locked segments per file, one arena with marker look-alikes in the gaps, the
arena with repeated views, a registered caller array, device tensors, device tensors at every start residue mod 16 -- in
INTERLEAVED_U8 and RGB_PLANAR_U8, at JPGPU_HOST_THREADS 1, 3 and unset; a 3 x 1 MiB staging ring that wraps; the one-unread-byte
files with the re-plan of a middle scan and a second upload behind it; failing progressive files with the replay; optimize_batch
over DRI > 0 and DRI = 0 files; n = 0; an upload right behind an unsynchronised decode; every refusal of upload_segments and
upload_device."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK = b"\xff\xd9\xff\xda\xff\x00\xff\xd0\xff\xff\x00"
LINES = []


def sha(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def emit(label, text):
    LINES.append("%s | %s" % (label, text))


def variety(jpegsynth, read_jpeg):
    good = bytes(jpegsynth.encode(160, 96, "420", 75, 2, seed=42))
    sos = good.index(b"\xff\xda")
    app = b"\xff\xe1" + (65000).to_bytes(2, "big") + bytes(64998)
    return [good, bytes(jpegsynth.encode(512, 512, "444", 75, 0, seed=3)), bytes(jpegsynth.encode(331, 177, "422", 80, 3, seed=9)),
            good + bytes(range(1, 200)), good[:-2] + b"\x5a\xff\xd9\xff\xfe\x00\x04ab", good[:-2] + b"\xff\xfe\x00\x04ab\xff\xd9",
            good[:sos + 14 + 200], read_jpeg("progress.jpg"), read_jpeg("yellowcat_progressive_restart.jpg"), read_jpeg("lake.jpg"),
            bytes(jpegsynth.encode(96, 64, "444", 75, 0, seed=5, noninterleaved=True)), good[:2] + app + app + good[2:], b"\xff\xd8", b""]


def split(data, cuts):
    cuts = sorted({c for c in cuts if 0 < c < len(data)})
    parts, prev = [], 0
    for c in cuts + [len(data)]:
        parts.append(bytes(data[prev:c]))
        prev = c
    return parts


def laid_out(torch, files, starts):
    places, pos = [], 64
    for f, r in zip(files, starts):
        pos += (r - pos) % 16
        places.append(pos)
        pos += len(f) + 23
    host = np.frombuffer(JUNK * (pos // len(JUNK) + 2), np.uint8)[:pos + 64].copy()
    for f, at in zip(files, places):
        host[at:at + len(f)] = np.frombuffer(f, np.uint8)
    big = torch.from_numpy(host).to("cuda:0")
    return big, [big[at:at + len(f)] for f, at in zip(files, places)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--raw", required=True)
    ap.add_argument("--digest", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import jpeglibrary_amd as jl
    from jpeglibrary_amd import _capi
    sys.path.remove(os.path.abspath(args.root))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    from golden_util import middle_scan_swallow_files, read_jpeg
    from tools import jpegsynth

    lib = _capi.lib
    U8, PLANAR = jl.FMT_INTERLEAVED_U8, jl.FMT_RGB_PLANAR_U8

    def last_error(ctx):
        return (lib.jpgpu_last_error(ctx._h) or b"").decode("latin-1")

    def stats(b):
        st, dst = b.ingest_stats(), b.device_ingest_stats()
        return " ".join("%s=%d" % kv for kv in list(st.items()) + list(dst.items()) if not kv[0].endswith("_ms"))

    def describe(b, label, decode=True, partial=()):
        """one line for the upload batch `b` holds; partial: images whose output is hashed although they failed (the replay's)"""
        if decode:
            b.decode().sync()
        out, first = [], None
        for i in range(len(b)):
            info = b.image_info(i)
            first = info.out_offset if first is None else first
            res = b.result(i)
            err = last_error(b.ctx) if res.status != 0 else ""
            fields = [getattr(info, k) for k, _ in _capi.ImageInfo._fields_ if k not in ("out_offset", "plane", "reserved")]
            planes = [(p.offset, p.width, p.height, p.pitch) for p in info.plane]
            pix = "-"
            if decode and info.status == 0 and (res.status == 0 or i in partial):
                o = b.output(i)
                pix = sha(np.ascontiguousarray(o).tobytes()) if not isinstance(o, list) else sha(b"".join(np.ascontiguousarray(p).tobytes() for p in o))
            out.append("[%d: %d %d %r info=%s planes=%s rel=%d out=%s]" % (i, res.status, res.detail, err, fields, planes, info.out_offset - first, pix))
        emit(label, "n=%d %s %s replays=%d" % (len(b), stats(b), " ".join(out), b.progressive_replays()))

    files = variety(jpegsynth, read_jpeg)
    tails = [files[0] + bytes([0x30 + k] * k) for k in range(16)]
    ctx = jl.Context(0)

    def every_source(tag, fmt):
        b = jl.Batch(ctx)
        describe(b.upload(files, fmt), tag + " contiguous")
        for name, cutter in (("16k", lambda d: list(range(16384, len(d), 16384))),
                             ("awkward", lambda d: [1, 2, 3, 4, 20, 21, len(d) // 3, len(d) // 3 + 1, len(d) - 2, len(d) - 1]),
                             ("whole", lambda d: [])):
            segs = [split(f, cutter(f)) for f in files]
            segs[1] = segs[1][:1] + [b""] + segs[1][1:]
            describe(b.upload_segments(segs, fmt), tag + " segments " + name)
        arena = ctx.host_alloc(sum(len(f) for f in files) + 64 * len(files))
        arena[:] = np.frombuffer(JUNK * (arena.size // len(JUNK) + 1), np.uint8)[:arena.size]
        views, pos = [], 0
        for f in files:
            arena[pos:pos + len(f)] = np.frombuffer(f, np.uint8)
            views.append(arena[pos:pos + len(f)])
            pos += (len(f) + 63) // 64 * 64
        describe(b.upload_segments(views, fmt, pinned=True), tag + " pinned segments")
        describe(b.upload_segments([[v[:len(v) // 2], v[len(v) // 2:]] if len(v) > 4 else [v] for v in views], fmt, pinned=True), tag + " pinned two segments per file")
        describe(b.upload_segments(views, fmt, arena=True), tag + " arena with junk in the gaps")
        describe(b.upload_segments([views[1], views[9], views[1], views[1], views[9]], fmt, arena=True), tag + " arena repeated views")
        mine = np.frombuffer(bytearray(files[1]), np.uint8)
        ctx.host_register(mine)
        describe(b.upload_segments([mine], fmt, pinned=True), tag + " registered caller array")
        ctx.host_unregister(mine)
        tensors = [torch.from_numpy(np.frombuffer(f, np.uint8).copy()).to("cuda:0") if f else torch.empty(0, dtype=torch.uint8, device="cuda:0") for f in files]
        describe(b.upload_tensors(tensors, fmt), tag + " device tensors")
        starts = [(5 * k + 3) % 16 for k in range(len(tails + files))]
        for shift in (0, 7):
            big, dviews = laid_out(torch, tails + files, [(s + shift) % 16 for s in starts])
            describe(b.upload_tensors(dviews, fmt), tag + " device tensors at residues +%d" % shift)
            del big, dviews
        b.close()
        ctx.host_free(arena)

    def with_threads(fn):
        for threads in ("1", "3", None):
            if threads is None:
                os.environ.pop("JPGPU_HOST_THREADS", None)
            else:
                os.environ["JPGPU_HOST_THREADS"] = threads
            fn("threads=%s" % (threads or "unset"))
        os.environ.pop("JPGPU_HOST_THREADS", None)

    with_threads(lambda tag: [every_source("%s fmt=%d" % (tag, fmt), fmt) for fmt in (U8, PLANAR)])

    # a small staging ring that wraps: 3 slots of 1 MiB under some 6 MB of small files
    small = [bytes(jpegsynth.encode(640, 480, "444", 92, k % 3, seed=500 + k)) for k in range(40)]
    os.environ["JPGPU_STAGING_SLOTS"], os.environ["JPGPU_STAGING_SLOT_MB"] = "3", "1"
    ring_ctx = jl.Context(0)
    del os.environ["JPGPU_STAGING_SLOTS"], os.environ["JPGPU_STAGING_SLOT_MB"]

    def ring(tag):
        b = jl.Batch(ring_ctx)
        describe(b.upload(small, U8), "%s small ring, %d bytes" % (tag, sum(len(f) for f in small)))
        describe(b.upload_segments([split(f, [len(f) // 2]) for f in small], PLANAR), tag + " small ring, two segments per file")
        b.close()
    with_threads(ring)
    ring_ctx.close()

    # one unread byte in front of the terminator: the header-only path's direct verdict; a middle scan's re-plan; an upload behind it
    good = bytes(jpegsynth.encode(104, 72, "420", 80, 4, seed=91))
    unread = []
    for k in (1, 2, 3):
        for tail in (b"\xff\xd9", b"\xff\xd9\xff\xd9", b"\xff\xd9\xff\xfe\x00\x04ab", b"\xff\xd9\xff\xfe\x00\x09ab"):
            unread.append(good[:-2] + bytes([0x5A] * k) + tail)
    b = jl.Batch(ctx)
    describe(b.upload(unread, U8), "one unread byte, header-only")
    middle = [bytes(f) for f in middle_scan_swallow_files()[0]]
    describe(b.upload(middle, U8), "one unread byte in a middle scan (re-plan)")
    describe(b.upload(unread[:3] + files[:3], PLANAR), "the upload behind the re-plan")
    tensors = [torch.from_numpy(np.frombuffer(f, np.uint8).copy()).to("cuda:0") for f in middle]
    describe(b.upload_tensors(tensors, U8), "one unread byte in a middle scan, device tensors")

    # failing progressive files: result() and the replay (a flipped bit in one scan's entropy-coded data, a restart marker out of turn)
    bad = [files[7], files[0]]
    for name in ("progress.jpg", "yellowcat_progressive_restart.jpg"):
        clean = read_jpeg(name)
        sos = [k for k in range(len(clean) - 1) if clean[k] == 0xFF and clean[k + 1] == 0xDA]
        for k in range(8):
            d = bytearray(clean)
            first = sos[k % len(sos)]
            end = sos[k % len(sos) + 1] if k % len(sos) + 1 < len(sos) else len(d) - 2
            at = first + 16 + (end - first - 16) * (k + 1) // 10
            if d[at] != 0xFF and d[at - 1] != 0xFF:
                d[at] ^= 0x10 << (k % 3)
            bad.append(bytes(d))
        rst = [k for k in range(sos[0], len(clean) - 1) if clean[k] == 0xFF and 0xD0 <= clean[k + 1] <= 0xD7]
        if rst:
            d = bytearray(clean)
            d[rst[len(rst) // 2] + 1] = 0xD0 + (d[rst[len(rst) // 2] + 1] - 0xD0 + 3) % 8
            bad.append(bytes(d))
    everything = tuple(range(len(bad)))
    describe(b.upload(bad, U8), "failing progressive files", partial=everything)
    describe(b.upload_tensors([torch.from_numpy(np.frombuffer(f, np.uint8).copy()).to("cuda:0") for f in bad], PLANAR), "failing progressive files, device tensors", partial=everything)
    describe(b.upload(files[:3], U8), "the upload behind the replay")

    # n = 0, and an upload right behind an unsynchronised decode
    describe(b.upload([], U8), "n=0 upload")
    describe(b.upload_segments([], U8), "n=0 upload_segments")
    describe(b.upload_tensors([], U8), "n=0 upload_tensors")
    for _ in range(3):
        b.upload(files[:4], U8).decode()
        b.upload(files[4:12], U8).decode()
    describe(b.upload(files[:4], U8), "upload behind an unsynchronised decode")
    b.close()

    # the optimizer's walk through upload_files (entropy-only plans)
    opt_files = [bytes(jpegsynth.encode(640, 368, "420", 75, 7, seed=3)), bytes(jpegsynth.encode(331, 177, "422", 80, 3, seed=9)), bytes(jpegsynth.encode(300, 180, "444", 80, 0, seed=9)), files[0], files[1], files[6], b""]
    for strip in (True, False):
        ob = jl.optimizer.OptimizeBatch(ctx).upload(opt_files, strip=strip).run()
        rows = []
        for i in range(len(opt_files)):
            res, size = ob.result(i)
            rows.append("[%d: %d %d %d %s]" % (i, res.status, res.detail, size, sha(ob.output(i)) if res.status == 0 else repr(last_error(ctx))))
        emit("optimize_batch strip=%d" % strip, " ".join(rows))
        ob.close()

    # refusals: status, message, images in the batch afterwards
    b = jl.Batch(ctx).upload(files[:2], U8)
    buf = np.frombuffer(files[0], np.uint8).copy()
    seg1 = (_capi.Segment * 1)(_capi.Segment(buf.ctypes.data, buf.size))
    one, minus = (C.c_int * 1)(1), (C.c_int * 1)(-1)
    dev = torch.from_numpy(buf).to("cuda:0")
    base = C.c_void_p()
    hip = C.CDLL(None)  # (the HIP runtime the process has loaded already: torch's)
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    hip.hipMalloc.restype = hip.hipFree.restype = C.c_int
    assert hip.hipMalloc(C.byref(base), 100) == 0
    p1, l1 = lambda p: (C.c_void_p * 1)(p), lambda n: (C.c_size_t * 1)(n)
    refusals = [
        ("upload: null argument", lambda: lib.jpgpu_batch_upload(b._h, None, l1(5), 1, U8)),
        ("upload_segments: null argument", lambda: lib.jpgpu_batch_upload_segments(b._h, None, one, 1, U8, 0)),
        ("upload_segments: null counts", lambda: lib.jpgpu_batch_upload_segments(b._h, seg1, None, 1, U8, 0)),
        ("upload_segments: negative segment count", lambda: lib.jpgpu_batch_upload_segments(b._h, seg1, minus, 1, U8, 0)),
        ("upload_segments: null segment with a length", lambda: lib.jpgpu_batch_upload_segments(b._h, (_capi.Segment * 1)(_capi.Segment(None, 7)), one, 1, U8, 0)),
        ("upload_segments: unknown flag", lambda: lib.jpgpu_batch_upload_segments(b._h, seg1, one, 1, U8, 8)),
        ("upload_segments: unknown format", lambda: lib.jpgpu_batch_upload_segments(b._h, seg1, one, 1, 99, 0)),
        ("upload_device: null argument", lambda: lib.jpgpu_batch_upload_device(b._h, None, l1(5), 1, U8)),
        ("upload_device: null lengths", lambda: lib.jpgpu_batch_upload_device(b._h, p1(dev.data_ptr()), None, 1, U8)),
        ("upload_device: null pointer", lambda: lib.jpgpu_batch_upload_device(b._h, p1(None), l1(5), 1, U8)),
        ("upload_device: unknown format", lambda: lib.jpgpu_batch_upload_device(b._h, p1(dev.data_ptr()), l1(dev.numel()), 1, -1)),
        ("upload_device: a host pointer", lambda: lib.jpgpu_batch_upload_device(b._h, p1(buf.ctypes.data), l1(buf.size), 1, U8)),
        ("upload_device: a range beyond its allocation", lambda: lib.jpgpu_batch_upload_device(b._h, p1(base.value), l1(1 << 20), 1, U8)),
    ]
    for label, call in refusals:
        b.upload(files[:2], U8)
        rc = call()
        emit("refused " + label, "status=%d message=%r n_images=%d %s" % (rc, last_error(ctx), len(b), stats(b)))
    describe(b.upload_tensors([dev], U8), "a good upload behind the refusals")
    assert hip.hipFree(base) == 0
    b.close()
    ctx.close()

    with open(args.raw, "w") as f:
        f.write("\n".join(LINES) + "\n")
    with open(args.digest, "w") as f:
        for line in LINES:
            f.write("%s | %s\n" % (line.split(" | ", 1)[0], hashlib.sha256(line.encode()).hexdigest()[:16]))
    print("%d lines, sha256 of the raw log %s" % (len(LINES), sha(("\n".join(LINES) + "\n").encode())))


if __name__ == "__main__":
    main()
