#!/usr/bin/env python3
"""tools/bench_decode_ingest.py -- what the decoder's upload costs by where the files lie: pageable host memory, one page-locked
arena, device memory (jpgpu_batch_upload_device), and device memory delivered by one hipMemcpyAsync per file first.
Not the headline benchmark (that is bench.py); prints one JSON line.

    python tools/bench_decode_ingest.py [--images 1024] [--steps 5] [--warmup 2] [--workload 4k_dri4]

ONE process, the headline file set (bench.py's generator and seeds), the same files for every input:
    pageable        Batch.upload(files)                            the staging ring
    pinned_arena    Batch.upload_segments(views, arena=True)       a few large DMAs from one page-locked arena
    device          Batch.upload_tensors(views of one tensor)      gather_device_kernel + heads + verdict, nothing else over the link
    device_memcpy   one hipMemcpyAsync D2D per file into 256-aligned slots of a second tensor (issued here, through the HIP runtime: the
                    naive form the gather replaces), a stream synchronisation, then upload_tensors of that tensor's views
For each: ms per upload and ms per upload + decode + sync (median and minimum over --steps), the ingest statistics of the last upload,
and one image against the oracle.  `ratios` holds the two figures the feature is held to (device upload over pinned-arena upload,
gather over per-file copies: each should be <= 1; the gather by the events around the kernel, the copies by events around their
issue and as wall time of issue + synchronisation) and `gather` the kernel's achieved bytes/s, read plus write."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _hip(name, *argtypes):
    """a function of the HIP runtime the process has loaded already (torch's copy: jpeglibrary_amd/_capi.py)"""
    fn = getattr(C.CDLL(None), name)
    fn.restype, fn.argtypes = C.c_int, list(argtypes)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=0, help="files per upload (default: the workload's batch size)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="4k_dri4")
    ap.add_argument("--gen-threads", type=int, default=0)
    args = ap.parse_args()

    import torch

    import bench
    import jpeglibrary_amd as jl
    from oracle import pyoracle as po
    from tools import jpegsynth

    n = args.images or bench.WORKLOADS[args.workload][5]
    gen_threads = args.gen_threads or bench.granted_cpus(bench.host_cpu_budget())
    files, sizes, _, _ = bench.make_inputs(jl.sharding, jpegsynth, args.workload, n, 0, gen_threads)
    total = int(sum(len(f) for f in files))
    ctx = jl.default_context()
    dev = torch.device("cuda", ctx.device)

    # the same bytes three times: where they were generated (pageable), in one page-locked arena, in one device tensor
    offs, pos = [], 0
    for f in files:
        offs.append(pos)
        pos += (len(f) + 255) // 256 * 256
    arena = ctx.host_alloc(pos)
    for f, at in zip(files, offs):
        arena[at:at + len(f)] = f
    pinned = [arena[at:at + len(f)] for f, at in zip(files, offs)]
    on_device = torch.from_numpy(arena).to(dev)
    tensors = [on_device[at:at + len(f)] for f, at in zip(files, offs)]
    torch.cuda.synchronize(dev)

    # the naive delivery: one D2D copy per file into a second tensor, on the null stream, between two events
    staged = torch.zeros_like(on_device)
    staged_views = [staged[at:at + len(f)] for f, at in zip(files, offs)]
    memcpy_async = _hip("hipMemcpyAsync", C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
    stream_sync = _hip("hipStreamSynchronize", C.c_void_p)
    event_record = _hip("hipEventRecord", C.c_void_p, C.c_void_p)
    elapsed = _hip("hipEventElapsedTime", C.POINTER(C.c_float), C.c_void_p, C.c_void_p)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert _hip("hipEventCreate", C.POINTER(C.c_void_p))(C.byref(e)) == 0
    pairs = [(d.data_ptr(), s.data_ptr(), len(f)) for d, s, f in zip(staged_views, tensors, files)]
    copies_wall, copies_dev = [], []

    def device_memcpy(b):
        t0 = time.perf_counter()
        event_record(ev[0], None)
        for d, s, m in pairs:
            if memcpy_async(d, s, m, 3, None) != 0:  # hipMemcpyDeviceToDevice
                raise RuntimeError("hipMemcpyAsync failed")
        event_record(ev[1], None)
        if stream_sync(None) != 0:
            raise RuntimeError("hipStreamSynchronize failed")
        copies_wall.append((time.perf_counter() - t0) * 1e3)
        ms = C.c_float()
        elapsed(C.byref(ms), ev[0], ev[1])
        copies_dev.append(ms.value)
        return b.upload_tensors(staged_views, jl.FMT_INTERLEAVED_U8)

    forms = {"pageable": lambda b: b.upload(files, jl.FMT_INTERLEAVED_U8),
             "pinned_arena": lambda b: b.upload_segments(pinned, jl.FMT_INTERLEAVED_U8, arena=True),
             "device": lambda b: b.upload_tensors(tensors, jl.FMT_INTERLEAVED_U8),
             "device_memcpy": device_memcpy}
    ref = po.decode_8bit(bytes(files[n // 2]))[0]
    inputs = {}
    for name, upload in forms.items():
        b = jl.Batch(ctx)
        for _ in range(args.warmup):
            upload(b).decode().sync()
        up, both, gather = [], [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            upload(b)
            t1 = time.perf_counter()
            b.decode().sync()
            t2 = time.perf_counter()
            up.append((t1 - t0) * 1e3)
            both.append((t2 - t0) * 1e3)
            gather.append(b.device_ingest_stats()["gather_ms"])
        st = b.ingest_stats()
        row = {"upload_ms_median": round(float(np.median(up)), 3), "upload_ms_min": round(min(up), 3),
               "upload_decode_ms_median": round(float(np.median(both)), 3), "upload_decode_ms_min": round(min(both), 3),
               "ingest_stats": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()},
               "bit_exact_vs_oracle": bool(b.result(n // 2).status == 0 and np.array_equal(b.output(n // 2), ref))}
        if name.startswith("device"):
            row["device_ingest_stats"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in b.device_ingest_stats().items()}
            row["gather_ms_median"] = round(float(np.median(gather)), 4)
            row["gather_ms_min"] = round(min(gather), 4)
        if name == "device_memcpy":
            row["per_file_copies_ms_wall_median"] = round(float(np.median(copies_wall[-args.steps:])), 4)
            row["per_file_copies_ms_events_median"] = round(float(np.median(copies_dev[-args.steps:])), 4)
        inputs[name] = row
        b.close()
    g = inputs["device"]["gather_ms_median"]
    out = {"metric": "ms per jpgpu_batch_upload by where the files lie (%s, %d files, %.1f MB)" % (args.workload, n, total / 1e6),
           "value": inputs["device"]["upload_ms_median"], "unit": "ms", "images": n, "steps": args.steps, "compressed_bytes": total, "inputs": inputs,
           "ratios": {"device_upload_over_pinned_arena_upload": round(inputs["device"]["upload_ms_median"] / inputs["pinned_arena"]["upload_ms_median"], 4),
                      "gather_over_per_file_copies_events": round(g / inputs["device_memcpy"]["per_file_copies_ms_events_median"], 4),
                      "gather_over_per_file_copies_wall": round(g / inputs["device_memcpy"]["per_file_copies_ms_wall_median"], 4),
                      "device_upload_over_copies_plus_upload": round(inputs["device"]["upload_ms_median"] / inputs["device_memcpy"]["upload_ms_median"], 4)},
           "gather": {"ms": g, "read_plus_write_TB_per_s": round(2 * total / (g * 1e-3) / 1e12, 3) if g > 0 else None,
                      "copy_ceiling_TB_per_s": "5.36-5.7 (README: the chip's measured copy rate, read plus write)"}}
    print(json.dumps(out))
    ctx.host_free(arena)


if __name__ == "__main__":
    main()
