"""What orientation="file" costs a torch consumer of phone photos (recorded in RESULTS.md, no test gate; a first measurement).

    python tools/bench_decode_orient.py [--images 256] [--reps 10] [--warmup 2] [--width 3840] [--height 2160]

`--images` 4:2:0 files of 3840 x 2160 at Q75 (the headline benchmark's recipe), every one with an Exif block of orientation 6.  ONE process;
per repetition, in the order A B A B:
  A  decode_to_tensors(files, orientation="file"): uint8 [3, W, H] tensors, turned by the library's one K3O launch behind K3's generic class;
  B  decode_to_tensors(files), as stored, through K3's fast class, then t.transpose(1, 2).flip(2).contiguous() per image in torch -- what a
     caller does without the feature.
A step is timed with the host's clock from before the call to behind a synchronise of the device; both include the upload.  Before any
timing the two results are compared (they must be equal).  Behind each round one decode() of two resident batches gives stage_ms()["idct"]
of the oriented route (K3's generic class + K3O) and of the stored one (K3's fast class, no turn).  K3O's own time is a kernel's and comes from
a profiler run of this tool (rocprofv3 --kernel-trace --stats -- python tools/bench_decode_orient.py --reps 2): `k3o_bytes` is what it moves,
3 bytes read and 3 written per pixel.  Medians over reps behind `--warmup` rounds.  One JSON line on stdout."""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeglibrary_amd as jl  # noqa: E402
from tools import jpegsynth  # noqa: E402


def exif_segment(o):
    """an APP1 "Exif" segment, little-endian, whose IFD0 holds Make, Orientation = o and Software"""
    entries = struct.pack("<HHI4s", 0x010F, 2, 4, b"abc\0") + struct.pack("<HHIHH", 0x0112, 3, 1, o, 0) + struct.pack("<HHI4s", 0x0131, 2, 4, b"xyz\0")
    tiff = b"II" + struct.pack("<HI", 42, 8) + struct.pack("<H", 3) + entries + struct.pack("<I", 0)
    payload = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def oriented_files(n, w, h, o=6):
    buf, sizes, stride = jpegsynth.encode_batch(n, w, h, "420", 75, 0, seed0=20261019, nthreads=min(16, os.cpu_count() or 1))
    seg = exif_segment(o)
    return [bytes(buf[i * stride:i * stride + 2]) + seg + bytes(buf[i * stride + 2:i * stride + int(sizes[i])]) for i in range(n)]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    W, H = args.width, args.height
    files = oriented_files(args.images, W, H)
    assert all(jl.identify_orientation(f) == 6 for f in files[:4])
    n = len(files)
    dev = torch.device("cuda", jl.default_context().device)

    def step_a():
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files, orientation="file")
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, tensors

    def step_b():
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files)
        out = [t.transpose(1, 2).flip(2).contiguous() for t in tensors]
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    (_, xa), (_, xb) = step_a(), step_b()
    assert len(xa) == len(xb) == n and all(a is not None and tuple(a.shape) == (3, W, H) and torch.equal(a, b) for a, b in zip(xa, xb))
    del xa, xb
    res_a = jl.Batch().set_orientation_policy("file").upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    res_b = jl.Batch().upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    work_a, work_b = res_a.plan_stats()["idct_work"], res_b.plan_stats()["idct_work"]
    assert work_a[0] > 0 and sum(work_a[1:]) == 0 and work_b[0] == 0, (work_a, work_b)  # the generic class against the fast one
    for r in (res_a, res_b):
        r.stage_ms()  # (drops the first decode's events)

    def stages():
        out = []
        for r in (res_a, res_b):
            r.decode().sync()
            out.append(r.stage_ms())
        return out

    for _ in range(args.warmup):
        step_a()
        step_b()
        stages()
    series = {"A1": [], "B1": [], "A2": [], "B2": [], "idct_oriented": [], "idct_stored": [], "huffman_oriented": [], "huffman_stored": []}
    for _ in range(args.reps):
        for name, step in (("A1", step_a), ("B1", step_b), ("A2", step_a), ("B2", step_b)):
            ms, out = step()
            series[name].append(ms)
            del out
        ka, kb = stages()
        series["idct_oriented"].append(ka["idct"])
        series["idct_stored"].append(kb["idct"])
        series["huffman_oriented"].append(ka["huffman"])
        series["huffman_stored"].append(kb["huffman"])
    med = {k: float(np.median(v)) for k, v in series.items()}
    a_med, b_med = float(np.median(series["A1"] + series["A2"])), float(np.median(series["B1"] + series["B2"]))
    print(json.dumps({"what": "decode_oriented_step_ms", "images": n, "width": W, "height": H, "orientation": 6, "reps": args.reps,
                      "compressed_bytes": sum(map(len, files)), "A_orientation_file_median_ms": a_med, "B_stored_then_torch_median_ms": b_med,
                      "A_over_B": a_med / b_med, "spread_A2_over_A1": med["A2"] / med["A1"], "spread_B2_over_B1": med["B2"] / med["B1"],
                      "idct_stage_generic_plus_k3o_ms": med["idct_oriented"], "idct_stage_fast_class_ms": med["idct_stored"],
                      "huffman_stage_dense_handoff_ms": med["huffman_oriented"], "huffman_stage_stored_ms": med["huffman_stored"],
                      "k3o_bytes": n * W * H * 6, "median_ms": med, "min_ms": {k: min(v) for k, v in series.items()},
                      "max_ms": {k: max(v) for k, v in series.items()}, "series_ms": {k: [round(x, 4) for x in v] for k, v in series.items()}}))


if __name__ == "__main__":
    main()
