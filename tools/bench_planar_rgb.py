"""What RGB_PLANAR_U8 costs in K3 beside RGB_U8 (recorded in RESULTS.md, no test gate).

    python tools/bench_planar_rgb.py [--images 256] [--reps 20] [--warmup 3]

The headline's input -- `--images` files of 3840 x 2160 4:2:0 Q75 DRI = 4 from bench.py's generator -- uploaded once per format into
three batches of ONE process, inputs resident.  Per repetition, in this order:  A  RGB_U8,  B  RGB_PLANAR_U8,  A again,  B again,
then  P  PLANAR_U8 (the byte-bound floor: no conversion, no chroma replication, a third fewer bytes).  Each figure is
Batch.stage_ms()["idct"] of one decode(): HIP events around K3 on the stream it ran on (a query behind every decode(), so each figure
is one decode's).  Medians over reps (A and B: 2 x reps decodes each) behind `--warmup` rounds.
The spread between the two A series is the measurement's own; B / A is read against it.  One JSON line on stdout."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeglibrary_amd as jl  # noqa: E402
from jpeglibrary_amd import sharding  # noqa: E402
from tools import jpegsynth  # noqa: E402

W, H = 3840, 2160


def resident(files, fmt):
    b = jl.Batch().upload(files, fmt).decode().sync()
    b.stage_ms()  # (drops the first decode's events)
    return b


def idct_ms(b):
    b.decode().sync()
    return b.stage_ms()["idct"]  # (exactly this decode's: every query starts the record again)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gen-threads", type=int, default=0)
    args = ap.parse_args()
    threads = args.gen_threads or min(16, len(os.sched_getaffinity(0)))
    buf, sizes, stride = jpegsynth.encode_batch(args.images, W, H, "420", 75, 4, seed0=sharding.rank_seed_base(0), nthreads=threads)
    files = [buf[i * stride:i * stride + int(sizes[i])] for i in range(args.images)]
    a, b, p = resident(files, jl.FMT_RGB_U8), resident(files, jl.FMT_RGB_PLANAR_U8), resident(files, jl.FMT_PLANAR_U8)
    # the two sinks hold the same bytes (image 0, after the timing's own kernels have run once)
    same = bool(np.array_equal(b.output(0), a.output(0).transpose(2, 0, 1)))
    for _ in range(args.warmup):
        for x in (a, b, p):
            idct_ms(x)
    series = {"A1": [], "B1": [], "A2": [], "B2": [], "P": []}
    for _ in range(args.reps):
        for name, x in (("A1", a), ("B1", b), ("A2", a), ("B2", b), ("P", p)):
            series[name].append(idct_ms(x))
    med = {k: float(np.median(v)) for k, v in series.items()}
    a_med, b_med = float(np.median(series["A1"] + series["A2"])), float(np.median(series["B1"] + series["B2"]))
    out_gb = args.images * W * H * 3 / 1e9
    print(json.dumps({"what": "k3_stage_ms_rgb_planar_vs_rgb", "images": args.images, "reps": args.reps, "same_bytes": same,
                      "rgb_u8_median_ms": a_med, "rgb_planar_u8_median_ms": b_med, "planar_u8_median_ms": med["P"],
                      "rgb_planar_over_rgb": b_med / a_med, "spread_A2_over_A1": med["A2"] / med["A1"], "spread_B2_over_B1": med["B2"] / med["B1"],
                      "output_GBps_rgb_u8": out_gb / (a_med * 1e-3), "output_GBps_rgb_planar_u8": out_gb / (b_med * 1e-3),
                      "median_ms": med, "min_ms": {k: min(v) for k, v in series.items()}, "max_ms": {k: max(v) for k, v in series.items()},
                      "series_ms": {k: [round(x, 4) for x in v] for k, v in series.items()}}))


if __name__ == "__main__":
    main()
