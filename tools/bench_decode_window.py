"""What a window saves in K3, and what it saves a torch consumer who would otherwise decode whole frames and slice (recorded in RESULTS.md).

    python tools/bench_decode_window.py [--images 256] [--reps 5] [--warmup 1]

The headline's input -- `--images` files of 3840 x 2160 4:2:0 Q75 DRI = 4 from bench.py's generator -- uploaded once per format
(RGB_PLANAR_U8, RGB_PLANAR_F16) and per window into batches of ONE process, inputs resident:
  A  whole frames;
  B  every image through one window: 1920 x 1080 at (960, 544) and 224 x 224 at (1808, 960), both in the 4:2:0 fast class, and 224 x 224 at
     (1801, 963), which takes the generic class.
Per window and repetition, in the order A B A B: one decode() each, Batch.stage_ms() of exactly that decode (K3 alone: HIP events on its own
stream) and the host's clock from before decode() to behind a synchronise of the device.  A's step ends with torch's
t[:, y:y+h, x:x+w].contiguous() of every image -- the route without windows --, B's with output_tensor(i) of every image.  Before any timing
B's tensor of image 0 is compared bit for bit with A's slice.  Medians over reps behind `--warmup` rounds; the spread between the two A
series is the measurement's own.  One JSON line per format and window on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeglibrary_amd as jl  # noqa: E402
from jpeglibrary_amd import sharding  # noqa: E402
from tools import jpegsynth  # noqa: E402

W, H = 3840, 2160
WINDOWS = [("1920x1080_aligned", (960, 544, 1920, 1080)), ("224x224_aligned", (1808, 960, 224, 224)), ("224x224_generic", (1801, 963, 224, 224))]
FORMATS = [("RGB_PLANAR_U8", jl.FMT_RGB_PLANAR_U8), ("RGB_PLANAR_F16", jl.FMT_RGB_PLANAR_F16)]


def resident(files, fmt, rect=None):
    b = jl.Batch()
    if rect is not None:
        b.set_windows([rect] * len(files))
    b.upload(files, fmt).decode().sync()
    b.stage_ms()  # (drops the first decode's events)
    return b


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gen-threads", type=int, default=0)
    args = ap.parse_args()
    threads = args.gen_threads or min(16, len(os.sched_getaffinity(0)))
    buf, sizes, stride = jpegsynth.encode_batch(args.images, W, H, "420", 75, 4, seed0=sharding.rank_seed_base(0), nthreads=threads)
    files = [buf[i * stride:i * stride + int(sizes[i])] for i in range(args.images)]
    n = len(files)
    for fmt_name, fmt in FORMATS:
        whole = resident(files, fmt)
        dev = torch.device("cuda", whole.ctx.device)
        for win_name, rect in WINDOWS:
            x, y, w, h = rect
            win = resident(files, fmt, rect)

            def step(b, slice_it):
                t0 = time.perf_counter()
                b.decode()
                out = [b.output_tensor(i) for i in range(n)]
                if slice_it:
                    out = [t[:, y:y + h, x:x + w].contiguous() for t in out]
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) * 1e3
                return ms, b.stage_ms(), out  # (exactly this decode's stages: every query starts the record again)

            (_, _, xa), (_, _, xb) = step(whole, True), step(win, False)
            same = bool(torch.equal(xa[0].view(torch.uint8), xb[0].view(torch.uint8))) and tuple(xb[0].shape) == (3, h, w)
            del xa, xb
            for _ in range(args.warmup):
                step(whole, True)
                step(win, False)
            series = {k: {"step_ms": [], "idct": [], "huffman": [], "marker_index": [], "total": []} for k in ("A1", "B1", "A2", "B2")}
            for _ in range(args.reps):
                for name, b, slice_it in (("A1", whole, True), ("B1", win, False), ("A2", whole, True), ("B2", win, False)):
                    ms, stages, out = step(b, slice_it)
                    del out
                    series[name]["step_ms"].append(ms)
                    for k, v in stages.items():
                        series[name][k].append(v)
            med = {name: {k: float(np.median(v)) for k, v in s.items()} for name, s in series.items()}
            pooled = lambda a, b, k: float(np.median(series[a][k] + series[b][k]))  # noqa: E731
            a_k3, b_k3 = pooled("A1", "A2", "idct"), pooled("B1", "B2", "idct")
            a_ms, b_ms = pooled("A1", "A2", "step_ms"), pooled("B1", "B2", "step_ms")
            stats = win.plan_stats()
            print(json.dumps({"what": "window_decode_ab", "format": fmt_name, "window": win_name, "rect": rect, "images": n, "reps": args.reps,
                              "same_bits_image0": same, "idct_work": stats["idct_work"], "idct_listed_mcus": stats["idct_listed_mcus"],
                              "A_whole_k3_ms": a_k3, "B_window_k3_ms": b_k3, "k3_B_over_A": b_k3 / a_k3,
                              "A_whole_then_torch_slice_step_ms": a_ms, "B_window_step_ms": b_ms, "step_B_over_A": b_ms / a_ms,
                              "spread_A2_over_A1_k3": med["A2"]["idct"] / med["A1"]["idct"], "spread_A2_over_A1_step": med["A2"]["step_ms"] / med["A1"]["step_ms"],
                              "pixels_B_over_A": (w * h) / (W * H), "stage_ms_median": med}), flush=True)
            win.close()
        whole.close()


if __name__ == "__main__":
    main()
