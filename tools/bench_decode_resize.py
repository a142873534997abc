"""What the resize stage (K4) saves a torch data loader that crops and resizes (recorded in RESULTS.md, no test gate).

    python tools/bench_decode_resize.py [--images 256] [--reps 10] [--warmup 2] [--size 224]

The headline's input -- `--images` files of 3840 x 2160 4:2:0 Q75 DRI = 4 from bench.py's generator -- and one random window per image
(seeded; area 8-100 % of the frame, aspect 3/4..4/3, RandomResizedCrop's rule), to float16 [N, 3, size, size] with ImageNet's mean / std.
ONE process; per repetition, in the order A B A B:
  A  decode_to_tensors(windows=..., dtype=float16, mean, std), then per image F.interpolate(t[None].float(), (size, size), mode="bilinear",
     antialias=True).half(), then torch.stack -- N ragged tensors, N small launches and two more passes over the pixels;
  B  decode_resized(files, (size, size), float16, mean, std, windows) -- the same decode and ONE launch behind it.
A step is timed with the host's clock from before the call to behind a synchronise of the device; both include the upload and both end
with one float16 [N, 3, size, size] tensor in device memory.  Before any timing the two results are compared (they differ by the rounding
of two different arithmetics: the largest difference is reported, in float16 units of the normalised samples).  Behind each A B A B round
one decode() of a resident batch with the same windows and resize gives Batch.resize_ms() (K4 alone, an event pair of its own) and
Batch.stage_ms()["idct"] (K3).  Medians over reps behind `--warmup` rounds.  K4's rate counts every source byte of the windows once plus the
bytes it writes.  One JSON line on stdout."""
import argparse
import json
import math
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
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def random_windows(n, seed=20261019):
    """one (x, y, w, h) per image: area 8-100 % of the frame, aspect (w / h) log-uniform in 3/4..4/3; the whole frame after ten misses"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        rect = (0, 0, W, H)
        for _ in range(10):
            area = rng.uniform(0.08, 1.0) * W * H
            aspect = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
            w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                rect = (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h)
                break
        out.append(rect)
    return out


def main():
    import torch
    import torch.nn.functional as F

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--gen-threads", type=int, default=0)
    args = ap.parse_args()
    threads = args.gen_threads or min(16, len(os.sched_getaffinity(0)))
    buf, sizes, stride = jpegsynth.encode_batch(args.images, W, H, "420", 75, 4, seed0=sharding.rank_seed_base(0), nthreads=threads)
    files = [buf[i * stride:i * stride + int(sizes[i])] for i in range(args.images)]
    n, size = len(files), (args.size, args.size)
    windows = random_windows(n)
    consts = jl.affine_from_mean_std(MEAN, STD)
    dev = torch.device("cuda", jl.default_context().device)

    def step_a():
        t0 = time.perf_counter()
        tensors, _ = jl.decode_to_tensors(files, dtype=torch.float16, mean=MEAN, std=STD, windows=windows)
        out = torch.stack([F.interpolate(t[None].float(), size, mode="bilinear", antialias=True).half()[0] for t in tensors])
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    def step_b():
        t0 = time.perf_counter()
        out, _ = jl.decode_resized(files, size, dtype=torch.float16, mean=MEAN, std=STD, windows=windows)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    (_, xa), (_, xb) = step_a(), step_b()
    assert xa.shape == xb.shape == (n, 3) + size and xa.dtype == xb.dtype == torch.float16
    max_diff = float((xa.float() - xb.float()).abs().max())
    del xa, xb
    resident = jl.Batch().set_output_affine(*consts).set_resize(size, torch.float16).set_windows(windows).upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    resident.stage_ms()  # (drops the first decode's events)

    def stages():
        resident.decode().sync()
        return resident.resize_ms(), resident.stage_ms()["idct"]

    for _ in range(args.warmup):
        for step in (step_a, step_b):
            step()
        stages()
    series = {"A1": [], "B1": [], "A2": [], "B2": [], "k4": [], "k3": []}
    for _ in range(args.reps):
        for name, step in (("A1", step_a), ("B1", step_b), ("A2", step_a), ("B2", step_b)):
            ms, out = step()
            series[name].append(ms)
            del out
        k4, k3 = stages()
        series["k4"].append(k4)
        series["k3"].append(k3)
    med = {k: float(np.median(v)) for k, v in series.items()}
    a_med, b_med = float(np.median(series["A1"] + series["A2"])), float(np.median(series["B1"] + series["B2"]))
    read = sum(3 * w * h for _, _, w, h in windows)
    written = n * 3 * size[0] * size[1] * 2
    print(json.dumps({"what": "decode_resize_step_ms_f16", "images": n, "size": list(size), "reps": args.reps, "max_abs_diff_A_B": max_diff,
                      "A_ragged_then_interpolate_median_ms": a_med, "B_decode_resized_median_ms": b_med, "B_over_A": b_med / a_med, "B_below_A": b_med < a_med,
                      "spread_A2_over_A1": med["A2"] / med["A1"], "spread_B2_over_B1": med["B2"] / med["B1"],
                      "resize_ms": med["k4"], "k3_idct_ms": med["k3"], "k4_bytes_read": read, "k4_bytes_written": written,
                      "k4_read_TBps": read / (med["k4"] * 1e-3) / 1e12, "k4_written_TBps": written / (med["k4"] * 1e-3) / 1e12,
                      "k4_total_TBps": (read + written) / (med["k4"] * 1e-3) / 1e12, "window_pixels_mean": read / 3 / n,
                      "median_ms": med, "min_ms": {k: min(v) for k, v in series.items()}, "max_ms": {k: max(v) for k, v in series.items()},
                      "series_ms": {k: [round(x, 4) for x in v] for k, v in series.items()}}))


if __name__ == "__main__":
    main()
