"""What the float sink saves a torch consumer, and what it costs in K3 (recorded in RESULTS.md, no test gate).

    python tools/bench_float_sink.py [--images 256] [--reps 10] [--warmup 2]

The headline's input -- `--images` files of 3840 x 2160 4:2:0 Q75 DRI = 4 from bench.py's generator -- uploaded once per format into
batches of ONE process, inputs resident.  Per repetition, in the order A B A B:
  A  the route without the sink: decode() to RGB_PLANAR_U8, output_tensor(i), then (t.float() * scale + bias).half() per image in torch;
  B  decode() to RGB_PLANAR_F16 with the same constants, output_tensor(i) per image.
A step is timed with the host's clock from before decode() to behind a synchronise of the device (both end with every float16 tensor of
the batch in device memory).  Before any timing A's and B's tensors of image 0 are compared bit for bit.  Behind each A B A B round one
decode() each of RGB_PLANAR_U8, _F16 and _F32 gives Batch.stage_ms()["idct"]: K3 alone, HIP events on its own stream.
Medians over reps behind `--warmup` rounds.  The spread between the two A series is the measurement's own; B / A is read against it.  The
K3 ratios stand beside the ratio of the bytes the shapes say K3 moves: the coefficients it reads (two bytes per sample: 3 bytes per pixel
of 4:2:0) plus 3, 6 or 12 output bytes per pixel.  One JSON line on stdout."""
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
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def resident(files, fmt, consts):
    b = jl.Batch().set_output_affine(*consts).upload(files, fmt).decode().sync()
    b.stage_ms()  # (drops the first decode's events)
    return b


def idct_ms(b):
    b.decode().sync()
    return b.stage_ms()["idct"]  # (exactly this decode's: every query starts the record again)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gen-threads", type=int, default=0)
    args = ap.parse_args()
    threads = args.gen_threads or min(16, len(os.sched_getaffinity(0)))
    buf, sizes, stride = jpegsynth.encode_batch(args.images, W, H, "420", 75, 4, seed0=sharding.rank_seed_base(0), nthreads=threads)
    files = [buf[i * stride:i * stride + int(sizes[i])] for i in range(args.images)]
    consts = jl.affine_from_mean_std(MEAN, STD)
    u8, f16, f32 = (resident(files, fmt, consts) for fmt in (jl.FMT_RGB_PLANAR_U8, jl.FMT_RGB_PLANAR_F16, jl.FMT_RGB_PLANAR_F32))
    dev = torch.device("cuda", u8.ctx.device)
    scale = torch.from_numpy(consts[0]).to(dev).reshape(3, 1, 1)
    bias = torch.from_numpy(consts[1]).to(dev).reshape(3, 1, 1)
    n = len(files)

    def step_a():
        t0 = time.perf_counter()
        u8.decode()
        out = [(u8.output_tensor(i).float() * scale + bias).half() for i in range(n)]
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    def step_b():
        t0 = time.perf_counter()
        f16.decode()
        out = [f16.output_tensor(i) for i in range(n)]
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    (_, xa), (_, xb) = step_a(), step_b()
    same = bool(torch.equal(xa[0].view(torch.int16), xb[0].view(torch.int16))) and xb[0].dtype == torch.float16
    del xa, xb
    for _ in range(args.warmup):
        for step in (step_a, step_b):
            step()
        for x in (u8, f16, f32):
            idct_ms(x)
    series = {"A1": [], "B1": [], "A2": [], "B2": [], "k3_u8": [], "k3_f16": [], "k3_f32": []}
    for _ in range(args.reps):
        for name, step in (("A1", step_a), ("B1", step_b), ("A2", step_a), ("B2", step_b)):
            ms, out = step()
            series[name].append(ms)
            del out
        for name, x in (("k3_u8", u8), ("k3_f16", f16), ("k3_f32", f32)):
            series[name].append(idct_ms(x))
    med = {k: float(np.median(v)) for k, v in series.items()}
    a_med, b_med = float(np.median(series["A1"] + series["A2"])), float(np.median(series["B1"] + series["B2"]))
    coef = 3.0  # bytes of coefficients per pixel of 4:2:0 (1.5 samples of two bytes)
    print(json.dumps({"what": "float_sink_step_ms_f16_tensors", "images": n, "reps": args.reps, "same_bits_image0": same,
                      "A_u8_then_torch_median_ms": a_med, "B_f16_sink_median_ms": b_med, "B_over_A": b_med / a_med,
                      "spread_A2_over_A1": med["A2"] / med["A1"], "spread_B2_over_B1": med["B2"] / med["B1"],
                      "k3_u8_ms": med["k3_u8"], "k3_f16_ms": med["k3_f16"], "k3_f32_ms": med["k3_f32"],
                      "k3_f16_over_u8": med["k3_f16"] / med["k3_u8"], "k3_f32_over_u8": med["k3_f32"] / med["k3_u8"],
                      "bytes_f16_over_u8": (coef + 6) / (coef + 3), "bytes_f32_over_u8": (coef + 12) / (coef + 3),
                      "median_ms": med, "min_ms": {k: min(v) for k, v in series.items()}, "max_ms": {k: max(v) for k, v in series.items()},
                      "series_ms": {k: [round(x, 4) for x in v] for k, v in series.items()}}))


if __name__ == "__main__":
    main()
