"""What the colour policy "file" costs a torch consumer of CMYK files (recorded in RESULTS.md, no test gate; a first measurement).

    python tools/bench_decode_color.py [--images 256] [--reps 10] [--warmup 2]

`--images` CMYK files of 1024 x 768 at Q85 as Pillow writes them (4 components 1x1, APP14 transform 0).  ONE process; per repetition, in the
order A B A B:
  A  decode_to_tensors(files, color="file"): uint8 [3, H, W] tensors, converted by the library's one K3C launch behind K3;
  B  decode_to_tensors(files, fmt=FMT_INTERLEAVED_U8): uint8 [H, W, 4] tensors of samples, then the same arithmetic in torch per image --
     d(s_c * s_k) in int32, permuted to [3, H, W].
A step is timed with the host's clock from before the call to behind a synchronise of the device; both include the upload.  Before any
timing the two results are compared (they must be equal).  Behind each round one decode() of two resident batches gives
stage_ms()["idct"] of the policy's route (K3's generic class + K3C, RGB_PLANAR_U8) and of INTERLEAVED_U8 (the same K3 work, no converter):
their difference is the converter's device time.  Medians over reps behind `--warmup` rounds.  One JSON line on stdout."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeglibrary_amd as jl  # noqa: E402

W, H = 1024, 768


def cmyk_files(n):
    from PIL import Image

    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    rng = np.random.default_rng(20261019)
    base = np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * 2 + yy * 3) % 256, 255 - (xx + yy) % 200], axis=-1)
    base = np.clip(base + rng.integers(-8, 9, base.shape), 0, 255).astype(np.uint8)
    files = []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(np.roll(base, (7 * i, 13 * i), (0, 1)), "CMYK").save(buf, format="JPEG", quality=85)
        files.append(buf.getvalue())
    return files


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    files = cmyk_files(args.images)
    assert all(jl.identify_color(f) == "cmyk" for f in files)
    n = len(files)
    dev = torch.device("cuda", jl.default_context().device)

    def step_a():
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files, color="file")
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, tensors

    def step_b():
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files, fmt=jl.FMT_INTERLEAVED_U8)
        out = []
        for t in tensors:
            x = t.to(torch.int32)
            p = x[..., :3] * x[..., 3:] + 128
            out.append(((p + (p >> 8)) >> 8).to(torch.uint8).permute(2, 0, 1).contiguous())
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    (_, xa), (_, xb) = step_a(), step_b()
    assert len(xa) == len(xb) == n and all(a is not None and tuple(a.shape) == (3, H, W) and torch.equal(a, b) for a, b in zip(xa, xb))
    del xa, xb
    res_a = jl.Batch().set_color_policy("file").upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    res_b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8).decode().sync()
    assert res_a.plan_stats()["idct_work"] == res_b.plan_stats()["idct_work"]  # the same K3 work: the generic class
    for r in (res_a, res_b):
        r.stage_ms()  # (drops the first decode's events)

    def stages():
        out = []
        for r in (res_a, res_b):
            r.decode().sync()
            out.append(r.stage_ms()["idct"])
        return out

    for _ in range(args.warmup):
        step_a()
        step_b()
        stages()
    series = {"A1": [], "B1": [], "A2": [], "B2": [], "idct_file_policy": [], "idct_samples": []}
    for _ in range(args.reps):
        for name, step in (("A1", step_a), ("B1", step_b), ("A2", step_a), ("B2", step_b)):
            ms, out = step()
            series[name].append(ms)
            del out
        ka, kb = stages()
        series["idct_file_policy"].append(ka)
        series["idct_samples"].append(kb)
    med = {k: float(np.median(v)) for k, v in series.items()}
    a_med, b_med = float(np.median(series["A1"] + series["A2"])), float(np.median(series["B1"] + series["B2"]))
    conv = med["idct_file_policy"] - med["idct_samples"]
    moved = n * W * H * 7  # the converter reads 4 bytes per pixel and writes 3
    print(json.dumps({"what": "decode_cmyk_step_ms", "images": n, "width": W, "height": H, "reps": args.reps, "compressed_bytes": sum(map(len, files)),
                      "A_color_file_median_ms": a_med, "B_samples_then_torch_median_ms": b_med, "A_over_B": a_med / b_med,
                      "spread_A2_over_A1": med["A2"] / med["A1"], "spread_B2_over_B1": med["B2"] / med["B1"],
                      "k3_generic_plus_converter_ms": med["idct_file_policy"], "k3_generic_ms": med["idct_samples"], "converter_ms_by_difference": conv,
                      "converter_TBps": moved / (conv * 1e-3) / 1e12 if conv > 0 else None,
                      "generic_class_Mpixels_per_s": n * W * H / (med["idct_samples"] * 1e-3) / 1e6,
                      "median_ms": med, "min_ms": {k: min(v) for k, v in series.items()}, "max_ms": {k: max(v) for k, v in series.items()},
                      "series_ms": {k: [round(x, 4) for x in v] for k, v in series.items()}}))


if __name__ == "__main__":
    main()
