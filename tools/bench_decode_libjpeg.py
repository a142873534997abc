"""What arithmetic="libjpeg" costs against the default decode and against upsampling="fancy" alone (recorded in RESULTS.md; a first
measurement, no ratio fixed in advance).

    python tools/bench_decode_libjpeg.py [--images 256] [--reps 10] [--warmup 2]

Two corpora of `--images` 4:2:0 files at Q75 with DRI = 4 (the headline benchmark's recipe): 3840 x 2160 and 1366 x 768.  ONE process; per
corpus and repetition, in the order A B J L A B J L:
  A  decode_to_tensors(files): K3's fused 4:2:0 class (the generic class for 1366 x 768, whose width is no multiple of 8);
  B  decode_to_tensors(files, upsampling="fancy"): the scratch road -- K3's generic class, then K3U;
  J  decode_to_tensors(files, upsampling="fancy", arithmetic="libjpeg"): the same road with K3J in the generic class's place: libjpeg's pixels;
  L  decode_to_tensors(files, arithmetic="libjpeg"): K3J, then the plain conversion.
A step is timed with the host's clock from before the call to behind a synchronise of the device; all include the upload.  Before any timing
image 0 of J is compared with Pillow's decode of the same file where Pillow is installed (they must be equal).  Behind each step round,
A B J L A B J L, one decode() of four resident batches gives stage_ms()["idct"], the device time of the whole output stage of each route.
Medians over reps behind `--warmup` rounds.  One JSON line per corpus on stdout."""
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
from tools import jpegsynth  # noqa: E402

ROUTES = {"A": {}, "B": {"upsampling": "fancy"}, "J": {"upsampling": "fancy", "arithmetic": "libjpeg"}, "L": {"arithmetic": "libjpeg"}}


def corpus(n, W, H, seed0):
    buf, sizes, stride = jpegsynth.encode_batch(n, W, H, "420", 75, 4, seed0=seed0, nthreads=min(16, os.cpu_count() or 1))
    return [bytes(buf[i * stride:i * stride + int(sizes[i])]) for i in range(n)]


def pillow_planes(f):
    try:
        from PIL import Image
    except ImportError:
        return None
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")).transpose(2, 0, 1))


def measure(torch, dev, files, W, H, reps, warmup):
    n = len(files)

    def step(**kw):
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files, **kw)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, tensors

    _, xj = step(**ROUTES["J"])
    assert len(xj) == n and all(t is not None and tuple(t.shape) == (3, H, W) for t in xj)
    want = pillow_planes(files[0])
    equals_pillow = None if want is None else bool(np.array_equal(xj[0].cpu().numpy(), want))
    assert equals_pillow is not False, "image 0 under arithmetic=\"libjpeg\", upsampling=\"fancy\" differs from Pillow's decode"
    del xj
    res = {}
    for name, kw in ROUTES.items():
        b = jl.Batch().set_upsampling_policy(kw.get("upsampling", "replicate")).set_arithmetic_policy(kw.get("arithmetic", "reference"))
        res[name] = b.upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    assert all(res[x].arithmetic(i) == 1 for x in "JL" for i in (0, n - 1)) and res["J"].plan_stats()["idct_listed_mcus"] == 0  # K3J's, none in K3's lists
    assert all(res[x].arithmetic(i) == 0 for x in "AB" for i in (0, n - 1))
    work = {x: res[x].plan_stats()["idct_work"] for x in "AB"}
    for r in res.values():
        r.stage_ms()  # (drops the first decode's events)

    def stage(name):
        res[name].decode().sync()
        return res[name].stage_ms()["idct"]

    for _ in range(warmup):
        for name, kw in ROUTES.items():
            step(**kw)
            stage(name)
    series = {x + k: [] for x in ROUTES for k in ("1", "2")}
    series.update({"out_" + x + k: [] for x in ROUTES for k in ("1", "2")})
    for _ in range(reps):
        for k in ("1", "2"):
            for name, kw in ROUTES.items():
                ms, out = step(**kw)
                del out
                series[name + k].append(ms)
        for k in ("1", "2"):  # A B J L A B J L on the resident batches
            for name in ROUTES:
                series["out_" + name + k].append(stage(name))
    med = {name: float(np.median(v)) for name, v in series.items()}
    stepm = {x: float(np.median(series[x + "1"] + series[x + "2"])) for x in ROUTES}
    outm = {x: float(np.median(series["out_" + x + "1"] + series["out_" + x + "2"])) for x in ROUTES}
    pairs_jb = [j / b for k in ("1", "2") for b, j in zip(series["out_B" + k], series["out_J" + k])]
    pairs_ja = [j / a for k in ("1", "2") for a, j in zip(series["out_A" + k], series["out_J" + k])]
    blocks = n * ((W + 15) // 16) * ((H + 15) // 16) * 6
    for r in res.values():
        r.close()
    return {"what": "decode_libjpeg_ms", "images": n, "width": W, "height": H, "reps": reps, "compressed_bytes": sum(map(len, files)),
            "image0_equals_pillow": equals_pillow, "k3_idct_work_by_class": work, "blocks": blocks,
            "step_median_ms": stepm, "output_stage_median_ms": outm,
            "J_over_B_output_stage": outm["J"] / outm["B"], "J_over_A_output_stage": outm["J"] / outm["A"], "L_over_A_output_stage": outm["L"] / outm["A"],
            "J_over_B_step": stepm["J"] / stepm["B"], "J_over_A_step": stepm["J"] / stepm["A"],
            "J_minus_B_output_stage_ms": outm["J"] - outm["B"],
            "J_over_B_output_stage_pairs_min_max": [min(pairs_jb), max(pairs_jb)], "J_over_A_output_stage_pairs_min_max": [min(pairs_ja), max(pairs_ja)],
            "spread_second_over_first": {x: med[x + "2"] / med[x + "1"] for x in ROUTES},
            "median_ms": med, "min_ms": {x: min(v) for x, v in series.items()}, "max_ms": {x: max(v) for x, v in series.items()},
            "series_ms": {x: [round(y, 4) for y in v] for x, v in series.items()}}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", jl.default_context().device)
    for W, H, seed0 in ((3840, 2160, 20261020), (1366, 768, 20261021)):
        files = corpus(args.images, W, H, seed0)
        print(json.dumps(measure(torch, dev, files, W, H, args.reps, args.warmup)), flush=True)
        del files


if __name__ == "__main__":
    main()
