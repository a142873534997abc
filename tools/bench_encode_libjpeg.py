"""What arithmetic="libjpeg" costs on the write side against the default encode, and what Pillow takes for the same batch (recorded in
RESULTS.md; a first measurement, no ratio fixed in advance).

    python tools/bench_encode_libjpeg.py [--images 64] [--reps 10] [--warmup 2] [--cpus 16]

`--images` pictures of 3840 x 2160 RGB (bench_encode.py's synthetic content, eight distinct ones) as (H, W, 3) tensors on the device, to
4:2:0 at Q75 with the standard tables.  ONE process; two resident batches, one per policy, and per repetition, in the order R J R J:
  R  EncodeBatch.encode() under arithmetic="reference": stage E1 is fdct_fused_kernel<2, 2, 3>;
  J  EncodeBatch.encode() under arithmetic="libjpeg":   stage E1J (e1j_fdct_kernel<2, 2>); everything behind it is the same code.
A step is timed with the host's clock around encode(), which ends with a synchronise of the context's stream; stage_ms()["fdct_quant"] of
the same call is the device time of the stage.  Before any timing image 0 of J is compared with Pillow's file for the same pixels (they
must be equal).  Pillow's time is Image.save(quality=75, subsampling=2) of the same batch into memory on a pool of `--cpus` threads (the
encoder releases the interpreter lock), best of three.  Medians over reps behind `--warmup` rounds.  One JSON line on stdout."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeglibrary_amd as jl  # noqa: E402
from tools.bench_encode import image  # noqa: E402

W, H, QUALITY = 3840, 2160, 75
COPY_CEILING_TBS = (5.36, 5.7)  # the part's measured copy ceiling (RESULTS.md)


def pillow_file(a):
    from PIL import Image

    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", quality=QUALITY, subsampling=2)
    return f.getvalue()


def pillow_batch_ms(images, n, cpus):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return None
    best = None
    with ThreadPoolExecutor(cpus) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            sizes = list(pool.map(lambda i: len(pillow_file(images[i % len(images)])), range(n)))
            ms = (time.perf_counter() - t0) * 1e3
            best = ms if best is None else min(best, ms)
    assert len(sizes) == n
    return best


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpus", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda", jl.default_context().device)
    images = [image(W, H, 20261020 + k) for k in range(min(8, args.images))]
    tensors = [torch.from_numpy(a).to(dev) for a in images]
    batch = [tensors[i % len(tensors)] for i in range(args.images)]
    routes = {"R": "reference", "J": "libjpeg"}
    enc = {x: jl.EncodeBatch().upload_tensors(batch, (2, 2), QUALITY, rgb=True, layout="hwc", arithmetic=p) for x, p in routes.items()}
    for x in routes:
        enc[x].encode()
    assert all(enc["J"].arithmetic(i) == 1 and enc["R"].arithmetic(i) == 0 for i in (0, args.images - 1))
    try:
        equals_pillow = enc["J"].output(0) == pillow_file(images[0])
    except ImportError:
        equals_pillow = None
    assert equals_pillow is not False, "image 0 under arithmetic=\"libjpeg\" differs from Pillow's file"
    stream_bytes = {x: len(enc[x].output(0)) for x in routes}

    def step(x):
        t0 = time.perf_counter()
        enc[x].encode()
        return (time.perf_counter() - t0) * 1e3, enc[x].stage_ms()

    for _ in range(args.warmup):
        for x in routes:
            step(x)
    series = {x + k: [] for x in routes for k in ("_step", "_e1", "_total")}
    for _ in range(args.reps):
        for _ in range(2):  # R J R J
            for x in routes:
                ms, stages = step(x)
                series[x + "_step"].append(ms)
                series[x + "_e1"].append(stages["fdct_quant"])
                series[x + "_total"].append(stages["total"])
    med = {k: float(np.median(v)) for k, v in series.items()}
    pairs = [j / r for r, j in zip(series["R_e1"], series["J_e1"])]
    pixels = args.images * W * H
    floor_bytes = pixels * 3 + pixels * 3  # 3 B/px of pixels in, 1.5 samples/px x int16 = 3 B/px of blocks out
    floor_ms = [floor_bytes / (c * 1e12) * 1e3 for c in COPY_CEILING_TBS]
    pillow_ms = pillow_batch_ms(images, args.images, args.cpus)
    for e in enc.values():
        e.close()
    print(json.dumps({"what": "encode_libjpeg_ms", "images": args.images, "width": W, "height": H, "quality": QUALITY, "subsampling": "4:2:0", "reps": args.reps,
                      "image0_equals_pillow": equals_pillow, "stream_bytes_image0": stream_bytes,
                      "e1_median_ms": {"reference": med["R_e1"], "libjpeg": med["J_e1"]}, "e1_min_ms": {"reference": min(series["R_e1"]), "libjpeg": min(series["J_e1"])},
                      "device_stages_median_ms": {"reference": med["R_total"], "libjpeg": med["J_total"]},
                      "encode_step_median_ms": {"reference": med["R_step"], "libjpeg": med["J_step"]},
                      "byte_floor": {"bytes": floor_bytes, "ms_at_copy_ceiling": floor_ms, "e1j_fraction_of_floor_rate": [f / med["J_e1"] for f in floor_ms]},
                      "e1j_over_e1": med["J_e1"] / med["R_e1"], "e1j_over_e1_pairs_min_max": [min(pairs), max(pairs)],
                      "step_libjpeg_over_reference": med["J_step"] / med["R_step"],
                      "pillow": {"threads": args.cpus, "batch_ms_best_of_3": pillow_ms,
                                 "pillow_over_libjpeg_step": None if pillow_ms is None else pillow_ms / med["J_step"]},
                      "series_ms": {k: [round(y, 4) for y in v] for k, v in series.items()}}), flush=True)


if __name__ == "__main__":
    main()
