"""What coding="optimized" and coding="progressive" cost against the standard coding under arithmetic="libjpeg", and what Pillow takes for the
same batch (recorded in RESULTS.md; a first measurement, no ratio fixed in advance).

    python tools/bench_encode_progressive.py [--images 64] [--reps 10] [--warmup 2] [--cpus 16]

`--images` pictures of 3840 x 2160 RGB (bench_encode.py's synthetic content, eight distinct ones) as (H, W, 3) tensors on the device, to
4:2:0 at Q75.  ONE process; three resident batches, one per coding, and per repetition, in the order S O P S O P:
  S  coding="standard":     E1J, then the one-pass entropy stage over the Annex K tables;
  O  coding="optimized":    E1J, the statistics kernel and libjpeg's table build on the host, then the same entropy stage;
  P  coding="progressive":  E1J, then EP1 .. EP6 (encode_progressive.hip) over the ten scans of every image.
A step is timed with the host's clock around encode(), which ends with a synchronise of the context's stream; stage_ms() of the same call
gives the device time by stage (include/jpgpu.h, 4e says which kernel counts where).  Before any timing image 0 of every coding is compared
with Pillow's file for the same pixels (they must be equal).  Pillow's time is Image.save of the same batch into memory on a pool of `--cpus`
threads, best of three, per coding.  Medians over reps behind `--warmup` rounds.  One JSON line on stdout."""
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
PILLOW = {"standard": {}, "optimized": {"optimize": True}, "progressive": {"progressive": True}}
STAGES = ("fdct_quant", "block_bits", "emit", "stuff", "total")


def pillow_file(a, coding):
    from PIL import Image

    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", quality=QUALITY, subsampling=2, **PILLOW[coding])
    return f.getvalue()


def pillow_batch_ms(images, n, cpus, coding):
    best = None
    with ThreadPoolExecutor(cpus) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            sizes = list(pool.map(lambda i: len(pillow_file(images[i % len(images)], coding)), range(n)))
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
    images = [image(W, H, 20261021 + k) for k in range(min(8, args.images))]
    tensors = [torch.from_numpy(a).to(dev) for a in images]
    batch = [tensors[i % len(tensors)] for i in range(args.images)]
    codings = ("standard", "optimized", "progressive")
    enc = {c: jl.EncodeBatch().upload_tensors(batch, (2, 2), QUALITY, rgb=True, layout="hwc", arithmetic="libjpeg", coding=c) for c in codings}
    for c in codings:
        enc[c].encode()
        assert enc[c].coding(0) == c
        assert enc[c].output(0) == pillow_file(images[0], c), "image 0 under coding=%r differs from Pillow's file" % c
    file_bytes = {c: int(sum(len(enc[c].output(i)) for i in range(min(8, args.images)))) for c in codings}  # the distinct pictures

    def step(c):
        t0 = time.perf_counter()
        enc[c].encode()
        return (time.perf_counter() - t0) * 1e3, enc[c].stage_ms()

    for _ in range(args.warmup):
        for c in codings:
            step(c)
    series = {c: {k: [] for k in ("step",) + STAGES} for c in codings}
    for _ in range(args.reps):
        for c in codings:
            ms, stages = step(c)
            series[c]["step"].append(ms)
            for k in STAGES:
                series[c][k].append(stages[k])
    med = {c: {k: float(np.median(v)) for k, v in series[c].items()} for c in codings}
    pillow_ms = {c: pillow_batch_ms(images, args.images, args.cpus, c) for c in codings}
    for e in enc.values():
        e.close()
    dominant = {c: max(STAGES[:4], key=lambda k: med[c][k]) for c in codings}
    print(json.dumps({"what": "encode_progressive_ms", "images": args.images, "width": W, "height": H, "quality": QUALITY, "subsampling": "4:2:0",
                      "reps": args.reps, "image0_equals_pillow": True, "file_bytes_first_8": file_bytes,
                      "encode_step_median_ms": {c: med[c]["step"] for c in codings},
                      "stage_median_ms": {c: {k: med[c][k] for k in STAGES} for c in codings}, "dominant_stage": dominant,
                      "step_over_standard": {c: med[c]["step"] / med["standard"]["step"] for c in codings},
                      "pillow": {"threads": args.cpus, "batch_ms_best_of_3": pillow_ms,
                                 "pillow_over_step": {c: pillow_ms[c] / med[c]["step"] for c in codings}},
                      "series_step_ms": {c: [round(y, 3) for y in series[c]["step"]] for c in codings}}), flush=True)


if __name__ == "__main__":
    main()
