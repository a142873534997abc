"""What the scaled decode saves against the full-size decode under the same policies (recorded in RESULTS.md; a first measurement, no
ratio fixed in advance).

    python tools/bench_decode_scaled.py [--images 256] [--reps 10] [--warmup 2]

Two corpora of `--images` 4:2:0 files at Q75 with DRI = 4 (the headline benchmark's recipe): 3840 x 2160 and 1366 x 768.  ONE process; per
corpus and repetition, in the order 1 2 4 8 1 2 4 8:
  1  decode_to_tensors(files, arithmetic="libjpeg", upsampling="fancy"): K3J, then K3U -- libjpeg's full-size pixels;
  2, 4, 8  the same call with scale=2, 4, 8: K3R in K3J's place, the reduced picture; 4:2:0 leaves no chroma ratio, so K3U does not run.
A step is timed with the host's clock from before the call to behind a synchronise of the device; all include the upload and the entropy
stage, which the scale does not change.  Before any timing image 0 at each scale is compared with Pillow's draft() decode of the same file
where Pillow is installed (they must be equal).  Behind the step rounds, in the same order, one decode() of four resident batches per
round gives stage_ms()["idct"], the device time of the whole output stage of each route; the batches are made behind the step rounds and
closed in front of the next ones, so that no round allocates beside tens of gigabytes it does not use.  Then, in the order F S F S,
decode_resized(files, (224, 224)) under the same policies with scale=1 (F) and scale="fit" (S).  The collector runs between the timed
calls, not inside them.
  The comparison is scale 1 in the same process: a reduced scale transforms no more, stores at most a quarter of the bytes and drops K3U,
so the tool ASSERTS that every scaled measurement is below the scale-1 measurement of its round, and prints the ratios.  Medians over
reps behind `--warmup` rounds.  One JSON line per corpus on stdout; the assertion comes behind the last line, and the exit status is 1 if
it fails.
  As recorded (profiles/scaled_ab.txt, RESULTS.md): the assertion holds for all 120 output-stage pairs (largest ratio 0.92) and FAILS for
the host-clocked steps: on 3840 x 2160, 8 of 120 calls -- scale-1 ones among them -- took 4.1-5.0 s instead of 17-31 ms and put pairs at
172, 182 and 154; on 1366 x 768, where a step is 8.5 ms and the scale can save 0.2-0.7, 5 of 20 pairs at 1/2 (largest 1.04) and 2 of 20 at
1/4 (largest 1.18) are at or above 1.  Medians: 25.6 / 21.0 / 17.9 / 17.3 ms and 8.51 / 8.26 / 7.91 / 7.83 ms at scale 1 / 2 / 4 / 8.
  Bytes per 4:2:0 MCU through K3R, as built: 768 B of coefficients in at every scale (six blocks of 128 B; the DMA is cut to the blocks'
first 16-byte piece only where EVERY component of the scan yields one sample, which 4:2:0 at 1/8 does not: its chroma is 2 x 2), and
192, 48, 12 B of samples out at 1/2, 1/4, 1/8 against 768 B at full size."""
import argparse
import gc
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

SCALES = (1, 2, 4, 8)
POLICIES = {"arithmetic": "libjpeg", "upsampling": "fancy"}
MCU_BYTES = {"coefficients_in": {s: 768 for s in SCALES}, "samples_out": {1: 768, 2: 192, 4: 48, 8: 12}, "one_piece_dma_at_an_eighth": False}


def corpus(n, W, H, seed0):
    buf, sizes, stride = jpegsynth.encode_batch(n, W, H, "420", 75, 4, seed0=seed0, nthreads=min(16, os.cpu_count() or 1))
    return [bytes(buf[i * stride:i * stride + int(sizes[i])]) for i in range(n)]


def pillow_planes(f, denom):
    try:
        from PIL import Image
    except ImportError:
        return None
    img = Image.open(io.BytesIO(f))
    w, h = img.size
    if denom > 1:
        img.draft("RGB", (w // denom, h // denom))
        assert img.size == (-(-w // denom), -(-h // denom)), img.size
    return np.ascontiguousarray(np.asarray(img.convert("RGB")).transpose(2, 0, 1))


def measure(torch, dev, files, W, H, reps, warmup):
    n = len(files)

    def step(scale):
        gc.collect()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files, scale=scale, **POLICIES)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, tensors

    def resized(scale):
        gc.collect()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out, results = jl.decode_resized(files, (224, 224), scale=scale, **POLICIES)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    equals_pillow = {}
    for s in SCALES:
        _, x = step(s)
        assert len(x) == n and all(t is not None and tuple(t.shape) == (3, -(-H // s), -(-W // s)) for t in x), s
        want = pillow_planes(files[0], s)
        equals_pillow[s] = None if want is None else bool(np.array_equal(x[0].cpu().numpy(), want))
        assert equals_pillow[s] is not False, "image 0 at scale %d differs from Pillow's draft() decode" % s
        del x
    series = {"%s%d_%s" % (kind, s, k): [] for kind in ("step", "out") for s in SCALES for k in ("1", "2")}
    series.update({"resized_%s_%s" % (s, k): [] for s in ("1", "fit") for k in ("1", "2")})
    for r in range(warmup + reps):
        for k in ("1", "2"):
            for s in SCALES:
                ms, out = step(s)
                del out
                if r >= warmup:
                    series["step%d_%s" % (s, k)].append(ms)
    res = {}
    for s in SCALES:
        b = jl.Batch().set_upsampling_policy("fancy").set_arithmetic_policy("libjpeg").set_scale_policy(s)
        res[s] = b.upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
        assert all(res[s].arithmetic(i) == 1 and res[s].scale(i) == s for i in (0, n - 1)) and res[s].plan_stats()["idct_listed_mcus"] == 0
        assert res[s].upsampling(0) == (1 if s == 1 else 0)  # (4:2:0: no ratio is left in the reduced picture)
        res[s].stage_ms()  # (drops the first decode's events)

    def stage(s):
        res[s].decode().sync()
        return res[s].stage_ms()["idct"]

    for r in range(warmup + reps):
        for k in ("1", "2"):
            for s in SCALES:
                ms = stage(s)
                if r >= warmup:
                    series["out%d_%s" % (s, k)].append(ms)
    for b in res.values():
        b.close()
    for r in range(warmup + reps):
        for k in ("1", "2"):
            for s in (1, "fit"):
                ms, out = resized(s)
                del out
                if r >= warmup:
                    series["resized_%s_%s" % (s, k)].append(ms)
    b = jl.Batch().set_arithmetic_policy("libjpeg").set_scale_fit((224, 224)).upload(files[:1], jl.FMT_RGB_PLANAR_U8)
    fit_scale = b.scale(0)
    b.close()

    def both(name):
        return series[name + "_1"] + series[name + "_2"]

    ratios, pairs = {}, {}
    for kind in ("step", "out"):
        for s in SCALES[1:]:
            p = [x / f for k in ("1", "2") for f, x in zip(series["%s1_%s" % (kind, k)], series["%s%d_%s" % (kind, s, k)])]
            pairs["%s%d_over_%s1" % (kind, s, kind)] = [min(p), max(p)]
            ratios["%s%d_over_%s1" % (kind, s, kind)] = float(np.median(both("%s%d" % (kind, s))) / np.median(both("%s1" % kind)))
    p = [x / f for k in ("1", "2") for f, x in zip(series["resized_1_" + k], series["resized_fit_" + k])]
    pairs["resized_fit_over_resized_1"] = [min(p), max(p)]
    ratios["resized_fit_over_resized_1"] = float(np.median(both("resized_fit")) / np.median(both("resized_1")))
    out = {"what": "decode_scaled_ms", "images": n, "width": W, "height": H, "reps": reps, "compressed_bytes": sum(map(len, files)),
           "image0_equals_pillow_draft": equals_pillow, "fit_scale_for_224": fit_scale, "bytes_per_420_mcu": MCU_BYTES,
           "step_median_ms": {s: float(np.median(both("step%d" % s))) for s in SCALES},
           "output_stage_median_ms": {s: float(np.median(both("out%d" % s))) for s in SCALES},
           "resized_median_ms": {s: float(np.median(both("resized_%s" % s))) for s in ("1", "fit")},
           "median_ratios": ratios, "pair_ratios_min_max": pairs,
           "series_ms": {x: [round(y, 4) for y in v] for x, v in series.items()}}
    print(json.dumps(out), flush=True)
    return {"%dx%d %s" % (W, H, name): mm[1] for name, mm in pairs.items() if mm[1] >= 1.0}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", jl.default_context().device)
    worst = {}
    for W, H, seed0 in ((3840, 2160, 20261020), (1366, 768, 20261021)):
        files = corpus(args.images, W, H, seed0)
        worst.update(measure(torch, dev, files, W, H, args.reps, args.warmup))
        del files
    assert not worst, "a scaled measurement is not below its scale-1 partner (largest ratio of a pair): %r" % worst


if __name__ == "__main__":
    main()
