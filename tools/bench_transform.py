#!/usr/bin/env python3
"""tools/bench_transform.py -- the optimizer's lossless transform next to the optimizer itself, on the optimizer's bench corpus
(tools/bench_optimize.py: 256 x 4K 4:2:0 Q75 DRI = 7).  One process alternates

    optimize_batch(files)                          unchanged code: the figure of the commit in front of the transform
    optimize_batch(files, orientations=[6] * n)    a quarter turn: blocks transposed, source lines a grid row apart
    optimize_batch(files, orientations=[2] * n)    a mirror: signs only

and prints one JSON line: the step times and their ratio, KX's launch alone (an event pair of its own), KX's bytes per second against the copy
ceiling RESULTS.md records for this part, and what the road in front of KX costs (the entropy decode, the dense copy of split scans: event
pairs as well).

    python tools/bench_transform.py [--images 256] [--steps 5] [--dri 7]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBS = (5.36, 5.7)  # RESULTS.md: device-to-device copy on this part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--dri", type=int, default=7)
    args = ap.parse_args()
    import jpeglibrary_amd as jl
    from tools import jpegsynth

    from bench import granted_cpus, host_cpu_budget
    threads = granted_cpus(host_cpu_budget())
    buf, sizes, stride = jpegsynth.encode_batch(args.images, args.width, args.height, "420", args.quality, args.dri, seed0=1, nthreads=threads)
    files = [bytes(buf[i * stride:i * stride + int(sizes[i])]) for i in range(args.images)]
    n = len(files)
    roads = {"plain": None, "turn6": [6] * n, "mirror2": [2] * n}
    batches = {}
    for name, orients in roads.items():
        b = jl.OptimizeBatch()
        if orients:
            b.set_orientations(orients)
        batches[name] = b.upload(files, True).run()  # (warm: buffers allocated, code objects loaded)
    wall = {name: [] for name in roads}
    dev = {name: [] for name in roads}
    stages = {name: [] for name in roads}
    for _ in range(args.steps):
        for name, b in batches.items():
            t0 = time.perf_counter()
            b.run()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            dev[name].append(b.last_ms())
            stages[name].append(b.turn_stage_ms())
    mean = lambda v: sum(v) / len(v)
    blocks = n * ((args.width + 15) // 16) * ((args.height + 15) // 16) * 6
    out = {"metric": "ms per step, optimizer with and without the lossless transform", "images": n, "dri": args.dri, "steps": args.steps,
           "blocks": blocks, "copy_ceiling_TBs": list(COPY_CEILING_TBS)}
    for name in roads:
        row = {"ms_per_step": round(mean(wall[name]), 3), "device_ms": round(mean(dev[name]), 3), "output_MB": round(sum(batches[name].result(i)[1] for i in range(n)) / 1e6, 1)}
        if roads[name]:
            kx, decode, dense = (mean([s[k] for s in stages[name]]) for k in range(3))
            tbs = 2 * blocks * 128 / (kx / 1e3) / 1e12 if kx > 0 else 0.0
            row.update({"kx_ms": round(kx, 4), "kx_TBs": round(tbs, 3), "kx_frac_of_copy_ceiling": round(tbs / COPY_CEILING_TBS[0], 3),
                        "entropy_decode_ms": round(decode, 3), "dense_copy_ms": round(dense, 3),
                        "ratio_to_plain": round(mean(wall[name]) / mean(wall["plain"]), 3)})
        out[name] = row
    print(json.dumps(out))
    for b in batches.values():
        b.close()


if __name__ == "__main__":
    main()
