#!/usr/bin/env python3
"""tools/bench_crop.py -- the optimizer's lossless window next to the optimizer itself, on the optimizer's bench corpus
(tools/bench_optimize.py: 256 x 4K 4:2:0 Q75 DRI = 7).  One process alternates

    optimize_batch(files)                                              untouched
    optimize_batch(files, windows=[centre] * n, origin="expand")        a centred 1920 x 1080 window
    optimize_batch(files, windows=[centre6] * n, orientations=[6] * n)  a centred 1920 x 1080 window of the quarter-turned frame
    optimize_batch([files[0]] * 64, windows=tiles)                      64 tiles of 512 x 512 from ONE file listed 64 times
    optimize_batch(files[:64], windows=tiles)                           the same tiles from 64 distinct files

and prints one JSON line: the step times, and beside each road of the coefficient kind turn_stage_ms() (KX alone, the entropy decode in front
of it, the dense copy of split scans) and turn_sources().  The entropy decode covers the WHOLE scan of every source whatever the window keeps;
the column worth reading is the tiles' decode stage, one source against 64.  A 4K frame holds 7 x 4 whole tiles of 512 x 512, so the 8 x 8 tiles
overlap: their origins step by 464 and 224 pixels, multiples of the 16-pixel MCU.

    python tools/bench_crop.py [--images 256] [--steps 5] [--dri 7]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    n, W, H = len(files), args.width, args.height
    centre = ((W - 1920) // 2, (H - 1080) // 2, 1920, 1080)
    centre6 = ((H - 1920) // 2, (W - 1080) // 2, 1920, 1080)  # (the turned frame is H x W)
    k = min(64, n)
    tiles = [((W - 512) // 7 // 16 * 16 * (t % 8), (H - 512) // 7 // 16 * 16 * (t // 8), 512, 512) for t in range(64)][:k]
    # name -> (files, windows, orientations)
    roads = {"plain": (files, None, None), "window": (files, [centre] * n, None), "window_turn6": (files, [centre6] * n, [6] * n),
             "tiles_one_file": ([files[0]] * k, tiles, None), "tiles_distinct_files": (files[:k], tiles, None)}
    batches = {}
    for name, (fs, windows, orients) in roads.items():
        b = jl.OptimizeBatch().set_origin_policy("expand")
        if orients:
            b.set_orientations(orients)
        if windows:
            b.set_windows(windows)
        batches[name] = b.upload(fs, True).run()  # (warm: buffers allocated, code objects loaded)
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
    out = {"metric": "ms per step, optimizer with and without the lossless window", "images": n, "dri": args.dri, "steps": args.steps}
    for name, (fs, windows, _) in roads.items():
        b = batches[name]
        row = {"files": len(fs), "ms_per_step": round(mean(wall[name]), 3), "device_ms": round(mean(dev[name]), 3),
               "output_MB": round(sum(b.result(i)[1] for i in range(len(fs))) / 1e6, 2)}
        if windows:
            kx, decode, dense = (mean([s[j] for s in stages[name]]) for j in range(3))
            row.update({"applied_window_0": list(b.window(0)), "turn_sources": b.turn_sources(), "kx_ms": round(kx, 4), "entropy_decode_ms": round(decode, 3),
                        "dense_copy_ms": round(dense, 3)})
            if len(fs) == n:
                row["ratio_to_plain"] = round(mean(wall[name]) / mean(wall["plain"]), 3)
        out[name] = row
    print(json.dumps(out))
    for b in batches.values():
        b.close()


if __name__ == "__main__":
    main()
