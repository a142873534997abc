#!/usr/bin/env python3
"""tools/trace/k2_plain_mix.py [n_images] [steps] [warmup] -- K2's PLAIN kernel (huffman_decode_kernel) under load: the benchmark's
4K 4:2:0 Q75 files with every second one sent through the optimizer, so that no two neighbours stage the same tables.  Every file is
then a run of its own; the planner pools the first eight runs and leaves the rest on the plain list (bench.py's workloads are all from
one encoder and never get there).  DRI = 7, not the benchmark's 4: the optimizer, like the reference's, gives up on a restart interval
that divides the MCU count (32 400).  Prints one JSON line: the plan, the Huffman stage's device time and the time per decode."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import jpeglibrary_amd as jl
from tools import jpegsynth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
buf, sizes, stride = jpegsynth.encode_batch(n, 3840, 2160, "420", 75, 7, seed0=1000)
files = [bytes(buf[i * stride:i * stride + int(sizes[i])]) for i in range(n)]
optimized = jl.optimize_batch(files[1::2], strip=False)
files[1::2] = [bytes(f) for f in optimized]
b = jl.Batch().upload(files, jl.FMT_INTERLEAVED_U8)
for _ in range(warmup):
    b.decode()
b.sync()
assert all(b.result(i).status == 0 for i in range(n))
b.stage_ms()  # (drops the warm-up's events: the next call averages over the timed steps, as in bench.py)
t0 = time.perf_counter()
for _ in range(steps):
    b.decode()
b.sync()
ms_per_step = (time.perf_counter() - t0) * 1e3 / steps
stage = b.stage_ms()
st = b.plan_stats()
print(json.dumps({"workload": f"{n} x 3840x2160 420 Q75 DRI=7, tables alternating", "k2_plain_work": st["k2_plain_work"], "k2_pools": st["k2_pools"],
                  "k2_pooled_chunks": st["k2_pooled_chunks"], "steps": steps, "stage_ms": {k: round(v, 4) for k, v in stage.items()}, "ms_per_step": round(ms_per_step, 4)}))
