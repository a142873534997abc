"""What INTERLEAVED_U8_SCALED costs in K3, and what the direct path of the decoder mirror saves (recorded in RESULTS.md, no test gate).

    python tools/bench_scaled_sink.py [--frames 256] [--reps 20] [--no-mirror]

1. K3 alone, frame hand-off: `--frames` frames of 3840 x 2160 4:2:0, one seeded coefficient set for all of them, in ONE process.
   Per repetition, in this order:  A  INTERLEAVED_U8 at P = 12 (code that the format did not change: the yardstick),
   B  INTERLEAVED_U8_SCALED at P = 12,  A again,  C  INTERLEAVED_U8_SCALED at P = 5.  Each figure is the host's clock around
   four run_idct() calls and one sync(), divided by four (Batch.stage_ms() has events for decode() only, and decode() would
   clear a handed-over frame's store): K3's kernels plus about a launch's latency, the same for every variant.
   The difference between the two A series is the spread of the measurement; B / A and C / A are read against it.
2. The mirror: one 3840 x 2160 4:2:0 P = 12 file per Decode() into JpegBufferOutputWriterGreaterThan8Bit -- the direct path
   (pixels from the device sink) against the same writer as a subclass, which keeps the per-block callback path.
One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeglibrary_amd as jl  # noqa: E402

W, H = 3840, 2160


def coefficient_set(seed):
    """blocks in MCU scan order of one 4:2:0 frame: sparse low-frequency coefficients of a photographic magnitude"""
    rng = np.random.default_rng(seed)
    n = (W // 16) * (H // 16) * 6
    z = np.zeros((n, 64), np.int16)
    z[:, 0] = rng.integers(-200, 200, n)
    keep = rng.random((n, 15)) < 0.4
    z[:, 1:16] = np.where(keep, rng.integers(-30, 31, (n, 15)), 0)
    return z


def resident(frames, precision, fmt, blocks):
    frame = {"width": W, "height": H, "precision": precision, "components": [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]}
    qt = np.stack([np.full(64, 8, np.uint16), np.full(64, 12, np.uint16), np.ones(64, np.uint16), np.ones(64, np.uint16)])
    b = jl.Batch().upload_frames([frame] * frames, np.stack([qt] * frames), fmt)
    for i in range(frames):
        b.set_coefficients(i, blocks)
    return b


def idct_ms(b, calls=4):
    b.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        b.run_idct()
    b.sync()
    return (time.perf_counter() - t0) * 1e3 / calls


def k3(frames, reps):
    blocks = coefficient_set(1)
    a = resident(frames, 12, jl.FMT_INTERLEAVED_U8, blocks)
    bb = resident(frames, 12, jl.FMT_INTERLEAVED_U8_SCALED, blocks)
    c = resident(frames, 5, jl.FMT_INTERLEAVED_U8_SCALED, blocks)
    for b in (a, bb, c, a, bb, c):  # warm-up
        idct_ms(b)
    series = {"A1": [], "B": [], "A2": [], "C": []}
    for _ in range(reps):
        for name, b in (("A1", a), ("B", bb), ("A2", a), ("C", c)):
            series[name].append(idct_ms(b))
    med = {k: float(np.median(v)) for k, v in series.items()}
    a_med = 0.5 * (med["A1"] + med["A2"])
    out_gb = frames * W * H * 3 / 1e9
    print(json.dumps({"what": "k3_idct_ms", "frames": frames, "reps": reps, "median_ms": med, "min_ms": {k: min(v) for k, v in series.items()},
                      "max_ms": {k: max(v) for k, v in series.items()}, "spread_A2_over_A1": med["A2"] / med["A1"], "B_over_A": med["B"] / a_med,
                      "C_over_A": med["C"] / a_med, "output_GBps_A": out_gb / (a_med * 1e-3), "series_ms": series}))


def file_4k_p12():
    """a 4K 4:2:0 file from the synthetic encoder, its frame header rewritten to SOF1 with P = 12 (the same entropy data: the
    samples sit around the 12-bit level shift)"""
    from tools import jpegsynth

    d = bytearray(jpegsynth.encode(W, H, "420", 75, 0, seed=5))
    k = d.index(b"\xff\xc0")
    d[k + 1], d[k + 4] = 0xC1, 12
    return bytes(d)


def mirror(reps):
    data = file_4k_p12()

    class ViaCallbacks(jl.JpegBufferOutputWriterGreaterThan8Bit):
        pass

    def once(cls):
        d = jl.JpegDecoder()
        d.SetInput(data)
        d.Identify()
        buf = np.zeros(d.Width * d.Height * 3, np.uint8)
        t0 = time.perf_counter()
        d.SetOutputWriter(cls(d.Width, d.Height, d.Precision, 3, buf))
        d.Decode()
        dt = time.perf_counter() - t0
        d.close()
        return dt * 1e3, buf

    once(jl.JpegBufferOutputWriterGreaterThan8Bit)
    direct = [once(jl.JpegBufferOutputWriterGreaterThan8Bit) for _ in range(reps)]
    cb_ms, cb_buf = once(ViaCallbacks)  # (seconds of Python per image: once)
    print(json.dumps({"what": "mirror_4k_p12_ms", "direct_median_ms": float(np.median([m for m, _ in direct])), "direct_min_ms": min(m for m, _ in direct),
                      "callback_path_ms": cb_ms, "same_bytes": bool(np.array_equal(direct[-1][1], cb_buf)), "file_bytes": len(data)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-mirror", action="store_true")
    args = ap.parse_args()
    k3(args.frames, args.reps)
    if not args.no_mirror:
        mirror(5)
