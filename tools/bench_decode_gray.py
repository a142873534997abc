"""What mode="gray" costs and saves against the three-plane decode and against PLANAR_U8, today's only other source of the luma samples
(recorded in RESULTS.md; a first measurement with one condition).

    python tools/bench_decode_gray.py [--images 256] [--reps 10] [--warmup 2]

Two corpora of `--images` 4:2:0 files at Q75 (the headline benchmark's recipe): 3840 x 2160, which K3 serves from its 4:2:0 fast class, and
1366 x 768, whose width is no multiple of 8 and which K3 serves from the byte-store generic class.  ONE process; per corpus and repetition, in
the order A B C A B C:
  A  decode_to_tensors(files): uint8 [3, H, W] tensors, K3;
  B  decode_to_tensors(files, mode="gray"): uint8 [1, H, W] tensors, K3Y's fast road -- no chroma block is read or transformed;
  C  a FMT_PLANAR_U8 decode of the same files: the luma samples as an MCU-padded plane beside the two chroma planes.
A step is timed with the host's clock from before the call to behind a synchronise of the device; all include the upload.  Before any timing
B is compared with plane 0 of C (the luma samples; they must be equal).  Behind each step round, A B A B, one decode() of three resident
batches gives stage_ms()["idct"], the device time of the whole output stage of each route, and stage_ms()["huffman"] (a grey image's scan is
always handed over dense).  Medians over reps behind `--warmup` rounds.
  The condition: the output stage of B is shorter than that of A in EVERY pair of the A B A B run (it moves half the bytes of a 4:2:0 MCU;
a ratio of 1 or more is a defect, not noise).  One JSON line per corpus on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeglibrary_amd as jl  # noqa: E402
from tools import jpegsynth  # noqa: E402


def corpus(n, W, H, seed0):
    buf, sizes, stride = jpegsynth.encode_batch(n, W, H, "420", 75, 0, seed0=seed0, nthreads=min(16, os.cpu_count() or 1))
    return [bytes(buf[i * stride:i * stride + int(sizes[i])]) for i in range(n)]


def measure(torch, dev, files, W, H, reps, warmup):
    n = len(files)

    def step(**kw):
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files, **kw)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, tensors

    def step_c():
        t0 = time.perf_counter()
        b = jl.Batch().upload(files, jl.FMT_PLANAR_U8).decode().sync()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, b

    (_, xa), (_, xb), (_, bc) = step(), step(mode="gray"), step_c()
    assert len(xa) == len(xb) == n and all(a is not None and tuple(a.shape) == (3, H, W) for a in xa) and all(b is not None and tuple(b.shape) == (1, H, W) for b in xb)
    for i in range(0, n, max(1, n // 8)):  # the grey plane is the luma plane of the native decode
        assert np.array_equal(xb[i][0].cpu().numpy(), bc.output(i)[0][:H, :W]), i
    bc.close()
    del xa, xb
    res = {"rgb": jl.Batch().upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync(),
           "gray": jl.Batch().set_channels_policy("gray").upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync(),
           "planar": jl.Batch().upload(files, jl.FMT_PLANAR_U8).decode().sync()}
    assert res["gray"].luma_work() == (n, 0) and res["gray"].plan_stats()["idct_listed_mcus"] == 0  # every image on K3Y's fast road, none in K3's lists
    work_rgb = res["rgb"].plan_stats()["idct_work"]
    for r in res.values():
        r.stage_ms()  # (drops the first decode's events)

    def stage(name):
        res[name].decode().sync()
        return res[name].stage_ms()

    for _ in range(warmup):
        step()
        step(mode="gray")
        step_c()[1].close()
        for name in res:
            stage(name)
    series = {k: [] for k in ("A1", "B1", "C1", "A2", "B2", "C2", "out_rgb1", "out_gray1", "out_rgb2", "out_gray2", "out_planar", "huffman_rgb", "huffman_gray")}
    for _ in range(reps):
        for name, kw in (("A1", {}), ("B1", {"mode": "gray"}), ("C1", None), ("A2", {}), ("B2", {"mode": "gray"}), ("C2", None)):
            if kw is None:
                ms, b = step_c()
                b.close()
            else:
                ms, out = step(**kw)
                del out
            series[name].append(ms)
        for k in ("1", "2"):  # A B A B on the resident batches
            sa, sb = stage("rgb"), stage("gray")
            series["out_rgb" + k].append(sa["idct"])
            series["out_gray" + k].append(sb["idct"])
            if k == "1":
                series["huffman_rgb"].append(sa["huffman"])
                series["huffman_gray"].append(sb["huffman"])
        series["out_planar"].append(stage("planar")["idct"])
    pairs = [g / a for k in ("1", "2") for a, g in zip(series["out_rgb" + k], series["out_gray" + k])]
    assert max(pairs) < 1.0, ("the grey output stage is not shorter than the three-plane one in every pair", pairs)  # the one condition
    med = {name: float(np.median(v)) for name, v in series.items()}
    a_med, b_med, c_med = (float(np.median(series[x + "1"] + series[x + "2"])) for x in "ABC")
    out_rgb, out_gray = (float(np.median(series["out_" + x + "1"] + series["out_" + x + "2"])) for x in ("rgb", "gray"))
    blocks = n * ((W + 15) // 16) * ((H + 15) // 16)
    gray_bytes = blocks * 4 * 128 + n * W * H  # four coefficient blocks of every MCU read, one byte per pixel written
    for r in res.values():
        r.close()
    return {"what": "decode_gray_ms", "images": n, "width": W, "height": H, "reps": reps, "compressed_bytes": sum(map(len, files)),
            "k3_idct_work_by_class_rgb": work_rgb,
            "A_rgb_planar_step_median_ms": a_med, "B_gray_step_median_ms": b_med, "C_planar_u8_step_median_ms": c_med,
            "B_over_A_step": b_med / a_med, "B_over_C_step": b_med / c_med, "spread_A2_over_A1": med["A2"] / med["A1"], "spread_B2_over_B1": med["B2"] / med["B1"],
            "output_stage_rgb_planar_ms": out_rgb, "output_stage_gray_ms": out_gray, "output_stage_planar_u8_ms": med["out_planar"],
            "gray_over_rgb_output_stage": out_gray / out_rgb, "gray_over_planar_u8_output_stage": out_gray / med["out_planar"],
            "gray_over_rgb_output_stage_pairs_min_max": [min(pairs), max(pairs)],
            "huffman_stage_rgb_ms": med["huffman_rgb"], "huffman_stage_gray_dense_handoff_ms": med["huffman_gray"],
            "gray_bytes": gray_bytes, "gray_output_stage_tb_per_s": gray_bytes / (out_gray * 1e-3) / 1e12,
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
