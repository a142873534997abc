"""What upsampling="fancy" costs a torch consumer, and what it buys (recorded in RESULTS.md, no test gate on the times; a first measurement).

    python tools/bench_decode_upsample.py [--images 256] [--reps 10] [--warmup 2] [--width 3840] [--height 2160] [--pillow-images 16]

`--images` 4:2:0 files of 3840 x 2160 at Q75 (the headline benchmark's recipe).  ONE process; per repetition, in the order A B C A B C:
  A  decode_to_tensors(files): uint8 [3, H, W] tensors with replicated chroma, through K3's fast class;
  B  decode_to_tensors(files, upsampling="fancy"): the same with libjpeg's triangle filter, through K3's generic class and the one K3U call;
  C  what a caller can do without the feature: a native-plane decode (FMT_PLANAR_U8: Y at full size, Cb and Cr as stored) and the same filter
     and the same integer colour conversion written in torch, image by image.
A step is timed with the host's clock from before the call to behind a synchronise of the device; all include the upload.  Before any timing
B and C are compared (they must be equal) and A must differ from them.  Behind each round one decode() of two resident batches gives
stage_ms()["idct"] of the replicated route (K3's fast class) and of the filtered one (K3's generic class + K3U), and Batch.upsampling_ms() gives
K3U alone, from an event pair of its own (JPGPU_TIME_UPSAMPLE=1); `k3u_bytes` is what it moves, 3 bytes read and 3 written per pixel.  Medians
over reps behind `--warmup` rounds.
  Against Pillow (libjpeg-turbo's integer IDCT, fancy upsampling and fixed-point colour conversion) on the first --pillow-images files: the
mean and the largest absolute difference of the RGB samples under both policies -- a finding -- and one condition: the mean under "fancy" is
the smaller one.  One JSON line on stdout."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["JPGPU_TIME_UPSAMPLE"] = "1"  # (read at every upload of this process: the event pair around K3U)

import jpeglibrary_amd as jl  # noqa: E402
from tools import jpegsynth  # noqa: E402


def ycc_rgb_factors():
    """the reference converter's 16.16 factors, derived in float32 as its Init derives them"""
    f = np.float32
    fix = lambda x: int(float(f(x) * f(1 << 16)) + 0.5)  # noqa: E731
    red, green, blue = f(299) / f(1000), f(587) / f(1000), f(114) / f(1000)
    f1 = f(2) - f(2) * red
    f3 = f(2) - f(2) * blue
    return fix(f1), -fix(red * f1 / green), fix(f3), -fix(blue * f3 / green)  # cr_r, cr_g, cb_b, cb_g


def torch_fancy_rgb(torch, planes, W, H, idx, k):
    """(Y, Cb, Cr) native planes of a 4:2:0 image (torch uint8, MCU-padded) -> uint8 [3, H, W]: the h2v2 triangle filter and the integer conversion"""
    y, cb, cr = planes
    jn, jf, rn, in_, if_, xb = idx
    ch, cw = (H + 1) // 2, (W + 1) // 2
    out = []
    for c in (cb, cr):
        c = c[:ch, :cw].to(torch.int32)
        s = 3 * c[jn] + c[jf]
        out.append(((3 * s[:, in_] + s[:, if_] + xb) >> 4) - 128)
    cbv, crv = out
    yv = y[:H, :W].to(torch.int32)
    cr_r, cr_g, cb_b, cb_g = k
    r = yv + ((cr_r * crv + 32768) >> 16)
    g = yv + ((cb_g * cbv + 32768 + cr_g * crv) >> 16)
    b = yv + ((cb_b * cbv + 32768) >> 16)
    return torch.stack([r, g, b]).clamp_(0, 255).to(torch.uint8)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--pillow-images", type=int, default=16)
    args = ap.parse_args()
    W, H = args.width, args.height
    buf, sizes, stride = jpegsynth.encode_batch(args.images, W, H, "420", 75, 0, seed0=20261020, nthreads=min(16, os.cpu_count() or 1))
    files = [bytes(buf[i * stride:i * stride + int(sizes[i])]) for i in range(args.images)]
    n = len(files)
    dev = torch.device("cuda", jl.default_context().device)
    k = ycc_rgb_factors()
    ch, cw = (H + 1) // 2, (W + 1) // 2
    ys, xs = torch.arange(H, device=dev), torch.arange(W, device=dev)
    jn, in_ = ys >> 1, xs >> 1
    jf = torch.where(ys % 2 == 0, jn - 1, jn + 1).clamp_(0, ch - 1)
    if_ = torch.where(xs % 2 == 0, in_ - 1, in_ + 1).clamp_(0, cw - 1)
    xb = torch.where(xs % 2 == 0, 8, 7).to(torch.int32)[None, :]
    idx = (jn, jf, None, in_, if_, xb)

    def step_a():
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, tensors

    def step_b():
        t0 = time.perf_counter()
        tensors, results = jl.decode_to_tensors(files, upsampling="fancy")
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, tensors

    def step_c():
        t0 = time.perf_counter()
        b = jl.Batch().upload(files, jl.FMT_PLANAR_U8).decode().sync()
        base, _ = b.output_device_ptr()
        out = []
        for i in range(n):
            info = b.image_info(i)
            planes = [torch.as_tensor(jl.batch._DeviceView(b, base + info.out_offset + info.plane[c].offset, (info.plane[c].height, info.plane[c].pitch)), device=dev)
                      for c in range(3)]
            out.append(torch_fancy_rgb(torch, planes, W, H, idx, k))
        torch.cuda.synchronize(dev)
        b.close()
        return (time.perf_counter() - t0) * 1e3, out

    (_, xa), (_, xb_), (_, xc) = step_a(), step_b(), step_c()
    assert len(xa) == len(xb_) == len(xc) == n and all(b is not None and tuple(b.shape) == (3, H, W) and torch.equal(b, c) for b, c in zip(xb_, xc))
    assert not torch.equal(xa[0], xb_[0])
    # ---- against Pillow, on the host
    from PIL import Image

    diffs = {"replicate": [], "fancy": []}
    for i in range(min(args.pillow_images, n)):
        ref = np.asarray(Image.open(io.BytesIO(files[i])).convert("RGB")).astype(np.int16).transpose(2, 0, 1)
        for name, x in (("replicate", xa[i]), ("fancy", xb_[i])):
            d = np.abs(x.cpu().numpy().astype(np.int16) - ref)
            diffs[name].append((float(d.mean()), int(d.max())))
    pillow = {name: {"mean_abs": float(np.mean([m for m, _ in v])), "max_abs": max(x for _, x in v)} for name, v in diffs.items() if v}
    if pillow:
        assert pillow["fancy"]["mean_abs"] < pillow["replicate"]["mean_abs"], pillow  # the one condition
    del xa, xb_, xc
    res_a = jl.Batch().upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    res_b = jl.Batch().set_upsampling_policy("fancy").upload(files, jl.FMT_RGB_PLANAR_U8).decode().sync()
    work_a, work_b = res_a.plan_stats()["idct_work"], res_b.plan_stats()["idct_work"]
    assert work_b[0] > 0 and sum(work_b[1:]) == 0 and work_a[0] == 0, (work_a, work_b)  # the generic class against the fast one
    assert all(res_b.upsampling(i) == 1 and res_a.upsampling(i) == 0 for i in range(n))
    for r in (res_a, res_b):
        r.stage_ms()  # (drops the first decode's events)

    def stages():
        out = []
        for r in (res_a, res_b):
            r.decode().sync()
            out.append(r.stage_ms())
        return out + [res_b.upsampling_ms()]

    for _ in range(args.warmup):
        step_a()
        step_b()
        step_c()
        stages()
    series = {"A1": [], "B1": [], "C1": [], "A2": [], "B2": [], "C2": [], "idct_replicate": [], "idct_fancy": [], "huffman_replicate": [], "huffman_fancy": [], "k3u": []}
    for _ in range(args.reps):
        for name, step in (("A1", step_a), ("B1", step_b), ("C1", step_c), ("A2", step_a), ("B2", step_b), ("C2", step_c)):
            ms, out = step()
            series[name].append(ms)
            del out
        ka, kb, k3u = stages()
        series["idct_replicate"].append(ka["idct"])
        series["idct_fancy"].append(kb["idct"])
        series["huffman_replicate"].append(ka["huffman"])
        series["huffman_fancy"].append(kb["huffman"])
        series["k3u"].append(k3u)
    med = {name: float(np.median(v)) for name, v in series.items()}
    a_med, b_med, c_med = (float(np.median(series[x + "1"] + series[x + "2"])) for x in "ABC")
    k3u_bytes = n * W * H * 6
    print(json.dumps({"what": "decode_upsample_step_ms", "images": n, "width": W, "height": H, "reps": args.reps, "compressed_bytes": sum(map(len, files)),
                      "A_replicate_median_ms": a_med, "B_fancy_median_ms": b_med, "C_native_planes_then_torch_median_ms": c_med,
                      "B_over_A": b_med / a_med, "B_over_C": b_med / c_med, "spread_A2_over_A1": med["A2"] / med["A1"], "spread_B2_over_B1": med["B2"] / med["B1"],
                      "idct_stage_fast_class_ms": med["idct_replicate"], "idct_stage_generic_plus_k3u_ms": med["idct_fancy"],
                      "huffman_stage_replicate_ms": med["huffman_replicate"], "huffman_stage_fancy_dense_handoff_ms": med["huffman_fancy"],
                      "k3u_ms": med["k3u"], "k3u_bytes": k3u_bytes, "k3u_tb_per_s": k3u_bytes / (med["k3u"] * 1e-3) / 1e12,
                      "pillow_images": min(args.pillow_images, n), "vs_pillow_rgb": pillow,
                      "median_ms": med, "min_ms": {x: min(v) for x, v in series.items()}, "max_ms": {x: max(v) for x, v in series.items()},
                      "series_ms": {x: [round(y, 4) for y in v] for x, v in series.items()}}))


if __name__ == "__main__":
    main()
