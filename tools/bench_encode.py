#!/usr/bin/env python3
"""tools/bench_encode.py -- Mpixels/s of the GPU encoder on synthetic 4K RGB images, next to the oracle
restatement on the host cores.  Not the headline benchmark (that is bench.py); prints one JSON line.

    python tools/bench_encode.py [--images 64] [--steps 5] [--width 3840 --height 2160] [--quality 75]
    python tools/bench_encode.py --workload het_8192 [--subsampling 420|444] [--optimize-coding] [--images 8]
    python tools/bench_encode.py --arrangement cmyk|420-split [--optimize-coding]
    python tools/bench_encode.py --input device|device_planar [--images 64]

--input host (the default) is the run described below.  --input device / device_planar: ONE process encodes the same images three ways --
numpy arrays through upload() (host), torch (H, W, 3) tensors through upload_tensors(layout='hwc') (device) and torch (3, H, W) tensors
through upload_tensors(layout='chw') (device_planar) -- with the UPLOAD INSIDE the timed step (for the device inputs it copies nothing),
and reports ms_per_step and stage_ms of each; `value` is the named input's rate.

--arrangement = a described image (jpgpu_encode_description) that is no EncodeAction arrangement, so the general kernels take it:
cmyk = four 1 x 1 components (four samples per pixel); 420-split = 2 x 2 / 1 x 1 / 1 x 1 from RGB pixels like the default run, but
with three quantisation tables and Huffman tables of its own per component -- the headline shape forced onto the general path.

--workload het_8192 = the reference's OWN encoder benchmark (tests/JpegLibrary.Benchmarks/EncoderBenchmark.cs:21-58, 77-135): the
8192 x 8192 canvas of HETissueSlide.jpg (drawn 2 x 2 into the top-left quarter, the rest black), decoded to Rgba32 pixels, encoded
as baseline Q75 with the standard tables, 4:4:4 or 4:2:0.  The reference times ConvertRgba32ToYCbCr8 + Encode of ONE image per
call; here: the same Rgba32 pixels in (input_rgb = 2: four bytes per pixel, the alpha byte stepped over), the colour conversion
fused into E1, a batch of canvases per call AND one canvas per call (`latency`).  --pixels rgb: three-byte pixels instead.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def image(w, h, seed):
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, 4)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([128 + 70 * np.sin(x / 37 + ph[0]) * np.cos(y / 53 + ph[1]), 128 + 60 * np.cos(x / 91 + y / 29 + ph[2]),
                    128 + 90 * np.sin((x + y) / 67 + ph[3])], axis=-1)
    img += rng.normal(0, 8, img.shape).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def described_arrangement(jl, name, w, h, quality, optimize_coding):
    from jpeglibrary_amd.encoder import describe

    sq, sh = jl.JpegStandardQuantizationTable, jl.JpegStandardHuffmanEncodingTable
    lum = sq.ScaleByQuality(sq.GetLuminanceTable(0, 0), quality).Elements
    chrom = sq.ScaleByQuality(sq.GetChrominanceTable(0, 1), quality).Elements
    codes = lambda t: None if optimize_coding else [(c.Symbol, c.Code, c.CodeLength) for c in t._codes]
    dc_l, ac_l, dc_c, ac_c = (codes(t) for t in (sh.GetLuminanceDCTable(), sh.GetLuminanceACTable(), sh.GetChrominanceDCTable(), sh.GetChrominanceACTable()))
    if name == "cmyk":
        comps = [(k + 1, 1, 1, t, t, t, (lum, chrom)[t]) for k, t in enumerate((0, 1, 1, 0))]
        return describe(w, h, comps, [(0, lum), (1, chrom)], [(0, 0, dc_l), (1, 0, ac_l), (0, 1, dc_c), (1, 1, ac_c)])
    comps = [(1, 2, 2, 0, 0, 0, lum), (2, 1, 1, 1, 1, 1, chrom), (3, 1, 1, 2, 2, 2, chrom)]
    return describe(w, h, comps, [(0, lum), (1, chrom), (2, chrom)], [(0, 0, dc_l), (1, 0, ac_l), (0, 1, dc_c), (1, 1, ac_c), (0, 2, dc_c), (1, 2, ac_c)],
                    input_rgb=1)


def bench_arrangement(jl, args):
    distinct = min(args.images, 16)
    with ThreadPoolExecutor(16) as ex:
        base = list(ex.map(lambda s: image(args.width, args.height, s), range(distinct)))
    if args.arrangement == "cmyk":  # a fourth sample per pixel
        base = [np.ascontiguousarray(np.concatenate([im, 255 - im[..., :1]], axis=-1)) for im in base]
    imgs = [base[i % distinct] for i in range(args.images)]
    desc = described_arrangement(jl, args.arrangement, args.width, args.height, args.quality, args.optimize_coding)
    desc.restart_interval = args.dri
    b = jl.EncodeBatch().upload_described(imgs, [desc] * args.images)
    b.encode()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        b.encode()
    dt = (time.perf_counter() - t0) / args.steps
    px = args.images * args.width * args.height
    print(json.dumps({"metric": f"Mpixels/s encoded (described arrangement {args.arrangement}, general kernels, {'built' if args.optimize_coding else 'given'} tables)",
                      "value": round(px / dt / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(dt * 1e3, 2), "images": args.images,
                      "arrangement": args.arrangement, "restart_interval": args.dri, "bytes_per_image": len(b.output(0)),
                      "stage_ms": {k: round(v, 3) for k, v in b.stage_ms().items()}}))


def bench_inputs(jl, po, args, base, imgs, luma):
    """host, device and device_planar over the same images in one process: upload + encode per step"""
    import torch

    dev = torch.device("cuda", jl.default_context().device)
    hwc = [torch.from_numpy(im).to(dev) for im in base]
    chw = [t.permute(2, 0, 1).contiguous() for t in hwc]
    torch.cuda.synchronize(dev)
    kw = dict(restart_interval=args.dri, optimize_coding=args.optimize_coding)
    forms = {"host": lambda b: b.upload(imgs, luma, args.quality, rgb=True, **kw),
             "device": lambda b: b.upload_tensors([hwc[i % len(hwc)] for i in range(args.images)], luma, args.quality, rgb=True, layout="hwc", **kw),
             "device_planar": lambda b: b.upload_tensors([chw[i % len(chw)] for i in range(args.images)], luma, args.quality, rgb=True, layout="chw", **kw)}
    ref = po.encode_8bit(po.rgb_to_ycbcr8(imgs[0]), luma[0], luma[1], args.quality, restart_interval=args.dri, optimize_coding=args.optimize_coding)
    px = args.images * args.width * args.height
    inputs = {}
    for name, upload in forms.items():
        b = jl.EncodeBatch()
        upload(b).encode()
        upload(b).encode()  # (the second encode of a batch sizes its one-pass buffer from the first)
        fdct, t0 = [], time.perf_counter()
        for _ in range(args.steps):
            upload(b).encode()
            fdct.append(b.stage_ms()["fdct_quant"])
        dt = (time.perf_counter() - t0) / args.steps
        inputs[name] = {"ms_per_step": round(dt * 1e3, 2), "mpixels_per_s": round(px / dt / 1e6, 1), "stage_ms": {k: round(v, 3) for k, v in b.stage_ms().items()},
                        "fdct_quant_ms_median": round(float(np.median(fdct)), 3), "fdct_quant_ms_min": round(float(min(fdct)), 3),
                        "byte_exact_vs_oracle": b.output(0) == ref}
        b.close()
    f = {k: v["fdct_quant_ms_median"] for k, v in inputs.items()}
    print(json.dumps({"metric": f"Mpixels/s encoded, upload inside the step (RGB 4:{args.subsampling[1]}:{args.subsampling[2]} baseline, input {args.input})",
                      "value": inputs[args.input]["mpixels_per_s"], "unit": "Mpixels/s", "ms_per_step": inputs[args.input]["ms_per_step"], "images": args.images,
                      "steps": args.steps, "width": args.width, "height": args.height, "input": args.input, "inputs": inputs,
                      "fdct_quant_ratio": {"device_over_host": round(f["device"] / f["host"], 4), "planar_over_interleaved": round(f["device_planar"] / f["device"], 4)}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--dri", type=int, default=0, help="restart interval in MCUs (0 = none, the reference encoder's only mode)")
    ap.add_argument("--workload", default="synthetic_4k", choices=["synthetic_4k", "het_8192"])
    ap.add_argument("--subsampling", default="420", choices=["420", "444"])
    ap.add_argument("--optimize-coding", action="store_true", help="Huffman tables from each image's own statistics (EncodeAction's switch)")
    ap.add_argument("--pixels", default=None, choices=["rgb", "rgba"], help="input pixels (default: rgba for het_8192 like the reference's benchmark, rgb otherwise)")
    ap.add_argument("--arrangement", default=None, choices=["cmyk", "420-split"], help="a described image the general kernels take (see above)")
    ap.add_argument("--input", default="host", choices=["host", "device", "device_planar"],
                    help="where the pixels are: numpy arrays (host), or torch tensors on the device, (H, W, 3) / (3, H, W); see above")
    args = ap.parse_args()
    import jpeglibrary_amd as jl

    if args.arrangement:
        return bench_arrangement(jl, args)
    from oracle import pyoracle as po

    luma = (2, 2) if args.subsampling == "420" else (1, 1)
    het = args.workload == "het_8192"
    if het:
        import bench

        args.width = args.height = 8192
        if args.images == 64:
            args.images = 8
        rgba = jl.decode_batch([bench.het_canvas(75)], jl.FMT_RGBA_U8)[0][0]  # EncoderBenchmark.Setup: decode + ConvertYCbCr8ToRgba32
        base = [np.ascontiguousarray(rgba)]
        distinct = 1
    else:
        distinct = min(args.images, 16)
        with ThreadPoolExecutor(16) as ex:
            base = list(ex.map(lambda s: image(args.width, args.height, s), range(distinct)))
    pixels = args.pixels or ("rgba" if het else "rgb")
    if pixels == "rgba" and base[0].shape[2] == 3:
        base = [np.ascontiguousarray(np.concatenate([im, np.full(im.shape[:2] + (1,), 255, np.uint8)], axis=-1)) for im in base]
    elif pixels == "rgb" and base[0].shape[2] == 4:
        base = [np.ascontiguousarray(im[..., :3]) for im in base]
    bpp = 4 if pixels == "rgba" else 3
    to_ycc = po.rgba_to_ycbcr8 if pixels == "rgba" else po.rgb_to_ycbcr8
    imgs = [base[i % distinct] for i in range(args.images)]
    if args.input != "host":
        if bpp != 3:
            ap.error("--input device / device_planar compare three-byte pixels: --pixels rgb")
        return bench_inputs(jl, po, args, base, imgs, luma)
    b = jl.EncodeBatch().upload(imgs, luma, args.quality, rgb=True, restart_interval=args.dri, optimize_coding=args.optimize_coding)
    b.encode()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        b.encode()
    dt = (time.perf_counter() - t0) / args.steps
    px = args.images * args.width * args.height
    stage = b.stage_ms()
    out0 = b.output(0)
    ref = po.encode_8bit(to_ycc(imgs[0]), luma[0], luma[1], args.quality, restart_interval=args.dri, optimize_coding=args.optimize_coding)
    latency = None
    if het:  # the reference encodes ONE image per call
        one = jl.EncodeBatch().upload(imgs[:1], luma, args.quality, rgb=True, optimize_coding=args.optimize_coding)
        one.encode()
        t1 = time.perf_counter()
        for _ in range(5):
            one.encode()
        latency = {"encode_ms": round((time.perf_counter() - t1) / 5 * 1e3, 3), "stage_ms": {k: round(v, 3) for k, v in one.stage_ms().items()},
                   "note": "one canvas per call, pixels resident in HBM, the finished stream left in HBM"}
        one.close()
    # ---- CPU baseline: the restatement (oracle/jpegenc.c through ctypes: the C call releases the GIL, so these ARE native threads),
    # one encoder per thread on the CPUs the process is granted; a bounded sample
    from bench import granted_cpus, host_cpu_budget
    budget = host_cpu_budget()
    cores = granted_cpus(budget)
    ycc = [to_ycc(im) for im in base[:min(distinct, 4)]]
    t1 = time.perf_counter()
    po.encode_8bit(ycc[0], luma[0], luma[1], args.quality, optimize_coding=args.optimize_coding)
    single = args.width * args.height / (time.perf_counter() - t1) / 1e6
    n_cpu = cores * (1 if het else 2)
    t1 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        list(ex.map(lambda k: po.encode_8bit(ycc[k % len(ycc)], luma[0], luma[1], args.quality, optimize_coding=args.optimize_coding), range(n_cpu)))
    cpu_dt = time.perf_counter() - t1
    cpu = n_cpu * args.width * args.height / cpu_dt / 1e6
    # ---- roofline of the dominant kernel (HBM: no contraction on this path).  Algorithmic bytes per stage: E1 reads the pixels
    # and writes the int16 zig-zag blocks; E2 and E3 read the blocks (E3 also writes the raw stream); E4 reads the raw stream
    # and writes the finished one.
    n_blocks = sum(b._blocks)
    out_bytes = sum(len(b.output(i)) for i in range(min(args.images, distinct))) / min(args.images, distinct) * args.images
    algo = {"fdct_quant": px * bpp + n_blocks * 128, "block_bits": n_blocks * 128 + n_blocks * 4, "emit": n_blocks * 128 + out_bytes, "stuff": 2 * out_bytes}
    one_pass = b.emit_passes()[0] > 0 and stage["emit"] < 0.05  # E2 + E3 ran as bits_emit_kernel (its time is under "block_bits")
    if one_pass:
        algo["block_bits"] = n_blocks * 128 + out_bytes
    dom = max(("fdct_quant", "block_bits", "emit", "stuff"), key=lambda k: stage[k])
    achieved = algo[dom] / (stage[dom] / 1e3) / 1e9
    metric = (f"Mpixels/s encoded (the reference's EncoderBenchmark canvas: 8192 x 8192 {'Rgba32' if bpp == 4 else 'RGB'}, 4:{args.subsampling[1]}:{args.subsampling[2]} baseline Q75, "
              f"{'optimised' if args.optimize_coding else 'standard'} tables)" if het else
              f"Mpixels/s encoded ({'Rgba32' if bpp == 4 else 'RGB'} 4:{args.subsampling[1]}:{args.subsampling[2]} baseline, {'optimised' if args.optimize_coding else 'standard'} tables)")
    print(json.dumps({"metric": metric, **({"latency": latency} if latency else {}), "value": round(px / dt / 1e6, 1), "unit": "Mpixels/s",
                      "ms_per_step": round(dt * 1e3, 2), "images": args.images, "bytes_per_pixel_in": bpp, "restart_interval": args.dri, "bytes_per_image": len(out0), "entropy_stage": "one pass (bits_emit_kernel; stage_ms.block_bits)" if one_pass else "two kernels (block_bits_kernel, emit_kernel)",
                      "byte_exact_vs_oracle": out0 == ref, "stage_ms": {k: round(v, 3) for k, v in stage.items()},
                      "roofline": {"kernel": {"fdct_quant": "enc_gather_kernel + fdct_quant_kernel" if os.environ.get("JPGPU_ENC_NO_FUSED") else "fdct_fused_kernel", "block_bits": "bits_emit_kernel" if one_pass else "block_bits_kernel", "emit": "emit_kernel",
                                              "stuff": "stuff_count_kernel + stuff_write_kernel"}[dom], "bound": "hbm", "achieved": round(achieved, 1),
                                   "peak": 8000.0, "unit": "GB/s", "frac": round(achieved / 8000.0, 4), "algorithmic_bytes": int(algo[dom]), "traffic": None,
                                   "note": "stage time by HIP events on the library's stream; E1 (fdct_fused_kernel) is VALU bound: ~76 % of the SIMD cycles issue a vector instruction (tools/trace/encoder_pmc.sh)"},
                      "cpu_baseline": {"value": round(cpu, 1), "unit": "Mpixels/s", "cores": cores, "kind": "port",
                                       "sample": f"{n_cpu} encodes of {len(ycc)} of the images (YCbCr8 in, the colour conversion not timed), one encoder per native thread ({cpu_dt:.1f} s wall); single thread {single:.1f} Mpixels/s",
                                       "host_cpu_budget": budget, "gpu_over_cpu": round(px / dt / 1e6 / cpu, 1)}}))


if __name__ == "__main__":
    main()
