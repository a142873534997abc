"""bench.py's own options: a plain run measures the headline and nothing else, --full adds the rest, --dump-outputs writes what
the timed path computed in its last step (the same inputs and the same sample from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Result:
    def __init__(self, status):
        self.status = status


class _FakeBatch:
    """What dump_outputs reads of a jl.Batch: per-image results and downloads (image 5 failed)."""

    def __init__(self, shape, planar=False):
        self.shape, self.planar = shape, planar

    def result(self, i):
        return _Result(3 if i == 5 else 0)

    def output(self, i):
        a = np.random.default_rng(i).integers(0, 256, self.shape).astype(np.uint8)
        return [a[..., 0], a[::2, ::2, 1]] if self.planar else a


@pytest.mark.parametrize("n,shape,planar", [(1024, (540, 960, 3), False), (3, (16, 16, 3), False), (40, (64, 64, 3), True)])
def test_dump_outputs_writes_float_arrays_within_budget_and_repeats(tmp_path, n, shape, planar):
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(_FakeBatch(shape, planar), n, str(d))
        arrays = {f: np.load(d / f) for f in sorted(os.listdir(d))}
        assert set(arrays) == {"status.npy", "sample_images.npy", "image_sums.npy", "pixels.npy"}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        runs.append(arrays)
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f], equal_nan=True), f
    a = runs[0]
    idx = a["sample_images.npy"].astype(int)
    assert len(a["status.npy"]) == n and len(idx) == min(n, bench.DUMP_IMAGES) and idx[0] == 0 and idx[-1] == n - 1
    batch = _FakeBatch(shape, planar)
    for row, i in enumerate(idx):
        if i == 5:  # a failed image has no output: its row is NaN
            assert np.isnan(a["image_sums.npy"][row]) and np.isnan(a["pixels.npy"][row]).all()
            continue
        o = batch.output(i)
        flat = np.concatenate([p.ravel() for p in o]) if planar else o.ravel()
        assert a["image_sums.npy"][row] == flat.sum(dtype=np.float64)
        assert np.isin(a["pixels.npy"][row], flat).all()
        if flat.size <= bench.DUMP_SAMPLES:
            assert np.array_equal(a["pixels.npy"][row], flat.astype(np.float32))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run's line holds the headline fields and none of --full's; its dump equals the checker's decode of the same
    synthetic inputs at the dumped positions, and a second run dumps the same arrays."""
    from jpeglibrary_amd import sharding
    from oracle import pyoracle as po
    from tools import jpegsynth

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "1080p_q90", "--images", "8", "--steps", "3",
                            "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        out = json.loads(lines[0])
        assert out["value"] > 0 and out["unit"] == "Mpixels/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["metric"].startswith("Mpixels/s decoded")
        for key in ("cpu_baseline", "value_ingest_inclusive", "parity_spot_check", "configs", "latency", "two_in_flight"):
            assert key not in out, key
        assert "read_frac_planar" not in out["roofline"] and "d2h_GBps" not in out["host"]
        runs.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f], equal_nan=True), f
    a = runs[0]
    assert (a["status.npy"] == 0).all() and len(a["status.npy"]) == 8
    width, height, ss, quality, dri, _ = bench.WORKLOADS["1080p_q90"]
    frac = np.sort(np.random.default_rng(bench.DUMP_SEED).random(bench.DUMP_SAMPLES))  # (8 images: all dumped, no draw of images first)
    assert a["sample_images.npy"].astype(int).tolist() == list(range(8))
    for i in range(8):
        ref = po.decode_8bit(bytes(jpegsynth.encode(width, height, ss, quality, dri, seed=sharding.rank_seed_base(0) + i)))[0].ravel()
        assert a["image_sums.npy"][i] == ref.sum(dtype=np.float64), i
        assert np.array_equal(a["pixels.npy"][i], ref[(frac * ref.size).astype(np.int64)].astype(np.float32)), i
