"""K3 stores the interleaved rows of 4:2:0 / 4:2:2 frames as whole 64-byte blocks per lane quad (jpeglibrary_amd/csrc/k3_store_quads.h):
in a tile whose quads are four MCUs side by side the lanes exchange 16-byte pieces in front of the stores, every other tile takes the same
loop with its own registers.  Everything here is compared bit for bit with the oracle, at the smallest shapes the corners occur at:

  lines of 16 * mpl pixels  mpl 4, 8: one short eligible tile; 5, 6: never eligible, the other leg of the same loop; 12: a tile wraps over
                            several lines at multiples of four MCUs; 44 (704 px): the second 40-MCU tile starts at column 40 and wraps after
                            one quad
  heights                   48 and 40 (4:2:0: whole MCUs and not -- the clipped bottom rows skip whole quads; 4:2:2's MCUs are 8 lines: 44 there),
                            96 and 88: more than 40 MCUs at mpl 12, a full and a short tile behind each other
  restart intervals         4 (the split kernel's slot order), 3 (its gather), 0 (dense, the subsequence decoder)
  hand-off                  every one of them with JPGPU_DENSE_HANDOFF=0 and =1, each setting in a child process of its own
  sinks                     INTERLEAVED_U8 and INTERLEAVED_U8_SCALED
  JPGPU_TILE_ALIGN=0        tiles of 42 MCUs: nothing eligible
  truncated files           a scan that ends inside a restart interval, decoded over the CALLER's canvas (JpegDecoder into a
                            JpegBufferOutputWriter8Bit: one device call per scan with kKeepUnreachedMcus set, device_batch_layout.cpp -- the
                            only path on which K3 clips a workgroup's range at the MCU the scan failed in, idct_output_body: `keep`; a
                            batch's own buffer gets zero samples through whole tiles instead).  704 px lines, tiles of 40 / 64 MCUs: the
                            tiles in front of the failing one are eligible, the clipped one has an MCU count that is no multiple of four.
                            That count is checked, not assumed: the same file through a batch reports the failing block
                            (result().error_block), and at least one cut per layout must leave whole-MCUs-reached % 4 != 0 behind a full
                            tile.  Against the oracle's partial decode (the whole one throws).

The files and the oracle's samples are made once, in the parent, and handed to the children as a file."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

MPLS = (4, 8, 5, 6, 12, 44)
HEIGHTS = {"420": (48, 40, 96, 88), "422": (48, 44, 96, 88)}
DRIS = (4, 3, 0)
SETTINGS = {"split": {"JPGPU_DENSE_HANDOFF": "0"}, "dense": {"JPGPU_DENSE_HANDOFF": "1"}, "unaligned_tiles": {"JPGPU_TILE_ALIGN": "0"}}


def _cases():
    """[(subsampling, width, height, dri, seed)]"""
    out = []
    for sub in ("420", "422"):
        for mpl in MPLS:
            for h in HEIGHTS[sub]:
                for dri in DRIS:
                    out.append((sub, 16 * mpl, h, dri, 700 + len(out)))
    return out


def _truncations(good):
    """the file cut inside its scan at three places, EOI kept: the scan ends in the middle of a restart interval"""
    sos = good.index(b"\xff\xda")
    start = sos + 2 + ((good[sos + 2] << 8) | good[sos + 3])
    return [good[:start + (len(good) - start) * k // 16] + b"\xff\xd9" for k in (6, 9, 13)]


_MADE = {}


def _made(tmp_path_factory):
    """the path of an .npz with every file, the oracle's samples of it and, for the truncated ones, the oracle's writer state"""
    if "path" not in _MADE:
        from oracle import pyoracle as po
        from tools import jpegsynth

        arrays = {}
        for i, (sub, w, h, dri, seed) in enumerate(_cases()):
            f = bytes(jpegsynth.encode(w, h, sub, 75, dri, seed=seed))
            arrays["file_%d" % i] = np.frombuffer(f, np.uint8)
            arrays["ref_%d" % i] = po.decode_8bit(f)[0]
        cut = []
        for sub in ("420", "422"):
            cut += _truncations(bytes(jpegsynth.encode(704, 48, sub, 75, 4, seed=690)))
        for i, f in enumerate(cut):
            px, _, err = po.decode_8bit_partial(f)
            assert err is not None, i  # (every cut makes the reference fail)
            arrays["cut_file_%d" % i] = np.frombuffer(f, np.uint8)
            arrays["cut_ref_%d" % i] = px
        path = str(tmp_path_factory.mktemp("k3_store_quads") / "made.npz")
        np.savez(path, **arrays)
        _MADE["path"] = path
    return _MADE["path"]


def _child(path):
    """decodes everything of the .npz under the environment the parent set; prints one line per difference and `DONE <files> <differences>`"""
    import jpeglibrary_amd as jl

    made = np.load(path)
    n = sum(1 for k in made.files if k.startswith("file_"))
    files = [made["file_%d" % i].tobytes() for i in range(n)]
    bad = 0
    for fmt in ("INTERLEAVED_U8", "INTERLEAVED_U8_SCALED"):  # (8-bit frames: the scaled sink's byte is the sample's clamp)
        b = jl.Batch().upload(files, getattr(jl, "FMT_" + fmt)).decode().sync()
        for i in range(n):
            want, res = made["ref_%d" % i], b.result(i)
            got = b.output(i)
            if (res.status, res.detail) != (0, 0) or got.shape != want.shape or not np.array_equal(got, want):
                bad += 1
                where = np.argwhere(got != want)[:4].tolist() if got.shape == want.shape else [got.shape, want.shape]
                print("DIFF", fmt, i, res.status, res.detail, where)
        b.close()
    n_cut = sum(1 for k in made.files if k.startswith("cut_file_"))
    # where the cut scans fail: whole MCUs in front of the failing block, from a batch's result (blocks per MCU: 6 in 4:2:0, 4 in 4:2:2; the
    # first three cuts are 4:2:0, tiles of 40 MCUs, the others 4:2:2, tiles of 64)
    cuts = [made["cut_file_%d" % i].tobytes() for i in range(n_cut)]
    b = jl.Batch().upload(cuts, jl.FMT_INTERLEAVED_U8).decode().sync()
    reached = [b.result(i).error_block // (6 if i < n_cut // 2 else 4) for i in range(n_cut)]
    b.close()
    print("REACHED", reached)
    for half, tile in ((reached[:n_cut // 2], 40), (reached[n_cut // 2:], 64)):
        if not any(r > tile and r % 4 != 0 for r in half):  # (the tiles are multiples of four MCUs)
            bad += 1
            print("DIFF cut: no clipped tile with an MCU count that is no multiple of four behind a full one", half)
    for i in range(n_cut):
        f, want = made["cut_file_%d" % i].tobytes(), made["cut_ref_%d" % i]
        d = jl.JpegDecoder()
        d.SetInput(f)
        d.Identify()
        out = np.zeros(d.Width * d.Height * 3, np.uint8)
        d.SetOutputWriter(jl.JpegBufferOutputWriter8Bit(d.Width, d.Height, 3, out))
        try:
            d.Decode()
            print("DIFF cut", i, "the decode did not fail")
            bad += 1
        except jl.JpegError:
            pass
        got = out.reshape(d.Height, d.Width, 3)
        if not np.array_equal(got, want):
            bad += 1
            print("DIFF cut", i, np.argwhere(got != want)[:4].tolist())
        d.close()
    print("DONE %d %d" % (2 * n + n_cut, bad))
    return bad


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_corner_of_the_quad_stores_is_bit_exact(setting, tmp_path_factory):
    path = _made(tmp_path_factory)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **SETTINGS[setting])
    for k in ("JPGPU_DENSE_HANDOFF", "JPGPU_TILE_ALIGN"):
        if k not in SETTINGS[setting]:
            env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    done = [ln for ln in r.stdout.splitlines() if ln.startswith("DONE ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    n_files, n_bad = (int(v) for v in done[0].split()[1:])
    assert n_bad == 0 and n_files == 2 * len(_cases()) + 6, r.stdout[-3000:]


if __name__ == "__main__":
    sys.exit(1 if _child(sys.argv[1]) else 0)
