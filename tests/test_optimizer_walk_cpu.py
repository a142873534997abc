"""The optimizer's host walks without a device (csrc/optimize_walk.h: Scan()'s and Optimize(strip)'s marker walks, the late-failure rule, the
swallowed-terminator verdict), through the stand-alone harness tools/fuzz/optimizer_walk_asan.cpp built with AddressSanitizer + UBSan:
memory safety on corrupted and truncated files, and parity with the oracle's JpegOptimizer on the CPU."""
import glob
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from golden_util import read_jpeg
from oracle import pyoracle as po
from test_sanitizers_cpu import SAN, _edits
from tools import jpegsynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
KINDS = {1: "InvalidDataException", 2: "InvalidOperationException"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "walk_asan")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "jpeglibrary_amd", "csrc"), os.path.join(ROOT, "tools", "fuzz", "optimizer_walk_asan.cpp"),
                    os.path.join(ROOT, "jpeglibrary_amd", "csrc", "host_parser.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def _walk(exe, paths):
    """one parsed line per file; the harness must leave with 0 (a sanitizer report ends it with another status)"""
    lines = []
    for at in range(0, len(paths), 200):
        r = subprocess.run([exe, *paths[at:at + 200]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lines += [json.loads(line) for line in r.stdout.splitlines()]
    assert [line["file"] for line in lines] == list(paths)
    return lines


def _write(directory, files):
    paths = []
    for k, data in enumerate(files):
        p = directory / f"{k:04d}.jpg"
        p.write_bytes(data)
        paths.append(str(p))
    return paths


def test_the_walks_are_clean_under_asan_and_ubsan_on_corrupted_files(harness, tmp_path):
    """the corpus of test_sanitizers_cpu.corrupted (the same files, seed and edits)"""
    rng = np.random.default_rng(2024)
    files = []
    for name in ("cramps.jpg", "lake.jpg", "progress.jpg", "yellowcat_progressive_restart.jpg", os.path.join("stress", "progressive_band_overrun.jpg")):
        data = read_jpeg(name)
        if len(data) > 60000:
            data = data[:data.index(b"\xff\xda") + 30000] + b"\xff\xd9"
        files += _edits(data, rng, 60)
    lines = _walk(harness, _write(tmp_path, files))
    assert len(lines) == 300
    statuses = {run["status"] for line in lines for run in line["runs"]}
    assert 0 in statuses and 1 in statuses  # (a corpus that is all refused, or all accepted, would cover one side of the walks only)


def test_the_walks_are_clean_on_every_truncation_of_a_small_file(harness, tmp_path):
    data = jpegsynth.encode(48, 32, "420", 75, 4, seed=11)
    behind_sos_header = data.index(b"\xff\xda") + 2 + int.from_bytes(data[data.index(b"\xff\xda") + 2:][:2], "big")
    lines = _walk(harness, _write(tmp_path, [data[:n] for n in range(behind_sos_header + 2)]))
    assert lines[0]["runs"][0]["status"] == 2 and lines[0]["runs"][0]["error"] == "Input buffer is not specified."
    assert all(run["status"] != 0 or run["late_status"] != 0 or n >= behind_sos_header for n, line in enumerate(lines) for run in line["runs"])


def test_the_walks_are_clean_on_the_optimizer_stress_files(harness):
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stress", "optimizer_*")))
    assert len(paths) >= 3
    _walk(harness, paths)


def _parity_files():
    stress = lambda name: read_jpeg(os.path.join("stress", name))
    return {"lake": read_jpeg("lake.jpg"), "cramps": read_jpeg("cramps.jpg"), "progress": read_jpeg("progress.jpg"),
            "batch_201": stress("optimizer_batch_201.jpg"), "dht_176": stress("optimizer_dht_in_place_of_sof_176.jpg"),
            "dht_189": stress("optimizer_dht_in_place_of_sof_189.jpg"), "444_72x56": jpegsynth.encode(72, 56, "444", 75, 0, seed=1),
            "grey_88x64_dri3": jpegsynth.encode(88, 64, "gray", 75, 3, seed=2),
            "420_48x32_dri4": jpegsynth.encode(48, 32, "420", 75, 4, seed=3)}  # (3 x 2 MCUs: no multiple of 4)


def test_the_walks_agree_with_the_oracle(harness, tmp_path):
    """Where the oracle's Optimize() succeeds the walks report nothing, early or late, and the oracle's bytes start with the host bytes in
    front of the DHT piece and end with those behind the entropy piece; where a walk itself refuses (InvalidData / InvalidOperation) the
    oracle throws the same kind with the walk's message in its text.  (None of these files is refused with NOT_SUPPORTED.)"""
    files = _parity_files()
    lines = _walk(harness, _write(tmp_path, list(files.values())))
    good = refused = 0
    for (name, data), line in zip(files.items(), lines):
        for run in line["runs"]:
            strip = bool(run["strip"])
            assert run["status"] != 3 and run["late_status"] != 3, (name, run)
            try:
                ref = po.optimize(data, strip)
            except po.OracleError as e:
                ref = e
            if not isinstance(ref, po.OracleError):
                assert run["status"] == 0 and run["late_status"] == 0, (name, strip, run["error"], run["late_error"])
                pieces = run["pieces"]
                assert pieces.count("DHT") == 1 and pieces.count("ENTROPY") == 1 and pieces.index("DHT") < pieces.index("ENTROPY"), (name, pieces)
                head = bytes.fromhex("".join(pieces[:pieces.index("DHT")]))
                tail = bytes.fromhex("".join(pieces[pieces.index("ENTROPY") + 1:]))
                assert len(head) > 4 and ref.startswith(head), (name, strip)
                assert len(tail) >= 2 and ref.endswith(tail), (name, strip)
                good += 1
            if run["status"] in KINDS:
                assert isinstance(ref, po.OracleError) and ref.kind == KINDS[run["status"]] and run["error"] in ref.message, (name, strip, run["error"], str(ref))
                refused += 1
    assert good >= 8 and refused >= 2, (good, refused)
