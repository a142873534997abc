"""The listing of the device-file ingest kernels (k0_device_files.hip), checked without a GPU: each compiles for gfx950 with no scratch
and no spills; the gather moves 16 bytes per lane and instruction on both sides, as global (not flat) accesses."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")
KERNELS = ["gather_device_kernel", "head_walk_kernel", "head_scan_kernel", "head_pack_kernel", "verdict_bytes_kernel"]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "k0_device_files.o" in makefile
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", makefile, re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "k0_device_files.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, "k0_device_files.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


def _mangled(text, kernel):
    (name,) = [n for n in re.findall(r"\.name:\s+(\S+)", text) if kernel in n]
    return name


def _body(text, name):
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(name) and ln.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i] or lines[i].startswith(".Lfunc_end"))
    return [ln.strip() for ln in lines[start:end] if ln.strip() and not ln.strip().startswith(";")]


def _resources(text, name):
    names = re.findall(r"\.name:\s+(\S+)", text)
    field = lambda key: dict(zip(names, (int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, text))))
    return {k: field(k)[name] for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_kernel_has_no_scratch_and_no_spills(isa, kernel):
    r = _resources(isa, _mangled(isa, kernel))
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 64, r  # eight waves per SIMD
    assert not [ln for ln in _body(isa, _mangled(isa, kernel)) if ln.startswith("scratch_")]


@pytest.mark.timeout(600)
def test_the_gather_moves_sixteen_bytes_per_lane_as_global_accesses(isa):
    body = _body(isa, _mangled(isa, "gather_device_kernel"))
    count = lambda op: sum(1 for ln in body if ln.split()[0] == op)
    assert count("global_load_dwordx4") == 4 and count("global_store_dwordx4") == 4, [ln for ln in body if "load" in ln or "store" in ln][:12]
    assert not [ln for ln in body if ln.startswith("flat_")]
