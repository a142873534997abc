"""The resource metadata of the progressive entropy coder's kernels (encode_progressive.hip), read from the gfx950 listing without a GPU:
none of the seven spills or uses scratch, each takes its LDS statically (2 KB at most: the scan's two tables or its two histograms), and
each stays within 48 VGPRs.  The planned occupancy is eight waves per SIMD, the most the hardware holds (it takes 64 VGPRs or fewer):
every kernel is one lane per block and hides its loads behind other waves.  The kernels use 38 VGPRs at most as built; 48 leaves the
compiler some room and still shows a regression long before the occupancy is lost."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["prog_classify_kernel", "prog_runs_kernel", "prog_stats_kernel", "prog_bits_kernel", "prog_offsets_kernel", "prog_emit_kernel",
           "prog_assemble_kernel"]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    flags = open(os.path.join(ROOT, "jpeglibrary_amd", "csrc", "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", flags, re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "encode_progressive.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(ROOT, "jpeglibrary_amd", "csrc", "encode_progressive.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


def _field(text, name):
    return re.findall(r"\.%s:\s+(\S+)" % name, text)


@pytest.mark.timeout(600)
def test_the_progressive_kernels_neither_spill_nor_use_scratch_and_keep_eight_waves(isa):
    names = _field(isa, "name")
    per = {f: dict(zip(names, _field(isa, f))) for f in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
                                                         "vgpr_count", "max_flat_workgroup_size")}
    for kernel in KERNELS:
        found = [n for n in names if kernel in n]
        assert len(found) == 1, (kernel, names)
        n = found[0]
        assert per["vgpr_spill_count"][n] == "0" and per["sgpr_spill_count"][n] == "0" and per["private_segment_fixed_size"][n] == "0", n
        assert int(per["group_segment_fixed_size"][n]) <= 2048, n  # static, and no limit on the workgroups per CU
        assert int(per["vgpr_count"][n]) <= 48, n                  # eight waves per SIMD need <= 64; 38 at most as built
        assert int(per["max_flat_workgroup_size"][n]) == 256, n
    source = open(os.path.join(ROOT, "jpeglibrary_amd", "csrc", "encode_progressive.hip")).read()
    assert "extern __shared__" not in source  # no kernel asks for LDS at launch
