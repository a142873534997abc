"""The resource metadata of encoder stage E1J's kernels (e1j_libjpeg.hip), read from the gfx950 listing without a GPU: the three instances
neither spill nor use scratch (a row or a column of a block, eight values, is all a lane holds), they take their LDS statically, and the
division of the quantisation is not the compiler's (v_rcp_iflag_f32 is what a 32-bit division by a run-time value expands to)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def e1j_isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    flags = open(os.path.join(ROOT, "jpeglibrary_amd", "csrc", "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", flags, re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "e1j_libjpeg.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(ROOT, "jpeglibrary_amd", "csrc", "e1j_libjpeg.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


def _field(text, name):
    return re.findall(r"\.%s:\s+(\S+)" % name, text)


@pytest.mark.timeout(600)
def test_the_e1j_kernels_neither_spill_nor_use_scratch(e1j_isa):
    names = _field(e1j_isa, "name")
    kernels = [n for n in names if "e1j_fdct_kernel" in n]
    assert len(kernels) == 3 and len({n for n in kernels}) == 3, names  # 2 x 2, 2 x 1, 1 x 1
    per = {f: dict(zip(names, _field(e1j_isa, f))) for f in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
                                                             "vgpr_count")}
    for n in kernels:
        assert per["vgpr_spill_count"][n] == "0" and per["sgpr_spill_count"][n] == "0" and per["private_segment_fixed_size"][n] == "0", n
        assert 0 < int(per["group_segment_fixed_size"][n]) <= 16 * 1024, n  # four workgroups and more per CU
        assert int(per["vgpr_count"][n]) <= 64, n                          # a full complement of waves
    assert not re.search(r"^\s*(scratch_|buffer_(load|store).*offen)", e1j_isa, re.M)


@pytest.mark.timeout(600)
def test_the_e1j_kernels_store_whole_records_and_divide_without_the_compilers_division(e1j_isa):
    for shape in ("ILi2ELi2E", "ILi2ELi1E", "ILi1ELi1E"):
        lines = e1j_isa.splitlines()
        start = next(i for i, ln in enumerate(lines) if "e1j_fdct_kernel" + shape in ln and ln.split(";")[0].strip().endswith(":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))  # (the early returns end the program too)
        body = [ln.strip() for ln in lines[start:end] if ln.strip() and not ln.strip().startswith(";")]
        ops = [ln.split()[0] for ln in body]
        assert ops.count("global_store_dwordx4") >= 1, shape
        assert any(op.startswith("v_mul_hi_u32") for op in ops), shape
        # a 32-bit division by a run-time value brings the reciprocal-and-correct expansion into the vector code: one is there, the wave's
        # first MCU index split into column and row, ahead of every loop; the 64 quantisations of a block add none
        assert sum(op.startswith("v_rcp_iflag_f32") for op in ops) <= 1, shape
