"""The listing of K4 (k4_resample.hip), checked without a GPU: resample_kernel<uint8_t | _Float16 | float>, one instantiation per sample type of
the resized buffer.  None uses scratch or spills a vector register, none holds a fused multiply-add or multiply-accumulate in float32 (the
definition rounds every multiply and every add on its own), the binary16 conversion is never the packed round-toward-zero one, the input
rows are staged with 16-byte loads and LDS writes, and the kernels listed here are all the file has."""
import os
import re
import subprocess

import pytest

from test_float_sink_isa_cpu import _fused, _opcodes
from test_planar_rgb_isa_cpu import CSRC, _resources

KERNELS = {"u8": "_ZN5jpgpu15resample_kernelIhEE", "f16": "_ZN5jpgpu15resample_kernelIDF16_EE", "f32": "_ZN5jpgpu15resample_kernelIfEE"}
STORE = {"u8": "global_store_byte", "f16": "global_store_short", "f32": "global_store_dword"}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "k4_resample.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, "k4_resample.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


@pytest.mark.timeout(600)
def test_the_instantiations_listed_here_are_all_the_file_has(isa):
    names = set(re.findall(r"\.name:\s+(\S+)", isa))
    kernels = {n for n in names if not n.endswith(".kd") and "resample_kernel" in n}
    assert len(kernels) == len(KERNELS) and all(any(n.startswith(p) for n in kernels) for p in KERNELS.values()), kernels
    assert {n for n in names if n.startswith("_Z")} == kernels, names  # (no other kernel in the file)
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read() and "k4_resample.o" in open(os.path.join(CSRC, "Makefile")).read()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", list(KERNELS))
def test_no_scratch_and_no_spilled_vector_register(isa, kind):
    r = _resources(isa, KERNELS[kind])
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 128, r  # (four waves per SIMD at the least: the LDS of a workgroup allows six workgroups per CU)
    ops = _opcodes(isa, KERNELS[kind])
    assert not any(op.startswith("scratch_") for op in ops), ops


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", list(KERNELS))
def test_no_multiply_is_fused_with_an_add(isa, kind):
    ops = _opcodes(isa, KERNELS[kind])
    assert _fused(ops) == 0, [op for op in ops if _fused([op])]
    assert not any("pkrtz" in op for op in ops)
    # the two passes are there as separate multiplies and adds (scalar or packed)
    assert ops.count("v_mul_f32") + ops.count("v_pk_mul_f32") >= 2 and ops.count("v_add_f32") + ops.count("v_pk_add_f32") >= 2, ops
    if kind == "u8":
        assert "v_rndne_f32" in ops  # (rint: ties to even)
    if kind == "f16":
        assert any(op in ("v_cvt_f16_f32", "v_cvt_pk_f16_f32") for op in ops)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", list(KERNELS))
def test_rows_are_staged_in_16_byte_pieces_and_every_store_is_one_sample(isa, kind):
    ops = _opcodes(isa, KERNELS[kind])
    assert ops.count("global_load_dwordx4") >= 3 and ops.count("ds_write_b128") >= 3, ops  # one staging loop per plane
    assert ops.count("ds_read_b64") >= 3 and "ds_read_u8" not in ops and "s_barrier" in ops  # eight taps of a plane per LDS read
    stores = {op for op in ops if op.startswith(("global_store", "flat_store"))}
    assert stores == {STORE[kind]}, stores
    lds = int(re.findall(r"\.group_segment_fixed_size:\s+(\d+)", isa)[0])
    assert lds <= 160 * 1024 // 6, lds
