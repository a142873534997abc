"""The listing of K3C (k3c_color.hip), checked without a GPU: color_convert_kernel<RGB_U8 | RGBA_U8 | RGB_PLANAR_U8 | _F16 | _F32>, one
instantiation per RGB format.  None uses scratch or spills a register, none holds a fused multiply-add or multiply-accumulate in float32 (the
affine step rounds its multiply and its add on their own), the binary16 conversion is never the packed round-toward-zero one, a group of four
4-component pixels is one 16-byte load, the results are packed with byte permutes, and the kernels listed here are all the file has."""
import os
import re
import subprocess

import pytest

from test_float_sink_isa_cpu import _fused, _opcodes
from test_planar_rgb_isa_cpu import CSRC, _resources

FORMATS = {"rgb_u8": 3, "rgba_u8": 4, "planar_u8": 7, "planar_f16": 8, "planar_f32": 9}
PREFIX = "_ZN5jpgpu12_GLOBAL__N_120color_convert_kernelILi%dEEE"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "k3c_color.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, "k3c_color.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


@pytest.mark.timeout(600)
def test_the_instantiations_listed_here_are_all_the_file_has(isa):
    names = {n for n in re.findall(r"\.name:\s+(\S+)", isa) if n.startswith("_Z")}
    assert len(names) == len(FORMATS) and all(any(n.startswith(PREFIX % f) for n in names) for f in FORMATS.values()), names
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in makefile and "k3c_color.o" in makefile


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_no_scratch_and_no_spilled_register(isa, fmt):
    prefix = PREFIX % FORMATS[fmt]
    r = _resources(isa, prefix)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 32, r  # (a streaming kernel: nothing but a group's pixels is alive)
    names = re.findall(r"\.name:\s+(\S+)", isa)
    sgpr_spills = dict(zip(names, (int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", isa))))
    assert [v for n, v in sgpr_spills.items() if n.startswith(prefix)] == [0]
    ops = _opcodes(isa, prefix)
    assert not any(op.startswith("scratch_") for op in ops), ops


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_no_multiply_is_fused_with_an_add(isa, fmt):
    ops = _opcodes(isa, PREFIX % FORMATS[fmt])
    assert _fused(ops) == 0, [op for op in ops if _fused([op])]
    assert not any("pkrtz" in op for op in ops)
    if fmt in ("planar_f16", "planar_f32"):  # the affine step is there, as separate multiplies and adds (scalar or packed)
        assert ops.count("v_mul_f32") + ops.count("v_pk_mul_f32") >= 2 and ops.count("v_add_f32") + ops.count("v_pk_add_f32") >= 2, ops
    else:
        assert not any(op.endswith("_f32") and op.startswith(("v_mul", "v_add")) for op in ops), ops
    if fmt == "planar_f16":
        assert any(op in ("v_cvt_f16_f32", "v_cvt_pk_f16_f32") for op in ops)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_four_pixels_per_lane_one_wide_load_and_byte_permutes(isa, fmt):
    ops = _opcodes(isa, PREFIX % FORMATS[fmt])
    assert ops.count("global_load_dwordx4") == 1, ops  # four CMYK / YCCK pixels
    assert ops.count("global_load_dwordx3") == 1, ops  # four Adobe-RGB pixels
    assert "v_perm_b32" in ops
    if fmt == "rgba_u8":
        assert "global_store_dwordx4" in ops
    if fmt == "rgb_u8":
        assert "global_store_dwordx3" in ops
