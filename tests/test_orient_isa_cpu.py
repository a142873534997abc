"""The listing of K3O (k3o_orient.hip), checked without a GPU: orient_convert_kernel<RGB_U8 | RGBA_U8 | RGB_PLANAR_U8 | _F16 | _F32>, one
instantiation per RGB format.  None uses scratch or spills a register, none holds a fused multiply-add or multiply-accumulate in float32, each
holds the LDS tile and stays within the registers DESIGN.md states, parks and fetches its pixels as single dwords around ONE barrier, and the
kernels listed here are all the file has.  K3C (k3c_color.hip), whose helpers moved into k3c_pixel.h for K3O to share, and K3 (k3_idct.hip)
keep the listings they had before K3O existed, by their instruction counts."""
import os
import re
import subprocess

import pytest

from test_float_sink_isa_cpu import _fused, _opcodes
from test_planar_rgb_isa_cpu import CSRC, _resources

FORMATS = {"rgb_u8": 3, "rgba_u8": 4, "planar_u8": 7, "planar_f16": 8, "planar_f32": 9}
PREFIX = "_ZN5jpgpu12_GLOBAL__N_121orient_convert_kernelILi%dEEE"
K3C_PREFIX = "_ZN5jpgpu12_GLOBAL__N_120color_convert_kernelILi%dEEE"
LDS_BYTES = 64 * 65 * 4  # a tile of 64 x 64 dwords at a pitch of 65
MAX_VGPRS = 64  # sixteen loads in flight per lane; eight waves per SIMD stay possible
# instructions per kernel of the commit in front of K3O (the Makefile's flags)
K3C_BEFORE = {3: 442, 4: 417, 7: 460, 8: 511, 9: 502}
K3_BEFORE = (88, 181697)  # kernels, instructions in all


def _listing(tmp_path_factory, source):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / (source + ".s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, source)], stderr=subprocess.DEVNULL)
    return asm.read_text()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return _listing(tmp_path_factory, "k3o_orient.hip")


def _kernels(text):
    return [n for n in re.findall(r"\.name:\s+(\S+)", text) if n.startswith("_Z")]


@pytest.mark.timeout(600)
def test_the_instantiations_listed_here_are_all_the_file_has(isa):
    names = set(_kernels(isa))
    assert len(names) == len(FORMATS) and all(any(n.startswith(PREFIX % f) for n in names) for f in FORMATS.values()), names
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in makefile and "k3o_orient.o" in makefile and "k3c_pixel.h" in makefile


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_no_scratch_no_spilled_register_and_the_stated_lds_and_vgprs(isa, fmt):
    prefix = PREFIX % FORMATS[fmt]
    r = _resources(isa, prefix)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= MAX_VGPRS, r
    names = re.findall(r"\.name:\s+(\S+)", isa)
    for key, want in (("sgpr_spill_count", 0), ("group_segment_fixed_size", LDS_BYTES)):
        values = dict(zip(names, (int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, isa))))
        assert [v for n, v in values.items() if n.startswith(prefix)] == [want], key
    ops = _opcodes(isa, prefix)
    assert not any(op.startswith("scratch_") for op in ops), ops


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_no_multiply_is_fused_with_an_add(isa, fmt):
    ops = _opcodes(isa, PREFIX % FORMATS[fmt])
    assert _fused(ops) == 0, [op for op in ops if _fused([op])]
    assert not any(op.startswith(("v_fma", "v_mad_f", "v_mac_f", "v_pk_fma", "v_fmac", "v_mad_mix")) for op in ops), ops
    assert not any("pkrtz" in op for op in ops)
    if fmt in ("planar_f16", "planar_f32"):  # the affine step is there, as separate multiplies and adds (scalar or packed)
        assert ops.count("v_mul_f32") + ops.count("v_pk_mul_f32") >= 2 and ops.count("v_add_f32") + ops.count("v_pk_add_f32") >= 2, ops
    else:  # no float arithmetic but the one multiply of the tile index's division by the tiles per row (a reciprocal estimate in float32)
        floats = [op for op in ops if op.endswith(("_f32", "_f16")) and op.startswith(("v_mul", "v_add", "v_sub", "v_pk_"))]
        assert floats in ([], ["v_mul_f32"]), floats
    if fmt == "planar_f16":
        assert any(op in ("v_cvt_f16_f32", "v_cvt_pk_f16_f32") for op in ops)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_one_barrier_dword_lds_traffic_and_wide_stores(isa, fmt):
    ops = _opcodes(isa, PREFIX % FORMATS[fmt])
    assert ops.count("s_barrier") == 1, ops.count("s_barrier")
    lds = {op for op in ops if op.startswith("ds_")}
    assert lds and lds <= {"ds_read_b32", "ds_write_b32", "ds_read2_b32", "ds_write2_b32"}, lds  # (the bank analysis of DESIGN.md is for dwords)
    assert "global_load_dword" in ops and "global_load_ubyte" in ops  # 4-byte pixels whole, 1- and 3-byte pixels by their bytes
    assert "v_perm_b32" in ops or fmt == "rgba_u8"
    if fmt == "rgba_u8":
        assert "global_store_dwordx4" in ops
    if fmt == "rgb_u8":
        assert "global_store_dwordx3" in ops
    if fmt == "planar_f32":
        assert "global_store_dwordx4" in ops
    if fmt == "planar_f16":
        assert "global_store_dwordx2" in ops


@pytest.mark.timeout(900)
def test_k3c_and_k3_keep_their_listings(tmp_path_factory):
    k3c = _listing(tmp_path_factory, "k3c_color.hip")
    got = {f: len(_opcodes(k3c, K3C_PREFIX % f)) for f in K3C_BEFORE}
    assert got == K3C_BEFORE and len(_kernels(k3c)) == len(K3C_BEFORE), got
    k3 = _listing(tmp_path_factory, "k3_idct.hip")
    names = _kernels(k3)
    assert (len(names), sum(len(_opcodes(k3, n)) for n in names)) == K3_BEFORE
