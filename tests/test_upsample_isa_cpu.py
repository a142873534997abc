"""The listing of K3U (k3u_upsample.hip), checked without a GPU: fancy_upsample_kernel<RGB_U8 | RGBA_U8 | RGB_PLANAR_U8 | _F16 | _F32 | staged>,
one instantiation per sink.  None uses scratch memory or spills a register, each stays within the registers and the LDS DESIGN.md states
(which leave eight waves per SIMD possible), the colour conversion holds no fused multiply-add, the scratch image is read in dwords and
three-dword pieces, and the kernels listed here are all the file has."""
import os
import re

import pytest

from test_float_sink_isa_cpu import _fused
from test_orient_isa_cpu import _kernels, _listing
from test_planar_rgb_isa_cpu import CSRC, _resources

SINKS = {"rgb_u8": "3", "rgba_u8": "4", "planar_u8": "7", "planar_f16": "8", "planar_f32": "9", "staged": "n1"}
PREFIX = "_ZN5jpgpu12_GLOBAL__N_121fancy_upsample_kernelILi%sEEE"
# the column sums of a tile of 128 x 16 pixels, 16 rows of 128 dwords, and the 11 rows of native samples a tile of 4:2:0 or 4:4:0 touches
LDS_BYTES = (16 + 11) * 128 * 4
# 32 registers; 512 / 32 = 16 waves per SIMD fit the register file and 160 KB / 13.5 KB = 11 workgroups of four waves the LDS, so the
# SIMD's own limit of eight waves is what bounds the occupancy
MAX_VGPRS = 32


def _opcodes(text, mangled_prefix):
    """the opcodes of every instruction of the kernel, up to the end of the function (the kernel leaves early in two places: an s_endpgm each)"""
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    out = []
    for ln in lines[start + 1:end]:
        s = ln.strip()
        if s and not s.startswith((";", ".")) and not s.endswith(":"):
            out.append(re.sub(r"_(e32|e64|sdwa|dpp)$", "", s.split()[0]))
    assert out.count("s_endpgm") >= 1
    return out


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return _listing(tmp_path_factory, "k3u_upsample.hip")


@pytest.mark.timeout(600)
def test_the_instantiations_listed_here_are_all_the_file_has(isa):
    names = set(_kernels(isa))
    assert len(names) == len(SINKS) and all(any(n.startswith(PREFIX % s) for n in names) for s in SINKS.values()), names
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in makefile and "k3u_upsample.o" in makefile and "k3u_taps.h" in makefile


@pytest.mark.timeout(600)
@pytest.mark.parametrize("sink", list(SINKS))
def test_no_scratch_no_spilled_register_and_the_stated_lds_and_vgprs(isa, sink):
    prefix = PREFIX % SINKS[sink]
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
@pytest.mark.parametrize("sink", list(SINKS))
def test_no_multiply_is_fused_with_an_add_in_the_colour_conversion(isa, sink):
    ops = _opcodes(isa, PREFIX % SINKS[sink])
    assert _fused(ops) == 0, [op for op in ops if _fused([op])]
    assert not any(op.startswith(("v_fma", "v_mad_f", "v_mac_f", "v_pk_fma", "v_fmac", "v_mad_mix")) for op in ops), ops
    assert not any("pkrtz" in op for op in ops)
    if sink in ("planar_f16", "planar_f32"):  # the affine step is there, as separate multiplies and adds (scalar or packed)
        assert ops.count("v_mul_f32") + ops.count("v_pk_mul_f32") >= 2 and ops.count("v_add_f32") + ops.count("v_pk_add_f32") >= 2, ops
    else:  # no float arithmetic but the one multiply of the tile index's division by the tiles per row (a reciprocal estimate in float32)
        floats = [op for op in ops if op.endswith(("_f32", "_f16")) and op.startswith(("v_mul", "v_add", "v_sub", "v_pk_"))]
        assert floats in ([], ["v_mul_f32"]), floats
    if sink == "planar_f16":
        assert any(op in ("v_cvt_f16_f32", "v_cvt_pk_f16_f32") for op in ops)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("sink", list(SINKS))
def test_wide_loads_dword_lds_traffic_and_wide_stores(isa, sink):
    ops = _opcodes(isa, PREFIX % SINKS[sink])
    assert ops.count("s_barrier") == 2, ops.count("s_barrier")  # behind the native samples and behind the column sums (vs == 2)
    lds = {op for op in ops if op.startswith("ds_")}
    assert lds and all(op.endswith("_b32") for op in lds), lds
    loads = {op for op in ops if op.startswith("global_load")}
    assert loads == {"global_load_dword", "global_load_dwordx3"}, loads  # a native sample per dword, four pixels' luma per three dwords: no byte loads
    wide = {"rgb_u8": "global_store_dwordx3", "staged": "global_store_dwordx3", "rgba_u8": "global_store_dwordx4", "planar_u8": "global_store_dword",
            "planar_f16": "global_store_dwordx2", "planar_f32": "global_store_dwordx4"}[sink]
    assert wide in ops, (wide, sorted(set(op for op in ops if op.startswith("global_store"))))
