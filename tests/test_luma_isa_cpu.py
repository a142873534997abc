"""The listings of K3Y (k3y_luma.hip) and of K4's one-plane form (k4y_resample_luma.hip), checked without a GPU.

luma_idct_kernel<uint8 | float16 | float32, windowed or not> and luma_plane_kernel<uint8 | float16 | float32>, resample_luma_kernel<the same
three>: none uses scratch memory or spills a register, none holds a fused multiply-add or multiply-accumulate in float32, each stays within the
registers its __launch_bounds__ and DESIGN.md state, the IDCT kernel fetches its coefficients by LDS-DMA around ONE barrier
and stores a block row as one piece of 8 bytes (uint8) or pieces of 16 (float16, float32); and the kernels listed here are all the two
files have.  (K3's and K3C's pinned listings: tests/test_orient_isa_cpu.py, which passes untouched.)"""
import os
import re

import pytest

from test_float_sink_isa_cpu import _fused
from test_orient_isa_cpu import _kernels, _listing
from test_planar_rgb_isa_cpu import CSRC, _resources
from test_upsample_isa_cpu import _opcodes

TYPES = {"u8": "h", "f16": "DF16_", "f32": "f"}
IDCT = "_ZN5jpgpu12_GLOBAL__N_116luma_idct_kernelI%sLb%dEEE"
PLANE = "_ZN5jpgpu12_GLOBAL__N_117luma_plane_kernelI%sEEv"
RESAMPLE = "_ZN5jpgpu20resample_luma_kernelI%sEEv"
IDCT_CASES = [(t, w) for t in TYPES for w in (0, 1)]
# __launch_bounds__(256, 4): four waves per SIMD need at most 512 / 4 = 128 registers per lane; the staging of 256 blocks and one table of
# 64 floats is 33 024 bytes, so four workgroups fit the 160 KiB of a CU as well
IDCT_MAX_VGPRS, IDCT_LDS = 128, 256 * 128 + 256
# __launch_bounds__(256): DESIGN.md states 64 registers (eight waves per SIMD) and a byte tile of 64 rows at a pitch of 68
PLANE_MAX_VGPRS, PLANE_LDS = 64, 64 * 68
# K4's bound (tests/test_resize_isa_cpu.py): four waves per SIMD at the least
RESAMPLE_MAX_VGPRS = 128
FMA = ("v_fma", "v_mad_f", "v_mac_f", "v_pk_fma", "v_fmac", "v_mad_mix")


@pytest.fixture(scope="module")
def k3y(tmp_path_factory):
    return _listing(tmp_path_factory, "k3y_luma.hip")


@pytest.fixture(scope="module")
def k4y(tmp_path_factory):
    return _listing(tmp_path_factory, "k4y_resample_luma.hip")


def _field(isa, prefix, key):
    names = re.findall(r"\.name:\s+(\S+)", isa)
    values = dict(zip(names, (int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, isa))))
    (v,) = [v for n, v in values.items() if n.startswith(prefix)]
    return v


def _clean(isa, prefix, max_vgprs):
    r = _resources(isa, prefix)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= max_vgprs, r
    assert _field(isa, prefix, "sgpr_spill_count") == 0
    ops = _opcodes(isa, prefix)
    assert not any(op.startswith("scratch_") for op in ops), ops
    assert _fused(ops) == 0, [op for op in ops if _fused([op])]
    assert not any(op.startswith(FMA) for op in ops), [op for op in ops if op.startswith(FMA)]
    assert not any("pkrtz" in op for op in ops)
    return ops


@pytest.mark.timeout(600)
def test_the_instantiations_listed_here_are_all_the_files_have(k3y, k4y):
    want = {IDCT % (TYPES[t], w) for t, w in IDCT_CASES} | {PLANE % t for t in TYPES.values()}
    names = set(_kernels(k3y))
    assert len(names) == len(want) and all(any(n.startswith(p) for n in names) for p in want), names
    want4 = {RESAMPLE % t for t in TYPES.values()}
    names4 = set(_kernels(k4y))
    assert len(names4) == len(want4) and all(any(n.startswith(p) for n in names4) for p in want4), names4
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in makefile
    for name in ("k3y_luma.o", "k4y_resample_luma.o", "k3_block_idct.h", "k4_resample_body.h"):
        assert name in makefile, name
    # the transform and the resampling are stated once: the new files and the old ones include the shared headers
    for src, header in (("k3y_luma.hip", "k3_block_idct.h"), ("k3_idct.hip", "k3_block_idct.h"), ("k4y_resample_luma.hip", "k4_resample_body.h"),
                        ("k4_resample.hip", "k4_resample_body.h")):
        assert '#include "%s"' % header in open(os.path.join(CSRC, src)).read(), (src, header)
    for src in ("k3y_luma.hip", "k3_idct.hip"):
        assert "void idct8(" not in open(os.path.join(CSRC, src)).read(), src


@pytest.mark.timeout(600)
@pytest.mark.parametrize("t,win", IDCT_CASES, ids=["%s-%s" % (t, "window" if w else "frame") for t, w in IDCT_CASES])
def test_the_idct_kernel_is_clean_and_stores_wide_pieces(k3y, t, win):
    prefix = IDCT % (TYPES[t], win)
    ops = _clean(k3y, prefix, IDCT_MAX_VGPRS)
    assert _field(k3y, prefix, "group_segment_fixed_size") == IDCT_LDS
    # eight DMA instructions of sixteen bytes per lane fill the staging; the lane reads its block back as eight 16-byte pieces and the table
    # in the transform's pair order; one barrier
    assert ops.count("global_load_lds_dwordx4") == 8 and ops.count("s_barrier") == 1, (ops.count("global_load_lds_dwordx4"), ops.count("s_barrier"))
    assert ops.count("ds_read_b128") >= 8 + 16
    # the transform is K3's: packed float arithmetic, rounding to even, the saturating pack
    assert "v_pk_mul_f32" in ops and "v_pk_add_f32" in ops and "v_rndne_f32" in ops and ops.count("v_sat_pk_u8_i16") == 32
    stores = [op for op in ops if op.startswith(("global_store", "flat_store"))]
    wide = {"u8": "global_store_dwordx2", "f16": "global_store_dwordx4", "f32": "global_store_dwordx4"}[t]
    narrow = {"u8": ("global_store_byte", "global_store_byte_d16_hi"), "f16": ("global_store_short", "global_store_short_d16_hi"), "f32": ("global_store_dword",)}[t]
    assert stores.count(wide) >= 8, stores  # a block row in one piece (uint8, float16); float32's second piece may share its tail with the edge path
    assert set(stores) <= {wide, *narrow} | ({"global_store_dwordx3"} if t == "f32" else set()), set(stores)
    if t != "u8":  # the affine step, as separate multiplies and adds
        assert ops.count("v_mul_f32") + ops.count("v_pk_mul_f32") >= 2 and ops.count("v_add_f32") + ops.count("v_pk_add_f32") >= 2
    if t == "f16":
        assert any(op in ("v_cvt_f16_f32", "v_cvt_pk_f16_f32") for op in ops)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("t", list(TYPES))
def test_the_plane_kernel_is_clean_and_parks_bytes_around_one_barrier(k3y, t):
    prefix = PLANE % TYPES[t]
    ops = _clean(k3y, prefix, PLANE_MAX_VGPRS)
    assert _field(k3y, prefix, "group_segment_fixed_size") == PLANE_LDS
    assert ops.count("s_barrier") == 1
    lds = {op for op in ops if op.startswith("ds_")}
    assert lds and lds <= {"ds_write_b8", "ds_write_b8_d16_hi", "ds_read_u8", "ds_read_u8_d16", "ds_read_u8_d16_hi"}, lds  # a parked pixel is one byte
    assert "global_load_dword" in ops and "global_load_ubyte" in ops  # 4-byte pixels whole, 1- and 3-byte pixels by their bytes
    stores = {op for op in ops if op.startswith(("global_store", "flat_store"))}
    assert stores == {{"u8": "global_store_byte", "f16": "global_store_short", "f32": "global_store_dword"}[t]}, stores
    if t != "u8":
        assert ops.count("v_mul_f32") >= 1 and ops.count("v_add_f32") >= 1


@pytest.mark.timeout(600)
@pytest.mark.parametrize("t", list(TYPES))
def test_the_one_plane_resampler_is_clean_and_reads_eight_taps_per_lds_read(k4y, t):
    prefix = RESAMPLE % TYPES[t]
    ops = _clean(k4y, prefix, RESAMPLE_MAX_VGPRS)
    assert _field(k4y, prefix, "group_segment_fixed_size") <= 160 * 1024 // 6
    assert ops.count("v_mul_f32") + ops.count("v_pk_mul_f32") >= 2 and ops.count("v_add_f32") + ops.count("v_pk_add_f32") >= 2
    assert ops.count("global_load_dwordx4") >= 1 and ops.count("ds_write_b128") >= 1 and ops.count("ds_read_b64") >= 1 and "ds_read_u8" not in ops and "s_barrier" in ops
    stores = {op for op in ops if op.startswith(("global_store", "flat_store"))}
    assert stores == {{"u8": "global_store_byte", "f16": "global_store_short", "f32": "global_store_dword"}[t]}, stores
    if t == "u8":
        assert "v_rndne_f32" in ops
    if t == "f16":
        assert any(op in ("v_cvt_f16_f32", "v_cvt_pk_f16_f32") for op in ops)
