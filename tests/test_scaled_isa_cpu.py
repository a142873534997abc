"""The listing of K3R (k3r_reduced.hip), checked without a GPU, from the compiler's resource table and the kernel's instructions.

reduced_kernel, the file's one kernel: no scratch memory, no spilled vector or scalar register, the registers its __launch_bounds__(256, 4)
allows, the LDS its design states -- K3J's staging of 256 blocks and four tables of 64 uint16 --, the eight DMA loads of sixteen bytes that
bring the coefficients in, and no float instruction in a transform of integers.  (The block transforms themselves are run on the CPU by
tests/test_scaled_cpu.py; every other kernel object's pinned listing passes untouched.)"""
import os

import pytest

from test_device_input_isa_cpu import _body
from test_luma_isa_cpu import _field
from test_orient_isa_cpu import _kernels, _listing
from test_planar_rgb_isa_cpu import CSRC, _resources

KERNEL = "_ZN5jpgpu12_GLOBAL__N_114reduced_kernelE"
# __launch_bounds__(256, 4): four waves per SIMD need at most 512 / 4 = 128 registers per lane; 256 * 128 + 4 * 128 = 33 280 bytes of LDS, so four
# workgroups fit the 160 KiB of a CU as well
MAX_VGPRS, LDS = 128, 256 * 128 + 4 * 128


@pytest.fixture(scope="module")
def k3r(tmp_path_factory):
    return _listing(tmp_path_factory, "k3r_reduced.hip")


@pytest.mark.timeout(600)
def test_the_kernel_listed_here_is_all_the_file_has(k3r):
    names = _kernels(k3r)
    assert len(names) == 1 and names[0].startswith(KERNEL), names
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for name in ("k3r_reduced.o", "k3r_reduced.h"):
        assert name in makefile, name
    src = open(os.path.join(CSRC, "k3r_reduced.hip")).read()
    assert '#include "k3r_reduced.h"' in src and "__launch_bounds__(kIslowThreads, 4)" in src
    assert "float" not in open(os.path.join(CSRC, "k3r_reduced.h")).read().replace("No float", "")  # the transforms are integers


@pytest.mark.timeout(600)
def test_no_scratch_no_spilled_register_and_the_stated_lds_and_vgprs(k3r):
    r = _resources(k3r, KERNEL)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert _field(k3r, KERNEL, "sgpr_spill_count") == 0
    assert r["vgpr_count"] <= MAX_VGPRS, r
    assert _field(k3r, KERNEL, "group_segment_fixed_size") == LDS


@pytest.mark.timeout(600)
def test_the_coefficients_come_by_dma_and_the_transforms_are_integers(k3r):
    ops = [ln.split()[0] for ln in _body(k3r, KERNEL)]
    assert ops.count("global_load_lds_dwordx4") == 8, ops.count("global_load_lds_dwordx4")
    assert not [op for op in ops if op.startswith(("scratch_", "buffer_"))]
    # (the compiler divides 32-bit integers through a float reciprocal -- v_rcp_iflag_f32, v_mul_f32, v_fma_f32 --; what K3's float transform
    # is made of -- packed arithmetic, adds and subtractions, rounding to even, the saturating pack -- is not here)
    floats = ("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32", "v_add_f32", "v_sub_f32", "v_rndne_f32", "v_sat_pk_u8_i16")
    assert not [op for op in ops if op.startswith(floats) or "_f16" in op or "_f64" in op], "K3's float transform in K3R"
    stores = {op for op in ops if op.startswith(("global_store", "flat_store"))}
    assert "global_store_dword" in stores and stores <= {"global_store_dword", "global_store_byte", "global_store_byte_d16_hi"}, stores
