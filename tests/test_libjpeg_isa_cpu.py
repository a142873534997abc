"""The listing of K3J (k3j_islow.hip), checked without a GPU, from the compiler's resource table alone.

islow_kernel, the file's one kernel: no scratch memory, no spilled vector or scalar register, the registers its __launch_bounds__(256, 4)
allows, and the LDS its design states -- the staging of 256 blocks and four tables of 64 uint16.  (The block transform itself is run on the
CPU by tests/test_libjpeg_cpu.py; every other kernel object's pinned listing passes untouched.)"""
import os

import pytest

from test_luma_isa_cpu import _field
from test_orient_isa_cpu import _kernels, _listing
from test_planar_rgb_isa_cpu import CSRC, _resources

KERNEL = "_ZN5jpgpu12_GLOBAL__N_112islow_kernelE"
# __launch_bounds__(256, 4): four waves per SIMD need at most 512 / 4 = 128 registers per lane; 256 * 128 + 4 * 128 = 33 280 bytes of LDS, so four
# workgroups fit the 160 KiB of a CU as well
MAX_VGPRS, LDS = 128, 256 * 128 + 4 * 128


@pytest.fixture(scope="module")
def k3j(tmp_path_factory):
    return _listing(tmp_path_factory, "k3j_islow.hip")


@pytest.mark.timeout(600)
def test_the_kernel_listed_here_is_all_the_file_has(k3j):
    names = _kernels(k3j)
    assert len(names) == 1 and names[0].startswith(KERNEL), names
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for name in ("k3j_islow.o", "k3j_islow.h"):
        assert name in makefile, name
    src = open(os.path.join(CSRC, "k3j_islow.hip")).read()
    assert '#include "k3j_islow.h"' in src and "__launch_bounds__(kIslowThreads, 4)" in src
    assert "float" not in open(os.path.join(CSRC, "k3j_islow.h")).read().replace("No float", "")  # the transform is integers


@pytest.mark.timeout(600)
def test_no_scratch_no_spilled_register_and_the_stated_lds_and_vgprs(k3j):
    r = _resources(k3j, KERNEL)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert _field(k3j, KERNEL, "sgpr_spill_count") == 0
    assert r["vgpr_count"] <= MAX_VGPRS, r
    assert _field(k3j, KERNEL, "group_segment_fixed_size") == LDS
