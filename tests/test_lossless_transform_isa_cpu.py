"""The listing of KX (kx_lossless.hip) compiled for gfx950, checked without a GPU: lossless_turn_kernel uses no scratch memory and spills no
register, and it moves its coefficients as 16-byte pieces -- global_load_dwordx4 in, global_store_dwordx4 out.  Nothing else is checked."""
import re

import pytest

from test_orient_isa_cpu import _kernels, _listing
from test_planar_rgb_isa_cpu import _resources
from test_upsample_isa_cpu import _opcodes

PREFIX = "_ZN5jpgpu12_GLOBAL__N_120lossless_turn_kernel"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return _listing(tmp_path_factory, "kx_lossless.hip")


@pytest.mark.timeout(600)
def test_no_scratch_and_no_spills(isa):
    names = _kernels(isa)
    assert len(names) == 1 and names[0].startswith(PREFIX), names
    r = _resources(isa, PREFIX)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    kernel_names = re.findall(r"\.name:\s+(\S+)", isa)
    spills = dict(zip(kernel_names, (int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", isa))))
    assert [v for n, v in spills.items() if n.startswith(PREFIX)] == [0]
    assert not any(op.startswith("scratch_") for op in _opcodes(isa, PREFIX))


@pytest.mark.timeout(600)
def test_sixteen_byte_global_loads_and_stores(isa):
    ops = _opcodes(isa, PREFIX)
    stores = {op for op in ops if op.startswith(("global_store", "flat_store"))}
    assert stores == {"global_store_dwordx4"}, stores
    # (what else is loaded from global memory is the descriptor's bytes and the transposition's table: at most eight bytes, never a coefficient)
    assert "global_load_dwordx4" in ops
    wide = {op for op in ops if op.startswith(("global_load", "flat_load")) and op.endswith(("dwordx3", "dwordx4"))}
    assert wide == {"global_load_dwordx4"}, wide
