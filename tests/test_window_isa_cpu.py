"""The listing of K3's window instantiations, checked without a GPU: idct_window_kernel<format, class> for the four fast layout classes of
RGB_U8 (3) and RGB_PLANAR_U8 / _F16 / _F32 (7, 8, 9), for the generic class of INTERLEAVED_U8 (0) and INTERLEAVED_U8_SCALED (6), and
flush_window_kernel<0 | 6>.  None spills a vector register or uses scratch, and the IDCT butterflies are not contracted: no instantiation
has more fused multiply-adds than the whole-frame kernel of the same format and class, whose count tests/test_isa_invariants_cpu.py and
tests/test_float_sink_isa_cpu.py pin."""
import re

import pytest

from test_float_sink_isa_cpu import _fused, _opcodes, isa  # noqa: F401  (the fixture: one compile of k3_idct.hip per module)
from test_planar_rgb_isa_cpu import _resources

WINDOW, WHOLE = "_ZN5jpgpu18idct_window_kernelILi%dELi%dEEE", "_ZN5jpgpu18idct_output_kernelILi%dELi%dEEE"
FLUSH_WINDOW, FLUSH_WHOLE = "_ZN5jpgpu19flush_window_kernelILi%dEEE", "_ZN5jpgpu19flush_output_kernelILi%dEEE"
CASES = [(WINDOW % (f, c), WHOLE % (f, c)) for f in (3, 7, 8, 9) for c in (1, 2, 3, 4)] + [(WINDOW % (f, 0), WHOLE % (f, 0)) for f in (0, 6)] + \
        [(FLUSH_WINDOW % f, FLUSH_WHOLE % f) for f in (0, 6)]
IDS = [re.sub(r"^_ZN5jpgpu\d+|EEE$", "", w).replace("ILi", "<").replace("ELi", ",") + ">" for w, _ in CASES]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("window,whole", CASES, ids=IDS)
def test_no_scratch_and_no_spills(isa, window, whole):  # noqa: F811
    r = _resources(isa, window)
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r


@pytest.mark.timeout(600)
@pytest.mark.parametrize("window,whole", CASES, ids=IDS)
def test_the_butterflies_are_not_contracted(isa, window, whole):  # noqa: F811
    ops, twin = _opcodes(isa, window), _opcodes(isa, whole)
    assert _fused(ops) <= _fused(twin), (_fused(ops), _fused(twin))
    # ... and the transform is there, as many packed operations as the whole-frame kernel has (the flush of a store of samples has none)
    for op in ("v_pk_mul_f32", "v_pk_add_f32"):
        assert ops.count(op) >= twin.count(op), (op, ops.count(op), twin.count(op))


def test_every_window_instantiation_is_listed_here(isa):  # noqa: F811
    names = {n for n in re.findall(r"\.name:\s+(\S+)", isa) if "window_kernel" in n}
    assert len(names) == len(CASES) and all(any(n.startswith(w) for n in names) for w, _ in CASES), sorted(names)
