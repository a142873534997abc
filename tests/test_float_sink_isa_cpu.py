"""The listing of K3's RGB_PLANAR_F16 / _F32 instantiations, checked without a GPU: idct_output_kernel<8 | 9, class> and
idct_split_kernel<8 | 9, class> for the four fast layout classes (1 = 4:4:4, 2 = 4:2:2, 3 = 4:2:0, 4 = gray) -- a split form for every class
idct_split_supported admits, which is all four -- and the float converter of the generic class.  None spills a vector register or uses
scratch, each stays within the 168 VGPRs three waves per SIMD allow, the affine step was not contracted into a fused multiply-add (no more
of those than the RGB_PLANAR_U8 twin has), the binary16 conversion is never the packed round-toward-zero one, and the task loop stores
whole 16-byte pieces: per plane one (F16) or two (F32) for a one-block task, two or four for a two-block one."""
import os
import re
import subprocess

import pytest

from test_k3_variants_cpu import k3_compiled_variants, k3_variant_rows
from test_planar_rgb_isa_cpu import CSRC, KERNELS, _resources, _task_loop

FMT_U8, FMT_F16, FMT_F32 = 7, 8, 9
BLOCKS_WIDE = {1: 1, 2: 2, 3: 2, 4: 1}  # layout class -> blocks a task spans
SPLIT_CLASSES = (1, 2, 3, 4)            # kernels.h: idct_split_supported(RGB_PLANAR_F16 / _F32, class)
CASES = [(fmt, form, cls) for fmt in (FMT_F16, FMT_F32) for cls in BLOCKS_WIDE for form in KERNELS if form == "dense" or cls in SPLIT_CLASSES]
IDS = ["%s-%s-class%d" % ("f16" if f == FMT_F16 else "f32", form, cls) for f, form, cls in CASES]
CONVERTERS = ["_ZN5jpgpu24ycc_to_rgb_planes_kernelIDF16_EE", "_ZN5jpgpu24ycc_to_rgb_planes_kernelIfEE"]
_FMA = ("v_fma_", "v_fmac_", "v_mad_f", "v_mac_f", "v_pk_fma_", "v_fma_mix", "v_mad_mix")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "k3_idct.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, "k3_idct.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


def _opcodes(text, mangled_prefix):
    """the opcodes of every instruction of the kernel"""
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    out = []
    for ln in lines[start + 1:end + 1]:
        s = ln.strip()
        if s and not s.startswith((";", ".")) and not s.endswith(":"):
            out.append(re.sub(r"_(e32|e64|sdwa|dpp)$", "", s.split()[0]))
    return out


def _fused(ops):
    return sum(op.startswith(_FMA) for op in ops)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt,form,cls", CASES, ids=IDS)
def test_every_instantiation_keeps_three_waves_per_simd_without_spill_or_scratch(isa, fmt, form, cls):
    r = _resources(isa, KERNELS[form] % (fmt, cls))
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 168, r


@pytest.mark.timeout(600)
def test_the_split_forms_are_the_ones_idct_split_supported_admits(isa):
    names = set(re.findall(r"\.name:\s+(\S+)", isa))
    for fmt in (FMT_F16, FMT_F32):
        have = {cls for cls in range(0, 6) if any(n.startswith(KERNELS["split"] % (fmt, cls)) for n in names)}
        assert have == set(SPLIT_CLASSES), (fmt, have)
    rows = k3_variant_rows()  # the rule itself (kernels.h: k3_variant), printed by a host program
    for fmt in (FMT_F16, FMT_F32):
        assert {cls for cls in range(0, 6) if rows[("split", fmt, cls)] != "-"} == set(SPLIT_CLASSES), fmt
        assert rows[("split", fmt, 0)] == "-" and rows[("split", fmt, 5)] == "-"
        assert all(rows[("split", fmt, cls)] == "%d,%d" % (fmt, cls) for cls in SPLIT_CLASSES)


@pytest.mark.timeout(600)
def test_the_listing_holds_exactly_the_variants_the_rule_enumerates(isa):
    """the idct_* and flush_* kernels of the listing against the rule's enumeration: neither a variant the launcher cannot reach nor one it
    reaches and nobody compiled"""
    names = set(re.findall(r"\.name:\s+(\S+)", isa))
    have = set()
    for n in names:
        m = re.match(r"_ZN5jpgpu\d+((?:idct|flush)_\w+?_kernel)ILi(\d+)E(?:Li(\d+)E)?EE", n)
        if m:
            have.add((m.group(1), tuple(int(v) for v in m.groups()[1:] if v is not None)))
    want = k3_compiled_variants()
    assert have == want, (sorted(have - want), sorted(want - have))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt,form,cls", CASES, ids=IDS)
def test_the_affine_step_is_not_fused_and_the_conversion_rounds_to_nearest(isa, fmt, form, cls):
    ops, twin = _opcodes(isa, KERNELS[form] % (fmt, cls)), _opcodes(isa, KERNELS[form] % (FMT_U8, cls))
    assert _fused(ops) <= _fused(twin), (_fused(ops), _fused(twin))
    assert not any("pkrtz" in op for op in ops)
    loop = _task_loop(isa, KERNELS[form] % (fmt, cls))
    samples = 8 * BLOCKS_WIDE[cls] * 3  # of one task: three planes
    assert sum(op.startswith("v_cvt_f32_ubyte") for op in loop) >= (samples if cls != 4 else samples // 3), loop  # (gray: one conversion serves three planes)
    assert loop.count("v_mul_f32") + 2 * loop.count("v_pk_mul_f32") >= samples and loop.count("v_add_f32") + 2 * loop.count("v_pk_add_f32") >= samples, loop
    if fmt == FMT_F16:  # round to nearest even: the packed form gfx950 has, or the scalar one
        assert 2 * loop.count("v_cvt_pk_f16_f32") + loop.count("v_cvt_f16_f32") == samples, loop


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fmt,form,cls", CASES, ids=IDS)
def test_the_task_loop_stores_whole_16_byte_pieces(isa, fmt, form, cls):
    loop = _task_loop(isa, KERNELS[form] % (fmt, cls))
    stores = [op for op in loop if op.startswith(("global_store", "flat_store", "scratch_"))]
    per_plane = 8 * BLOCKS_WIDE[cls] * (2 if fmt == FMT_F16 else 4) // 16
    assert stores == ["global_store_dwordx4"] * (3 * per_plane), stores
    assert not any(op.startswith(("v_writelane", "v_readlane")) for op in loop), loop  # (scalars parked in vector lanes move outside this loop)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", CONVERTERS, ids=["f16", "f32"])
def test_the_converter_of_the_generic_class(isa, name):
    r = _resources(isa, name)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    ops = _opcodes(isa, name)
    assert _fused(ops) == 0 and not any("pkrtz" in op for op in ops), ops
    # one sample per store: a plane's start is aligned for one sample only
    want = "global_store_short" if "DF16_" in name else "global_store_dword"
    assert [op for op in ops if op.startswith("global_store")] == [want] * 3, ops
