"""The listing of fdct_fused_kernel's planar instances (device uploads with JPGPU_PIXELS_PLANAR: 4:2:0, 4:2:2 and 4:4:4 from three tight planes),
checked without a GPU.  They are the interleaved instances with another fetch, so they are held to what
test_isa_invariants_cpu.py::test_the_fused_encoder_kernel_keeps_the_fdct_in_ieee_steps demands of those: no spill, no scratch, at most 168 VGPRs,
twelve waves' worth of LDS per CU, the FDCT as packed IEEE multiplies and additions -- and the fetch is one wide load per plane: 16 bytes
where an MCU is two blocks wide, 8 where it is one (three fetch sites: the first round's, the look-ahead's, the dword-aligned edge rows')."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")

KERNEL = "_ZN5jpgpu17fdct_fused_kernelILi%dELi%dELi%dEEE"
PLANAR = 1  # the BPP argument of the planar instances (kEfPlanar)
SHAPES = [(2, 2), (2, 1), (1, 1)]


@pytest.fixture(scope="module")
def enc_isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "encode_kernels.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, "encode_kernels.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


def _body(text, mangled_prefix):
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return [ln.strip() for ln in lines[start:end] if ln.strip() and not ln.strip().startswith(";")]


def _resources(text, mangled_prefix):
    names = re.findall(r"\.name:\s+(\S+)", text)
    field = lambda key: dict(zip(names, (int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, text))))
    (name,) = [n for n in names if n.startswith(mangled_prefix)]
    return {k: field(k)[name] for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("h,v", SHAPES, ids=["420", "422", "444"])
def test_a_planar_instance_keeps_the_fused_kernel_s_resources(enc_isa, h, v):
    r = _resources(enc_isa, KERNEL % (h, v, PLANAR))
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 168, r
    assert r["group_segment_fixed_size"] * 12 <= 160 * 1024, r  # twelve waves per CU


@pytest.mark.timeout(600)
@pytest.mark.parametrize("h,v", SHAPES, ids=["420", "422", "444"])
def test_a_planar_instance_keeps_the_fdct_in_packed_ieee_steps(enc_isa, h, v):
    """The counts test_the_fused_encoder_kernel_keeps_the_fdct_in_ieee_steps demands of fdct_fused_kernel<2, 2, 3>: five packed butterflies of
    14 multiplications and 26 additions.  With H = 2 a lane has the left and the right block of its row side by side in one packed pass 1
    (92 v_pk_mul_f32 / 134 v_pk_add_f32).  With H = 1 its row is ONE block wide, so the planar 4:4:4 instance pairs the rows of two consecutive
    gather rounds instead (96 / 136; as one scalar butterfly per round, which the interleaved 4:4:4 instances keep, it was 86 / 128)."""
    body = _body(enc_isa, KERNEL % (h, v, PLANAR))
    op = lambda ln: re.sub(r"_(e32|e64|sdwa|dpp)$", "", ln.split()[0])
    count = lambda name: sum(1 for ln in body if op(ln) == name)
    print("fdct_fused_kernel<%d, %d, planar>: v_pk_mul_f32 %d, v_pk_add_f32 %d, v_fma_f32 + v_fmac_f32 %d" %
          (h, v, count("v_pk_mul_f32"), count("v_pk_add_f32"), count("v_fma_f32") + count("v_fmac_f32")))
    assert count("v_fma_f32") + count("v_fmac_f32") <= 2 * 2  # quant_pair's refined reciprocal, once per table
    n_butterflies = 2 + 1 + 2  # pass 1 (edge + fast variant), pass 2 of luma, chroma pass 1 + pass 2
    assert count("v_pk_mul_f32") >= 14 * n_butterflies
    assert count("v_pk_add_f32") >= 26 * n_butterflies


@pytest.mark.timeout(600)
@pytest.mark.parametrize("h,v", SHAPES, ids=["420", "422", "444"])
def test_a_planar_instance_fetches_one_wide_load_per_plane(enc_isa, h, v):
    body = _body(enc_isa, KERNEL % (h, v, PLANAR))
    wide = "global_load_dwordx4" if h == 2 else "global_load_dwordx2"
    assert sum(1 for ln in body if ln.split()[0] == wide) >= 3, [ln for ln in body if ln.startswith("global_load")]


@pytest.mark.timeout(600)
def test_the_interleaved_instances_keep_their_names_and_come_first(enc_isa):
    names = [n for n in re.findall(r"\.name:\s+(\S+)", enc_isa) if "fdct_fused_kernel" in n]
    want = [KERNEL % (h, v, bpp) for bpp in (3, 4, PLANAR) for (h, v) in SHAPES]
    assert len(names) == 9 and [any(n.startswith(w) for n in names) for w in want] == [True] * 9, names
    assert names[0].startswith(KERNEL % (2, 2, 3)), names  # (the instance test_isa_invariants_cpu.py looks at)
