"""The ISA of the kernels that serve the headline once K2 hands its coefficients to K3 as half-line planes, checked without a GPU:
idct_split_kernel<INTERLEAVED_U8, 4:2:0> computes what idct_output_kernel<0, 3> computes (the same packed-op counts, nothing
contracted), inside the budget that keeps three waves on a SIMD (168 VGPRs, no spill, no scratch); the pooled Huffman kernel
with its second flush neither spills nor uses scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    out = tmp_path_factory.mktemp("isa")
    procs = []
    for name in ("k2_huffman.hip", "k3_idct.hip"):
        asm = out / (name + ".s")
        procs.append((asm, subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S",
                                             "--cuda-device-only", "-o", str(asm), os.path.join(CSRC, name)], stderr=subprocess.DEVNULL)))
    text = []
    for asm, p in procs:
        assert p.wait() == 0, asm
        text.append(asm.read_text())
    return "\n".join(text)


def _resources(text, mangled_prefix):
    names = re.findall(r"\.name:\s+(\S+)", text)
    field = lambda key: dict(zip(names, (int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, text))))
    (name,) = [n for n in names if n.startswith(mangled_prefix)]
    return {k: field(k)[name] for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}


def _body(text, mangled_prefix):
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return [ln.strip() for ln in lines[start:end] if ln.strip() and not ln.strip().startswith(";")]


HEADLINE = "_ZN5jpgpu17idct_split_kernelILi0ELi3EEE"  # INTERLEAVED_U8, 4:2:0, half-line planes


@pytest.mark.timeout(600)
def test_the_split_form_of_the_headline_kernel_computes_the_same_transform(isa):
    body = _body(isa, HEADLINE)
    count = lambda op: sum(1 for ln in body if re.sub(r"_(e32|e64|sdwa|dpp)$", "", ln.split()[0]) == op)
    assert count("v_pk_add_f32") == 256
    assert count("v_pk_mul_f32") == 128
    assert count("v_rndne_f32") == 64
    assert count("v_fma_f32") + count("v_fmac_f32") + count("v_pk_fma_f32") <= 1
    assert not any(ln.split()[0].startswith("v_mfma") for ln in body)


@pytest.mark.timeout(600)
def test_the_split_form_of_the_headline_kernel_keeps_three_waves_per_simd(isa):
    r = _resources(isa, HEADLINE)
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 168, r


@pytest.mark.timeout(600)
def test_every_split_form_is_free_of_spills_and_scratch(isa):
    names = [n for n in re.findall(r"\.name:\s+(\S+)", isa) if "idct_split_kernel" in n]
    assert len(names) >= 10
    for n in names:
        r = _resources(isa, n)
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)


@pytest.mark.timeout(600)
def test_the_pooled_huffman_kernel_with_both_flushes_does_not_spill(isa):
    r = _resources(isa, "_ZN5jpgpu19huffman_pool_kernelILi11EEE")
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
