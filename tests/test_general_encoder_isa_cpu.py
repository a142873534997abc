"""The two ISA invariants of test_isa_invariants_cpu.py for the general encoder's FDCT kernel (enc_general_fdct_kernel, one lane per
MCU of a described arrangement), checked without a GPU:

* FastFloatingPointDCT.TransformFDCT (FastFloatingPointDCT.cs:194-362) is not contracted: the 16 eight-point butterflies of a block
  keep their 14 multiplications each, and the only fused multiply-adds are the four per coefficient that reproduce the hardware's
  IEEE division (quant_divide) plus the two of the refined reciprocal (quant_pair);
* the kernel neither spills nor uses scratch (a block of 64 samples and the carried block stay in registers)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def enc_isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    flags = open(os.path.join(ROOT, "jpeglibrary_amd", "csrc", "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", flags, re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / "encode_kernels.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(ROOT, "jpeglibrary_amd", "csrc", "encode_kernels.hip")], stderr=subprocess.DEVNULL)
    return asm.read_text()


def _body(text, mangled_prefix):
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.rstrip().split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return [ln.strip() for ln in lines[start:end] if ln.strip() and not ln.strip().startswith(";")]


@pytest.mark.timeout(600)
def test_the_general_fdct_kernel_keeps_the_butterflies_in_ieee_steps(enc_isa):
    body = _body(enc_isa, "_ZN5jpgpu23enc_general_fdct_kernel")
    op = lambda ln: re.sub(r"_(e32|e64|sdwa|dpp)$", "", ln.split()[0])
    count = lambda name: sum(1 for ln in body if op(ln) == name)
    fused = count("v_fma_f32") + count("v_fmac_f32") + 2 * count("v_pk_fma_f32")
    assert fused <= 4 * 64 + 2, fused  # quant_divide's four per coefficient, quant_pair's two
    multiplies = count("v_mul_f32") + 2 * count("v_pk_mul_f32")
    assert multiplies >= 16 * 14 + 64 + 64, multiplies  # the butterflies, x 0.125, the quotient's first step
    assert count("v_rndne_f32") == 64  # MathF.Round, half to even, once per coefficient
    assert not any(ln.split()[0].startswith("v_mfma") for ln in body)


@pytest.mark.timeout(600)
def test_the_general_encoder_kernels_neither_spill_nor_use_scratch(enc_isa):
    names = re.findall(r"\.name:\s+(\S+)", enc_isa)
    spills = dict(zip(names, re.findall(r"\.vgpr_spill_count:\s+(\d+)", enc_isa)))
    sspills = dict(zip(names, re.findall(r"\.sgpr_spill_count:\s+(\d+)", enc_isa)))
    scratch = dict(zip(names, re.findall(r"\.private_segment_fixed_size:\s+(\d+)", enc_isa)))
    mine = [n for n in names if "enc_general_fdct_kernel" in n or any(k + "ILb1E" in n for k in ("block_bits_kernel", "block_stats_kernel", "emit_kernel"))]
    assert len(mine) == 4, mine
    for n in mine:
        assert spills[n] == "0" and sspills[n] == "0" and scratch[n] == "0", n
