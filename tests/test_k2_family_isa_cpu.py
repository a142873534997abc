"""The listings of the K2 family (k2_huffman.hip, k2s_subseq.hip), checked without a GPU, against the commit in front of k2_wave.h.

K2 and the final pass of K2S take their block decode, their dense flush, their stream open, their workgroup set-up and their ticket loop
from one header, k2_wave.h.  Sharing them must cost nothing: for the twelve kernels built on the header -- huffman_decode_kernel<7..11>,
huffman_pool_kernel<7..11>, subseq_final_kernel<false | true> -- the registers, the spills, the scratch and the static LDS are EXACTLY what
the parent commit's were (a LOWER VGPR count is how the four DC predictors falling into an indexed private array showed itself, see
k2_decode_dc), every memory and synchronisation opcode occurs as often as it did, and the instruction total is at most the parent's + 0.5 %.
The other kernels of the two files are not touched and keep their opcode sequences; no instantiation is added or lost.

PARENT holds what the same command (the Makefile's flags, -S --cuda-device-only) gave at the parent commit."""
import hashlib
import os
import re
import subprocess
from collections import Counter

import pytest

from test_float_sink_isa_cpu import _opcodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jpeglibrary_amd")
CSRC = os.path.join(PKG, "csrc")
FILES = ("k2_huffman.hip", "k2s_subseq.hip")
RESOURCES = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
MEMORY_AND_SYNC = ("global_load_", "global_store_", "global_atomic_", "ds_read", "ds_write", "ds_bpermute_b32", "s_barrier")
FAMILY = ("huffman_decode_kernel", "huffman_pool_kernel", "subseq_final_kernel")

# kernel -> (instructions, the RESOURCES in their order, {memory or synchronisation opcode: count})
PARENT_FAMILY = {
    "_ZN5jpgpu19huffman_pool_kernelILi10EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEjPjjPKjPNS_13DevScanStatusEPsiS2_j":
        (3500, (168, 106, 0, 33, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_add": 1, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx2": 1, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu19huffman_pool_kernelILi11EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEjPjjPKjPNS_13DevScanStatusEPsiS2_j":
        (3500, (168, 106, 0, 33, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_add": 1, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx2": 1, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu19huffman_pool_kernelILi7EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEjPjjPKjPNS_13DevScanStatusEPsiS2_j":
        (3570, (171, 106, 0, 33, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_add": 1, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx2": 1, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu19huffman_pool_kernelILi8EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEjPjjPKjPNS_13DevScanStatusEPsiS2_j":
        (3570, (167, 106, 0, 33, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_add": 1, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx2": 1, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu19huffman_pool_kernelILi9EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEjPjjPKjPNS_13DevScanStatusEPsiS2_j":
        (3500, (168, 106, 0, 33, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_add": 1, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx2": 1, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu19subseq_final_kernelILb0EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPNS_13DevScanStatusEPKNS_12DevHuffTableES2_SA_SA_PK15HIP_vector_typeIiLj4EEPsijPjSA_jj":
        (3643, (71, 70, 0, 0, 0, 0), {"ds_bpermute_b32": 22, "ds_read2_b32": 4, "ds_read_b128": 8, "ds_read_b32": 16, "ds_read_u16": 6, "ds_read_u8": 6, "ds_write2_b32": 20, "ds_write_b128": 24, "ds_write_b16": 3, "ds_write_b32": 8, "global_atomic_umax": 1, "global_atomic_umin": 1, "global_load_dword": 5, "global_load_dwordx4": 20, "global_load_ubyte": 83, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx4": 8, "s_barrier": 1}),
    "_ZN5jpgpu19subseq_final_kernelILb1EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPNS_13DevScanStatusEPKNS_12DevHuffTableES2_SA_SA_PK15HIP_vector_typeIiLj4EEPsijPjSA_jj":
        (3664, (96, 98, 0, 0, 0, 0), {"ds_bpermute_b32": 22, "ds_read2_b32": 4, "ds_read_b128": 8, "ds_read_b32": 16, "ds_read_u16": 6, "ds_read_u8": 6, "ds_write2_b32": 20, "ds_write_b128": 24, "ds_write_b16": 3, "ds_write_b32": 8, "global_atomic_add": 1, "global_atomic_umax": 1, "global_atomic_umin": 1, "global_load_dword": 5, "global_load_dwordx2": 1, "global_load_dwordx4": 20, "global_load_ubyte": 83, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx4": 8, "s_barrier": 1}),
    "_ZN5jpgpu21huffman_decode_kernelILi10EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPNS_13DevScanStatusEPKNS_12DevHuffTableEPsiS2_j":
        (3393, (151, 106, 0, 14, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu21huffman_decode_kernelILi11EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPNS_13DevScanStatusEPKNS_12DevHuffTableEPsiS2_j":
        (3393, (151, 106, 0, 14, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu21huffman_decode_kernelILi7EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPNS_13DevScanStatusEPKNS_12DevHuffTableEPsiS2_j":
        (3465, (151, 106, 0, 14, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu21huffman_decode_kernelILi8EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPNS_13DevScanStatusEPKNS_12DevHuffTableEPsiS2_j":
        (3465, (151, 106, 0, 14, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
    "_ZN5jpgpu21huffman_decode_kernelILi9EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPNS_13DevScanStatusEPKNS_12DevHuffTableEPsiS2_j":
        (3393, (151, 106, 0, 14, 0, 0), {"ds_read2_b32": 3, "ds_read_b128": 20, "ds_read_b32": 10, "ds_read_u16": 4, "ds_read_u8": 4, "ds_write2_b32": 14, "ds_write_b128": 32, "ds_write_b16": 3, "ds_write_b32": 5, "global_atomic_umax": 3, "global_atomic_umin": 2, "global_load_dword": 2, "global_load_dwordx4": 16, "global_load_ubyte": 85, "global_load_ushort": 9, "global_store_dword": 1, "global_store_dwordx2": 1, "global_store_dwordx4": 16, "s_barrier": 1}),
}
# kernel -> sha1 of its opcodes, one per line
PARENT_OTHERS = {
    "_ZN5jpgpu15lut_pool_kernelEPKNS_12DevHuffTableEPh":
        "8de9199fbdc23ee32c54e39488275d498d559df0",
    "_ZN5jpgpu18subseq_same_kernelEPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPKNS_13DevScanStatusEPjS9_":
        "f51d0631fd2400176ff9791e402b921c62179b47",
    "_ZN5jpgpu18subseq_scan_kernelEPKNS_7DevScanEPKjS4_PjPK15HIP_vector_typeIiLj4EEPS7_":
        "0e8c8020ea5810a33bc941b9d971867a4c60056e",
    "_ZN5jpgpu19sr_lut_build_kernelEPKNS_7DevScanEPKjPKhPh":
        "e2eea178383f76e94406f2b995a5ea2cf4404a1e",
    "_ZN5jpgpu19subseq_check_kernelEPjjjj":
        "8dfdbad4c66e3480ad7b568998ae4e5801f663c6",
    "_ZN5jpgpu19subseq_order_kernelEPKNS_7DevScanEPKNS_8HuffWorkEPKNS_13DevScanStatusEPKjSA_Pjj":
        "ef28b3c855431c6a89629dff1e2d6dc3d0761fa0",
    "_ZN5jpgpu19subseq_round_kernelILb0EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPKNS_13DevScanStatusEPKNS_12DevHuffTableES2_SA_PjSH_SH_P15HIP_vector_typeIiLj4EESH_iijSA_S2_":
        "bc0f878fedd79d1a2d64f339e8204b385b236fb7",
    "_ZN5jpgpu19subseq_round_kernelILb1EEEvPKhPKNS_7DevScanEPKNS_8HuffWorkEPKjPKNS_13DevScanStatusEPKNS_12DevHuffTableES2_SA_PjSH_SH_P15HIP_vector_typeIiLj4EESH_iijSA_S2_":
        "09618e4d5193d060875e9bcef3bf3aebc3e7691b",
    "_ZN5jpgpu23subseq_propagate_kernelEPKNS_7DevScanEPKjS4_PjS5_S5_P15HIP_vector_typeIiLj4EES5_S5_":
        "9e9d756d8d13f9f5e9bbbee12815a4b92c3b2501",
}


def _listing(tmp_path_factory, source):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    m = re.search(r"^CXXFLAGS\s*[:?]?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    cxxflags = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
    asm = tmp_path_factory.mktemp("isa") / (source + ".s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *[f for f in cxxflags if not f.startswith("-W")], "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, source)], stderr=subprocess.DEVNULL)
    return asm.read_text()


def _metadata(text):
    """{kernel: {field: value}} from the listing's .amdgpu_metadata (one list item at the kernels' indentation per kernel)"""
    meta = text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")]
    out = {}
    for item in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", item, re.M).group(1)
        out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, item).group(1)) for k in RESOURCES}
    return out


def _measure(text):
    """what PARENT_FAMILY and PARENT_OTHERS record, of one listing"""
    family, others = {}, {}
    for name, res in _metadata(text).items():
        ops = _opcodes(text, name)
        if any(k in name for k in FAMILY):
            family[name] = (len(ops), tuple(res[k] for k in RESOURCES), dict(sorted(Counter(op for op in ops if op.startswith(MEMORY_AND_SYNC)).items())))
        else:
            others[name] = hashlib.sha1("\n".join(ops).encode()).hexdigest()
    return family, others


@pytest.fixture(scope="module")
def measured(tmp_path_factory):
    family, others = {}, {}
    for source in FILES:
        f, o = _measure(_listing(tmp_path_factory, source))
        family.update(f)
        others.update(o)
    return family, others


@pytest.mark.timeout(900)
def test_no_instantiation_is_added_or_lost(measured):
    family, others = measured
    assert len(PARENT_FAMILY) == 12 and set(family) == set(PARENT_FAMILY), set(family) ^ set(PARENT_FAMILY)
    assert set(others) == set(PARENT_OTHERS), set(others) ^ set(PARENT_OTHERS)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kernel", sorted(PARENT_FAMILY))
def test_the_family_keeps_its_registers_its_memory_traffic_and_its_length(measured, kernel):
    total, resources, memory = measured[0][kernel]
    want_total, want_resources, want_memory = PARENT_FAMILY[kernel]
    print(kernel, "instructions", total, "parent", want_total, dict(zip(RESOURCES, resources)))
    assert dict(zip(RESOURCES, resources)) == dict(zip(RESOURCES, want_resources))  # (the VGPR count may not go DOWN either)
    assert resources[RESOURCES.index("private_segment_fixed_size")] == 0
    assert memory == want_memory, {op: (memory.get(op, 0), want_memory.get(op, 0)) for op in set(memory) | set(want_memory) if memory.get(op) != want_memory.get(op)}
    assert total * 1000 <= want_total * 1005, (total, want_total)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kernel", sorted(PARENT_OTHERS))
def test_the_other_kernels_keep_their_opcode_sequences(measured, kernel):
    assert measured[1][kernel] == PARENT_OTHERS[kernel]


def _sources(top):
    for d, _, files in os.walk(top):
        for f in files:
            if not f.endswith((".o", ".so", ".pyc")):
                yield os.path.join(d, f)


def test_each_shared_piece_exists_once():
    text = {p: open(p, errors="replace").read() for p in _sources(PKG)}
    csrc = [t for p, t in text.items() if p.startswith(CSRC + os.sep)]
    for call in ("k2_symbol<true>", "k2_symbol<false>"):
        assert sum(t.count(call) for t in csrc) == 1, call
    assert not [p for p, t in text.items() if "JPGPU_K2_TICKET_AHEAD" in t]
    assert os.path.isfile(os.path.join(ROOT, "tools", "microbench", "k2_ticket_ahead", "ticket_ahead.patch"))
    hdrs = re.search(r"^HDRS\s*=\s*(.*)$", text[os.path.join(CSRC, "Makefile")], re.M).group(1).split()
    assert "k2_wave.h" in hdrs
    including = sorted(os.path.basename(p) for p, t in text.items() if '#include "k2_wave.h"' in t)
    assert including == ["k2_huffman.hip", "k2s_subseq.hip"], including
