"""The quad exchange in the listing of K3's headline kernels, checked without a GPU: in idct_output_kernel<INTERLEAVED_U8, 4:2:0> and its
split form the task loop (`Depth=2`) exchanges 16-byte pieces between the lanes of a quad with selected quad_perm DPP moves -- one
v_cndmask_b32_dpp each, two per output dword, 24 per trip -- and no other cross-lane operation; its instructions per trip are pinned to what
the finished listing gives (the parent commit's: 60 dense / 61 split), and both kernels keep three waves on a SIMD."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")

DENSE = "_ZN5jpgpu18idct_output_kernelILi0ELi3EEE"  # INTERLEAVED_U8, 4:2:0, dense blocks
SPLIT = "_ZN5jpgpu17idct_split_kernelILi0ELi3EEE"   # ... half-line planes
# per trip of the task loop: the parent's 60 / 61 + 24 selected moves + 4 s_mov_b64 of the lane masks + the wait states in front of the first
# DPP read (one s_nop) + the second and third store's own lane offsets (2 or 3 v_add_u32, a wait state the compiler places between them)
TRIP_AT_MOST = {DENSE: 93, SPLIT: 94}
SELECTED_MOVES = 24

_LABEL = re.compile(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)")


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


def _task_loop(text, mangled_prefix):
    """the whole lines of the kernel's instructions in basic blocks of loop depth 2, in the listing's order"""
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    lines = lines[start + 1:end + 1]
    out, depth = [], 0
    for i, ln in enumerate(lines):
        if _LABEL.match(ln):
            notes, j = ln, i + 1
            while j < len(lines) and lines[j].lstrip().startswith(";") and not _LABEL.match(lines[j]) and "ASM" not in lines[j]:
                notes += lines[j]
                j += 1
            depths = [int(d) for d in re.findall(r"Depth=(\d+)", notes)]
            depth = max(depths) if depths else 0
            continue
        s = ln.strip()
        if not s or s.startswith(";") or s.startswith(".") or s.endswith(":"):
            continue
        if depth == 2:
            out.append(s)
    return out


def _resources(text, mangled_prefix):
    names = re.findall(r"\.name:\s+(\S+)", text)
    field = lambda key: dict(zip(names, (int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, text))))
    (name,) = [n for n in names if n.startswith(mangled_prefix)]
    return {k: field(k)[name] for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kernel", [DENSE, SPLIT], ids=["dense", "split"])
def test_the_task_loop_exchanges_pieces_with_selected_quad_perm_moves(isa, kernel):
    loop = _task_loop(isa, kernel)
    assert loop, "no loop of depth 2"
    dpp = [ln for ln in loop if "quad_perm:" in ln]
    assert len(dpp) == SELECTED_MOVES, dpp
    assert all(ln.startswith("v_cndmask_b32_dpp") and "row_mask:0xf" in ln and "bank_mask:0xf" in ln and "bound_ctrl" in ln for ln in dpp), dpp
    # nothing else crosses lanes: no other DPP control, no LDS permute, no lane read
    assert not any(re.search(r"row_(shl|shr|ror|bcast|mirror|half_mirror)|wave_(shl|shr|rol|ror)", ln) for ln in loop), loop
    assert not any(ln.split()[0].startswith(("ds_bpermute", "ds_permute", "ds_swizzle", "v_readlane", "v_writelane", "v_readfirstlane")) for ln in loop), loop
    # the wait states a DPP read needs behind a vector write of its source are in front of the first one
    first = loop.index(dpp[0])
    assert any(ln.startswith("s_nop") for ln in loop[max(0, first - 3):first]), loop[max(0, first - 3):first]
    # the moves lie between the byte permutes and the stores
    last_perm = max(i for i, ln in enumerate(loop) if ln.startswith("v_perm_b32"))
    first_store = min(i for i, ln in enumerate(loop) if ln.startswith("global_store_dwordx4"))
    assert last_perm < first and loop.index(dpp[-1]) < first_store, (last_perm, first, first_store)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kernel", [DENSE, SPLIT], ids=["dense", "split"])
def test_the_trip_is_no_longer_than_the_listing_s(isa, kernel):
    loop = _task_loop(isa, kernel)
    assert len(loop) <= TRIP_AT_MOST[kernel], (len(loop), loop)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kernel", [DENSE, SPLIT], ids=["dense", "split"])
def test_both_forms_keep_three_waves_per_simd(isa, kernel):
    r = _resources(isa, kernel)
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 168, r
