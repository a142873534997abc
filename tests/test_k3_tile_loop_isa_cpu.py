"""The ISA of K3's tile loop on the headline's path, checked without a GPU: in idct_output_kernel<INTERLEAVED_U8, 4:2:0> and its split
form the output assembly's task loop (the one loop nested in the tile loop: `Depth=2` in the listing) holds no full 32-bit multiply,
no 64-bit multiply-add, no division set-up and no fetch of the frame's width or height; the split form looks a tile's flags up once
per staging block.

The flag look-ups are counted by their byte loads against the parent commit's listing of idct_split_kernel<0, 3>: 29
global_load_ubyte (three look-up sites of eight loads each, and the five byte loads of the scan descriptor the dense form has too).
At most a quarter of that may remain; the look-ups themselves are the byte loads the split form has beyond the dense form's
(24 in the parent, at most a quarter of those too).  No wait on vmcnt lies between the task loop's stores and the wait for the next
tile's DMA: the stores drain under the next tile's transform.  Both kernels keep three waves on a SIMD: at most 168 VGPRs, no spill,
no scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")

DENSE = "_ZN5jpgpu18idct_output_kernelILi0ELi3EEE"  # INTERLEAVED_U8, 4:2:0, dense blocks
SPLIT = "_ZN5jpgpu17idct_split_kernelILi0ELi3EEE"   # ... half-line planes
PARENT_SPLIT_BYTE_LOADS = 29
PARENT_DENSE_BYTE_LOADS = 5  # idct_output_kernel<0, 3> of the parent: the scan descriptor's bytes

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


def _resources(text, mangled_prefix):
    names = re.findall(r"\.name:\s+(\S+)", text)
    field = lambda key: dict(zip(names, (int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, text))))
    (name,) = [n for n in names if n.startswith(mangled_prefix)]
    return {k: field(k)[name] for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}


def _kernel_lines(text, mangled_prefix):
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start + 1:end + 1]


def _opcode(ln):
    return re.sub(r"_(e32|e64|sdwa|dpp)$", "", ln.split()[0])


def _instructions_by_depth(text, mangled_prefix, whole_lines=False, tile_only=False):
    """[(loop depth of the basic block, opcode or whole line)] of a kernel, in the listing's order; the depth is what the listing's block
    comments say (none: 0)"""
    out, depth, lines = [], 0, _kernel_lines(text, mangled_prefix)
    tile_loop_at = None  # the first instruction of the loop header that has a child loop
    for i, ln in enumerate(lines):
        if _LABEL.match(ln):
            notes, j = ln, i + 1
            while j < len(lines) and lines[j].lstrip().startswith(";") and not _LABEL.match(lines[j]) and "ASM" not in lines[j]:
                notes += lines[j]
                j += 1
            depths = [int(d) for d in re.findall(r"Depth=(\d+)", notes)]
            depth = max(depths) if depths else 0
            if "Child Loop" in notes and tile_loop_at is None:
                tile_loop_at = len(out)
            continue
        s = ln.strip()
        if not s or s.startswith(";") or s.startswith(".") or s.endswith(":"):
            continue
        out.append((depth, s if whole_lines else _opcode(s)))
    if tile_only:
        # the tile loop: the one loop with a loop inside it (the split form has a small loop of its own in front of it), with the blocks
        # of it that the listing puts in front of its header; the task loop is the last thing in the listing
        start = tile_loop_at
        while start > 0 and out[start - 1][0] >= 1:
            start -= 1
        assert all(d >= 1 for d, _ in out[start:-1]), "the tile loop runs to the end of the listing"
        return out[start:-1]  # (without s_endpgm)
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kernel", [DENSE, SPLIT], ids=["dense", "split"])
def test_the_task_loop_neither_divides_nor_multiplies_in_full(isa, kernel):
    ins = _instructions_by_depth(isa, kernel)
    assert max(d for d, _ in ins) == 2  # (the tile loop and the task loop in it; nothing deeper)
    loop = [op for d, op in ins if d == 2]
    # it is the output assembly: two LDS reads, the byte permutes, three 16-byte stores per task
    assert loop.count("ds_read_b128") == 2 and loop.count("global_store_dwordx4") == 3 and loop.count("v_perm_b32") >= 16, loop
    for op in ("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_rcp_iflag_f32", "global_load_ushort"):
        assert op not in loop, (op, loop)
    assert not any(op.startswith(("global_load", "s_load", "v_rcp", "v_div")) for op in loop), loop


@pytest.mark.timeout(600)
def test_the_split_form_looks_a_tile_s_flags_up_once_per_staging_block(isa):
    ops = [op for _, op in _instructions_by_depth(isa, SPLIT)]
    assert ops.count("global_load_ubyte") <= PARENT_SPLIT_BYTE_LOADS // 4, ops.count("global_load_ubyte")
    # the look-ups apart from the scan descriptor's bytes, which the dense form loads too: 29 - 5 = 24 in the parent
    dense = [op for _, op in _instructions_by_depth(isa, DENSE)].count("global_load_ubyte")
    assert 0 < ops.count("global_load_ubyte") - dense <= (PARENT_SPLIT_BYTE_LOADS - PARENT_DENSE_BYTE_LOADS) // 4
    in_tile_loop = lambda k: [op for _, op in _instructions_by_depth(isa, k, tile_only=True)].count("global_load_ubyte")
    assert in_tile_loop(SPLIT) - in_tile_loop(DENSE) == 1  # one look-up a tile


def _is_vm_wait(line):
    return line.startswith("s_waitcnt") and "vmcnt" in line


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kernel", [DENSE, SPLIT], ids=["dense", "split"])
def test_a_tile_s_stores_are_not_waited_for_before_the_next_tile_s_dma_wait(isa, kernel):
    """vmcnt retires in order: a wait on it behind the task loop, or at the head of the next tile, is a wait for the tile's own output
    stores.  In the listing's order the tile loop is: head (dequantisation) -- barrier -- DMA, transform -- the wait for the DMA --
    barrier -- task loop (last).  Every vmcnt wait of the tile loop lies between its two barriers."""
    tile = [ln for _, ln in _instructions_by_depth(isa, kernel, whole_lines=True, tile_only=True)]
    depth = [d for d, _ in _instructions_by_depth(isa, kernel, whole_lines=True, tile_only=True)]
    barriers = [i for i, ln in enumerate(tile) if ln.startswith("s_barrier")]
    stores = [i for i, ln in enumerate(tile) if ln.startswith("global_store_dwordx4") and depth[i] == 2]
    assert len(barriers) == 2 and len(stores) == 3 and barriers[1] < stores[0], (barriers, stores)
    waits = [i for i, ln in enumerate(tile) if _is_vm_wait(ln)]
    assert waits and all(barriers[0] < i < barriers[1] for i in waits), [(i, tile[i]) for i in waits]
    assert any(ln.startswith("global_load_lds_dwordx4") for ln in tile[barriers[0]:waits[0]])  # (it is the DMA's wait)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kernel", [DENSE, SPLIT], ids=["dense", "split"])
def test_both_forms_keep_three_waves_per_simd(isa, kernel):
    r = _resources(isa, kernel)
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 168, r
