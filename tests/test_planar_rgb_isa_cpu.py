"""The listing of K3's RGB_PLANAR_U8 instantiations, checked without a GPU: idct_output_kernel<7, class> and idct_split_kernel<7, class> for
the four fast layout classes (1 = 4:4:4, 2 = 4:2:2, 3 = 4:2:0, 4 = gray).  None spills or uses scratch, each stays within the 168 VGPRs that
three waves per SIMD allow (their __launch_bounds__), and the task loop (`Depth=2`: the one loop nested in the tile loop) ends in exactly three
stores, one per plane -- 16 bytes each where an MCU is two blocks wide, 8 bytes each where it is one -- and never in byte or short stores."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jpeglibrary_amd", "csrc")

FMT_RGB_PLANAR_U8 = 7
CLASSES = {1: "global_store_dwordx2", 2: "global_store_dwordx4", 3: "global_store_dwordx4", 4: "global_store_dwordx2"}  # layout class -> its store
KERNELS = {"dense": "_ZN5jpgpu18idct_output_kernelILi%dELi%dEEE", "split": "_ZN5jpgpu17idct_split_kernelILi%dELi%dEEE"}
CASES = [(form, cls) for cls in CLASSES for form in KERNELS]

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


def _name(form, cls):
    return KERNELS[form] % (FMT_RGB_PLANAR_U8, cls)


def _task_loop(text, mangled_prefix):
    """the opcodes of the kernel's instructions in basic blocks of loop depth 2, in the listing's order"""
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(mangled_prefix) and ln.split(";")[0].strip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    lines = lines[start + 1:end + 1]
    out, depth, deepest = [], 0, 0
    for i, ln in enumerate(lines):
        if _LABEL.match(ln):
            notes, j = ln, i + 1
            while j < len(lines) and lines[j].lstrip().startswith(";") and not _LABEL.match(lines[j]) and "ASM" not in lines[j]:
                notes += lines[j]
                j += 1
            depths = [int(d) for d in re.findall(r"Depth=(\d+)", notes)]
            depth = max(depths) if depths else 0
            deepest = max(deepest, depth)
            continue
        s = ln.strip()
        if not s or s.startswith(";") or s.startswith(".") or s.endswith(":"):
            continue
        if depth == 2:
            out.append(re.sub(r"_(e32|e64|sdwa|dpp)$", "", s.split()[0]))
    assert deepest == 2, deepest  # (the tile loop and the task loop in it; nothing deeper)
    return out


def _resources(text, mangled_prefix):
    names = re.findall(r"\.name:\s+(\S+)", text)
    field = lambda key: dict(zip(names, (int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, text))))
    (name,) = [n for n in names if n.startswith(mangled_prefix)]
    return {k: field(k)[name] for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("form,cls", CASES, ids=["%s-class%d" % c for c in CASES])
def test_every_instantiation_keeps_three_waves_per_simd_without_spill_or_scratch(isa, form, cls):
    r = _resources(isa, _name(form, cls))
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 168, r


@pytest.mark.timeout(600)
@pytest.mark.parametrize("form,cls", CASES, ids=["%s-class%d" % c for c in CASES])
def test_the_task_loop_ends_in_three_stores_one_per_plane(isa, form, cls):
    loop = _task_loop(isa, _name(form, cls))
    assert loop, "no loop of depth 2"
    stores = [op for op in loop if op.startswith(("global_store", "flat_store"))]
    assert stores == [CLASSES[cls]] * 3, stores
    assert not any(op.startswith(("global_store_byte", "global_store_short")) for op in loop), loop
    if cls != 4:  # the channels are gathered with byte permutes, three per dword stored (a gray pixel is its sample in all three planes)
        assert loop.count("v_perm_b32") >= 3 * 3 * (4 if CLASSES[cls].endswith("x4") else 2), loop
