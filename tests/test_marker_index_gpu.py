"""K1 (jpeglibrary_amd/csrc/k1_markers.hip) byte for byte against tests/marker_index_model.py on hand-made entropy segments.

K1 is a pure function of (bytes, DRI, interval count) and chooses its code path by PLACE: classify16's interior (SWAR) lanes against
its per-byte edge lanes, the one-pass form's group tile writer against marker_write_chunk, the give-up's self-count, the three-kernel
form.  The corpus of marker_index_model puts every pattern the reference's bit reader accepts (JpegBitReader.cs:95-138) on every
edge -- lane, wave, chunk, group -- with every byte of it once on each side.  Nothing here runs K2: the segments are not Huffman data.

Compared, all exactly: udata[0 .. ulen + 2), ends[], ends_u[] and the status words n_ends, terminator, decoded_mcus, end_pos, ulen.
Nothing behind the closing entry is compared.  K1 runs twice on every upload (its tags and descriptors are never cleared).

Legs: the default wait budget (marker_fallbacks() == 0); JPGPU_K1_SPIN_BUDGET=0; the three upload routes for file bytes; the
three-kernel form in a child process (JPGPU_K1_THREE_PASS is read once per process).  Then valid files with fill bytes end to end:
first_marker_kernel's verdict, the decoders behind udata and the optimizer behind ends[]."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeglibrary_amd as jl
import marker_index_model as mm
from jpeglibrary_amd import _capi
from oracle import pyoracle as po
from tools import jpegsynth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEBUG = C.CDLL(_capi.LIB_PATH)  # (accessors for tests, not part of the C ABI of include/jpgpu.h)
_RUN_K1 = _DEBUG.jpgpu_debug_batch_run_marker_index
_RUN_K1.restype, _RUN_K1.argtypes = C.c_int, [C.c_void_p]
_INDEX = _DEBUG.jpgpu_debug_batch_marker_index
_INDEX.restype = C.c_longlong
_INDEX.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
_ONEPASS = _DEBUG.jpgpu_debug_batch_k1_onepass
_ONEPASS.restype, _ONEPASS.argtypes = C.c_int, [C.c_void_p]
HEAD = ("misalign", "data_len", "dri", "n_intervals", "total_mcus", "n_ends", "terminator", "decoded_mcus", "end_pos", "ulen")
STATUS = HEAD[5:]


@pytest.fixture(autouse=True)
def _default_budget(monkeypatch):
    monkeypatch.delenv("JPGPU_K1_SPIN_BUDGET", raising=False)


def read_index(b, i, k, case):
    """what K1 left for scan job k of image i; None where the image failed at upload or has no such job"""
    head = (C.c_uint32 * 10)()
    ends, ends_u = np.zeros(case.n_intervals, np.uint32), np.zeros(case.n_intervals, np.uint32)
    udata = np.zeros(len(case.file) + 16, np.uint8)
    rc = _INDEX(b._h, i, k, head, ends.ctypes.data, ends_u.ctypes.data, ends.size, udata.ctypes.data, udata.size)
    if rc == -1:
        return None
    got = dict(zip(HEAD, head))
    assert rc == got["n_ends"], "%s: the status K1 left does not fit the scan: %r" % (case.name, got)
    got.update(ends=ends[:rc].tolist(), ends_u=ends_u[:rc].tolist(), udata=udata[:got["ulen"] + 2].tobytes())
    return got


def differences(case, got, exp):
    """[] or one line that names the first mismatch and the instance nearest to it"""
    raw = None
    for k in STATUS:
        if got[k] != exp[k]:
            raw = exp["end_pos"]
            what = "%s %d, model %d" % (k, got[k], exp[k])
            break
    else:
        for name in ("ends", "ends_u"):
            bad = [j for j in range(exp["n_ends"]) if got[name][j] != exp[name][j]]
            if bad:
                raw, what = exp["ends"][bad[0]], "%s[%d] %d, model %d (%d entries differ)" % (name, bad[0], got[name][bad[0]], exp[name][bad[0]], len(bad))
                break
        else:
            if got["udata"] == exp["udata"]:
                return []
            g, e = np.frombuffer(got["udata"], np.uint8), np.frombuffer(exp["udata"], np.uint8)
            u = int(np.flatnonzero(g != e)[0])
            raw, what = mm.raw_position(exp["marks"], u), "udata[%d] %02x, model %02x (%d bytes differ)" % (u, g[u], e[u], int((g != e).sum()))
    return ["%s: %s; raw offset %d = %d from the aligned base; nearest instance %r" % (case.name, what, raw, raw + got["misalign"], case.instance_near(raw))]


def plain_upload(b, cases):
    """an upload route: uploads the cases' files, returns (data_off & 15 intended for each, what to call when the batch is done with them)"""
    b.upload([c.file for c in cases])
    return [c.misalign for c in cases], None


def batches(cases, max_bytes=12 << 20, max_files=600):
    cur, size = [], 0
    for c in cases:
        if cur and (size + len(c.file) > max_bytes or len(cur) >= max_files):
            yield cur
            cur, size = [], 0
        cur.append(c)
        size += len(c.file)
    if cur:
        yield cur


def check(cases, upload=plain_upload):
    """uploads the cases many files per batch, runs K1 twice on every upload and compares both runs with the model; returns the
    batch's count of give-ups"""
    b = jl.Batch()
    bad, n_compared = [], 0
    for c in cases:
        c.check_instances()  # (on the CPU, before the upload)
    for group in batches(cases):
        misalign, release = upload(b, group)
        try:
            bad, n_compared = _compare_group(b, group, misalign, bad, n_compared)
        finally:
            if release:
                release()
    assert not bad, "%d of %d comparisons differ:\n%s" % (len(bad), n_compared, "\n".join(bad[:12]))
    fallbacks = b.marker_fallbacks()
    b.close()
    return fallbacks


def _compare_group(b, group, misalign, bad, n_compared):
    """K1 twice on the upload, both runs against the model"""
    for run in range(2):
        assert _RUN_K1(b._h) == 0, b.ctx.last_error()
        for i, c in enumerate(group):
            status = b.image_info(i).status
            if not c.identify_ok:  # Identify() throws on these bytes: no scan job, K1 has nothing to index
                assert status != 0 and read_index(b, i, 0, c) is None, c.name
                continue
            assert status == 0, (c.name, status)
            for k in range(c.jobs):
                got, exp = read_index(b, i, k, c), mm.expected(c, k)
                assert got is not None, (c.name, k)
                want = dict(dri=c.dri, n_intervals=c.n_intervals, total_mcus=c.total_mcus)
                if k == 0:
                    want.update(misalign=misalign[i], data_len=len(c.file) - c.data_pos)
                assert {x: got[x] for x in want} == want, (c.name, k, got, want)
                bad += ["run %d job %d: %s" % (run, k, d) for d in differences(c, got, exp)]
                n_compared += 1
            assert read_index(b, i, c.jobs, c) is None, c.name  # no such job
    return bad, n_compared


# ------------------------------------------------------------------------------------------------ the direct legs

@pytest.mark.parametrize("family", mm.FAMILIES)
def test_marker_index_equals_the_model(family):
    assert check(mm.family(family)) == 0  # (no group ran out of patience)


@pytest.mark.parametrize("family", mm.FAMILIES)
def test_marker_index_without_patience_equals_the_model(family, monkeypatch):
    """a spin budget of zero (read per call): a group that finds a predecessor's record missing counts the chunks in front of it
    itself -- the same index whatever the counter says"""
    monkeypatch.setenv("JPGPU_K1_SPIN_BUDGET", "0")
    check(mm.family(family))


def test_long_segment_beside_two_hundred_short_ones(monkeypatch):
    """the scan-interleaved order list: the 70 groups of the long segment among the single groups of 200 short files"""
    short = mm.family("heads")[::4][:200]
    assert len(short) == 200
    cases = short[:100] + [mm.long_case()] + short[100:]
    assert check(cases) == 0
    monkeypatch.setenv("JPGPU_K1_SPIN_BUDGET", "0")
    check(cases)


def _arena_upload(b, cases):
    """one page-locked arena, file i at a place of its own modulo 16: the device copy mirrors the arena's layout"""
    pos, at = 0, []
    for i, c in enumerate(cases):
        at.append(pos)
        pos = (pos + len(c.file) + 63) // 64 * 64 + (i + 1) * 5 % 16
    ctx = b.ctx
    arena = ctx.host_alloc(pos + 64)
    try:
        assert arena.ctypes.data % 16 == 0
        arena[:] = np.frombuffer(b"\xff\xd9\xff\xda\xff\x00\xff\xd0\xff\xff\x00" * (arena.size // 11 + 1), np.uint8)[:arena.size]  # marker look-alikes in the gaps
        views = []
        for c, p in zip(cases, at):
            arena[p:p + len(c.file)] = np.frombuffer(c.file, np.uint8)
            views.append(arena[p:p + len(c.file)])
        b.upload_segments(views, jl.FMT_INTERLEAVED_U8, arena=True)
        assert b.ingest_stats()["n_pinned_dma"] >= 1
    except BaseException:
        ctx.host_free(arena)
        raise
    # (a segment starts where its file lies in the arena; the arena goes back to the context that gave it when the batch is done with it)
    return [(p + c.misalign) % 16 for c, p in zip(cases, at)], lambda: ctx.host_free(arena)


def _tensor_upload(b, cases):
    """files in device memory: views into one tensor (one copy to the device), every file at a place of its own modulo 16"""
    import torch

    pos, at = 0, []
    for i, c in enumerate(cases):
        at.append(pos)
        pos += len(c.file) + (i * 3 + 1) % 16
    host = np.zeros(pos, np.uint8)
    for c, p in zip(cases, at):
        host[p:p + len(c.file)] = np.frombuffer(c.file, np.uint8)
    dev = torch.from_numpy(host).to(torch.device("cuda", b.ctx.device))
    b.upload_tensors([dev[p:p + len(c.file)] for c, p in zip(cases, at)])
    return [c.misalign for c in cases], None  # (the batch's own copy of a file starts at a multiple of 16)


@pytest.mark.parametrize("route", ["upload", "arena", "tensors"])
def test_marker_index_behind_every_upload_route(route):
    """the routes file bytes take to the device change where a segment starts: the heads, at all 16 alignments, behind each"""
    assert check(mm.family("heads"), {"upload": plain_upload, "arena": _arena_upload, "tensors": _tensor_upload}[route]) == 0


# ------------------------------------------------------------------------------------------------ the three-kernel form

def _onepass_here():
    b = jl.Batch().upload([mm.family("heads")[0].file])
    on = _ONEPASS(b._h)
    b.close()
    return on


def _three_pass_child():
    assert _onepass_here() == 0, "JPGPU_K1_THREE_PASS=1 did not select the three-kernel form"
    cases = mm.corpus()
    for fam in mm.FAMILIES:
        check(mm.family(fam))
    print("K1FORM three_pass cases %d" % len(cases))


def test_three_kernel_form_equals_the_model_in_a_child_process():
    """marker_count_kernel / marker_prefix_kernel / marker_write_kernel on the whole corpus.  JPGPU_K1_THREE_PASS is read once per
    process: a child of its own, which asserts that the one-pass form is off"""
    assert _onepass_here() == 1  # (here it is on)
    env = dict(os.environ, JPGPU_K1_THREE_PASS="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    env.pop("JPGPU_K1_SPIN_BUDGET", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "three_pass"], env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("K1FORM ")]
    assert r.returncode == 0 and lines == ["K1FORM three_pass cases %d" % len(mm.corpus())], r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ end to end, on valid files

E2E_SHAPES = ((512, 384, "420", 98, 1), (448, 320, "444", 95, 0), (496, 352, "422", 96, 3))
OPTIMIZER_SHAPES = E2E_SHAPES[1:]  # (the oracle's optimizer refuses the 4:2:0 Q98 DRI 1 original)


@functools.lru_cache(maxsize=None)
def _e2e_files():
    plain = [bytes(jpegsynth.encode(w, h, ss, q, dri, seed=900 + k)) for k, (w, h, ss, q, dri) in enumerate(E2E_SHAPES)]
    return plain, [mm.insert_fill(f, 40 + k) for k, f in enumerate(plain)]


def test_fill_bytes_in_valid_files_change_nothing_end_to_end():
    """runs of 1-40 FF in front of stuffed bytes, RSTs and the EOI: the same samples as the oracle's for the edited file and as the
    unedited file's, planned from the headers alone (fill in front of EOI does not change first_marker_kernel's verdict)"""
    plain, edited = _e2e_files()
    for f, e in zip(plain, edited):  # (on the CPU: fill in many places, and in front of the EOI of every file)
        assert len(e) > len(f) + 500 and e.endswith(b"\xff\xff\xd9") and f.endswith(b"\xff\xd9") and not f.endswith(b"\xff\xff\xd9")
    b = jl.Batch().upload(edited + plain, jl.FMT_INTERLEAVED_U8)
    st = b.ingest_stats()
    assert st["n_full_walk"] == 0, st
    for _ in range(2):
        b.decode().sync()
        for i, e in enumerate(edited):
            ref, _ = po.decode_8bit(e)
            assert b.result(i).status == 0 and b.result(i + 3).status == 0, i
            assert np.array_equal(b.output(i), ref), i
            assert np.array_equal(b.output(i), b.output(i + 3)), i
    assert b.marker_fallbacks() == 0
    b.close()


def test_optimizer_reads_the_raw_offsets_of_files_with_fill():
    """ends[] (raw offsets) is read by the transcode kernels alone: optimize_batch of the edited files gives the oracle's bytes"""
    plain, edited = _e2e_files()
    assert all(e.endswith(b"\xff\xff\xd9") for e in edited)
    want = []
    for k in (1, 2):
        ref = po.optimize(plain[k], False)  # (on the CPU: the oracle succeeds on the unedited file ...)
        assert po.optimize(edited[k], False) == ref  # (... and fill changes nothing for it)
        want.append(ref)
    assert jl.optimize_batch([edited[1], edited[2]], strip=False) == want
    assert jl.optimize_batch([plain[1], plain[2]], strip=False) == want


if __name__ == "__main__":
    {"three_pass": _three_pass_child}[sys.argv[1]]()
