"""The progressive decoder (k2p_progressive.hip and the planner in front of it) on scan scripts no encoder of this tree emits.

The inputs are the catalogue of tests/progscript.py, written at test time from fixed seeds; tests/test_progressive_scripts_cpu.py
shows without a GPU that the checker's store for every one of them equals the numbers the file was made from, and that libjpeg
reads them.  Everything compared here is an integer, every comparison is exact:

  * status and detail string against the checker's;
  * INTERLEAVED_U8 against the checker's buffer (of a failing file: what its partial flush leaves), RGBA_U8 of three-component
    files against the reference callers' colour step on it, EXTENDED_U16 of three entries against the 16-bit sink;
  * the coefficient store behind the entropy stage against expected_store on EVERY block of every component -- the components
    Dispose() never transforms included, which the checker's tap does not report -- and zero outside a component's grid.

Every regime asserts through Batch.progressive_plan() that the launches it is named for were the ones taken.
"""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import jpeglibrary_amd as jl
import progscript as ps
from golden_util import read_jpeg
from jpeglibrary_amd import _capi
from oracle import pyoracle as po
from tools import jpegsynth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(ps.CATALOGUE)
CLEAN = [n for n in NAMES if ps.CATALOGUE[n].outcome == ps.CLEAN]
STATUS_NAMES = {0: "OK", 1: "InvalidDataException", 2: "InvalidOperationException", 3: "NotSupportedException"}
PLANNER_ENV = ("JPGPU_PROG_NO_PIPELINE", "JPGPU_PROG_NO_CHAINS", "JPGPU_PROG_STREAM_MAX_INTERVALS", "JPGPU_PROG_FORCE_PIPELINE",
               "JPGPU_DEBUG_DELAY_SCAN", "JPGPU_PROG_BY_SCAN", "JPGPU_DEBUG_MAX_PROGRESSIVE_SCANS", "JPGPU_PROG_SPIN_BUDGET")


@pytest.fixture(autouse=True)
def _planner_defaults(monkeypatch):
    """(the suite is also run under the A/B switches: every test here names the ones it wants)"""
    for k in PLANNER_ENV:
        monkeypatch.delenv(k, raising=False)


class Ref:
    def __init__(self, name, data, outcome, store):
        self.name, self.data, self.outcome, self.store = name, data, outcome, store
        self.out8, self.info, err = po.decode_8bit_partial(data)
        assert (ps.CLEAN if err is None else (err.kind, err.message)) == outcome, (name, err)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    b = ps.build(name)
    e = b.entry
    return Ref(name, b.data, e.outcome, ps.store_in_mcu_order(b.expected, e.comps, e.width, e.height))


@functools.lru_cache(maxsize=None)
def foreign_files():
    """a reference golden (libjpeg's script), the synthetic generator's script and a baseline file"""
    out = []
    for tag, data in (("progress.jpg", read_jpeg("progress.jpg")), ("jpegsynth_progressive", bytes(jpegsynth.encode(136, 88, "420", 80, 0, seed=7, progressive=True))),
                      ("jpegsynth_baseline", bytes(jpegsynth.encode(96, 64, "420", 75, 2, seed=5)))):
        r = Ref.__new__(Ref)
        r.name, r.data, r.outcome, r.store = tag, data, ps.CLEAN, None
        r.out8, r.info = po.decode_8bit(data)
        out.append(r)
    return out


def check_statuses_and_samples(b, refs, fmt=jl.FMT_INTERLEAVED_U8):
    bad = []
    for i, r in enumerate(refs):
        res = b.result(i)
        if r.outcome == ps.CLEAN:
            if res.status != 0:
                bad.append((r.name, "status", STATUS_NAMES.get(res.status, res.status), _capi.lib.jpgpu_detail_string(res.detail).decode()))
                continue
        elif (STATUS_NAMES.get(res.status), _capi.lib.jpgpu_detail_string(res.detail).decode()) != r.outcome:
            bad.append((r.name, "status", res.status, _capi.lib.jpgpu_detail_string(res.detail).decode(), r.outcome))
            continue
        if fmt == jl.FMT_INTERLEAVED_U8:
            want = r.out8
        elif fmt == jl.FMT_RGBA_U8:
            want = po.ycbcr8_to_rgb(r.out8, rgba=True)
        else:
            want = po.decode_16bit(r.data)[0]
        got = b.output(i)
        if got.shape != want.shape or not np.array_equal(got, want):
            where = np.argwhere((got != want).any(axis=2))[:1].tolist() if got.shape == want.shape else got.shape
            bad.append((r.name, "samples", int((got != want).sum()) if got.shape == want.shape else -1, where))
    assert not bad, bad


def check_stores(b, refs):
    """the store behind the entropy stage: every block of every component, and zero outside the components' grids"""
    bad = []
    for i, r in enumerate(refs):
        if r.store is None or r.outcome != ps.CLEAN:
            continue
        got = b.coefficients(i)
        if got.shape != r.store.shape:
            bad.append((r.name, got.shape, r.store.shape))
        elif not np.array_equal(got, r.store):
            blocks = np.argwhere((got != r.store).any(axis=1)).reshape(-1)
            k = int(blocks[0])
            bad.append((r.name, len(blocks), k, np.argwhere(got[k] != r.store[k]).reshape(-1)[:6].tolist(), got[k][got[k] != r.store[k]][:6].tolist(),
                        r.store[k][got[k] != r.store[k]][:6].tolist()))
    assert not bad, bad


def expected_form(plan):
    """the launches run_progressive() takes for a plan that fits the machine, by default"""
    return "pipelined_gated" if plan["pipelined"] else "chains" if plan["chains_ok"] else "by_level"


def decode_and_check(refs, fmt=jl.FMT_INTERLEAVED_U8, stores=True, decodes=1):
    """upload -> (entropy stage alone, store compared) -> decode() x decodes, statuses and samples compared each time.
    Returns (plan behind the upload, plan behind the last decode)."""
    b = jl.Batch().upload([r.data for r in refs], fmt)
    planned = b.progressive_plan()
    assert planned["launch_form"] == "none"
    if stores:
        b.run_entropy().sync()
        check_stores(b, refs)
    for _ in range(decodes):
        b.decode().sync()
        check_statuses_and_samples(b, refs, fmt)
    done = b.progressive_plan()
    assert b.progressive_fallbacks() == 0
    b.close()
    return planned, done


# ----------------------------------------------------------------------------------------------- regime 1: one file per batch

def has_restart_intervals(name):
    """(every catalogue script with a DRI has scans of several intervals, and one of more than 16)"""
    return any(sc.dri for sc in ps.CATALOGUE[name].script)


def pipelinable(name):
    """one pipelined launch: every scan a single stream with at most three direct producers"""
    return not has_restart_intervals(name) and ps.planner_model(ps.CATALOGUE[name].script)["max_deps"] <= 3


# what the entries are in the catalogue for, beyond what planner_model says of every one of them
PLAN_FACTS = {
    # 64 scans: the last count the dependency bookkeeping covers -- still one pipelined launch, band k behind band k - 1
    "gray_single_coefficient_bands": lambda p: p["pipelined"] and p["levels"] == 63 and p["max_deps"] == 1 and p["launch_form"] == "pipelined_gated",
    "gray_single_bands_refined": lambda p: not p["pipelined"] and p["max_deps"] >= 4 and p["levels"] == 126 and p["launch_form"] == "chains",
    "gray_deep_sa": lambda p: p["pipelined"] and p["levels"] == 7,
    "precision8_al13": lambda p: p["pipelined"] and p["levels"] == 14,
    # contiguous bands follow each other (a first pass may write up to Se + 15): one direct producer, one more level per band
    "three_bands_then_refinement": lambda p: p["pipelined"] and p["max_deps"] == 1 and p["levels"] == 4,
    "five_bands_then_one_refinement": lambda p: p["pipelined"] and p["max_deps"] == 1 and p["levels"] == 6,
    # bands more than 15 coefficients apart do not: all three dependency words of the refinement live / one too many
    "three_separate_bands_then_refinement": lambda p: p["pipelined"] and p["max_deps"] == 3 and p["levels"] == 2 and p["launch_form"] == "pipelined_gated",
    "four_separate_bands_then_refinement": lambda p: not p["pipelined"] and p["max_deps"] == 4 and p["chains_ok"] and p["launch_form"] == "chains",
    "dc_three_producers": lambda p: p["pipelined"] and p["max_deps"] == 3 and p["launch_form"] == "pipelined_gated",
    "shared_tables_ids_0_to_3": lambda p: not p["pipelined"] and p["max_deps"] == 4 and p["launch_form"] == "chains",
    "dri_changes_between_scans": lambda p: p["lane_work"] > 0 and not p["pipelined"] and not p["chains_ok"] and p["launch_form"] == "by_level",
    "cmyk": lambda p: all(n > 0 for n in p["chain_scans"]) and p["launch_form"] == "pipelined_gated",
    "eob_run_over_32767": lambda p: p["pipelined"] and p["levels"] == 3 and p["launch_form"] == "pipelined_gated",
    "dc_only": lambda p: p["scans"] == 1 and p["levels"] == 1 and p["chain_scans"] == [1, 0, 0, 0, 0],
}


@pytest.mark.parametrize("name", NAMES)
def test_entry_in_a_batch_of_its_own(name):
    """default plan: statuses, samples in every layout the entry has, the store, three decode() calls in a row (the store is
    cleared each time), and the plan: the planner's rule restated (progscript.planner_model) and what the entry is there for"""
    r = ref_of(name)
    e = ps.CATALOGUE[name]
    planned, done = decode_and_check([r], decodes=3)
    if r.outcome == ps.CLEAN:
        m = ps.planner_model(e.script)
        assert {k: planned[k] for k in ("scans", "levels", "max_deps")} == {k: m[k] for k in ("scans", "levels", "max_deps")}, (planned, m)
        assert planned["pipelined"] == pipelinable(name) and planned["chains_ok"] == (not has_restart_intervals(name)), planned
        if has_restart_intervals(name):
            assert planned["lane_work"] > 0 and sum(planned["chain_scans"]) < planned["scans"], planned
        else:
            assert planned["chain_scans"] == m["chain_scans"] and planned["lane_work"] == 0, (planned, m)
            assert planned["pipe_waves"] + planned["wave_tails"] == planned["scans"], planned
        assert done["launch_form"] == expected_form(planned), (planned, done)
        assert dict(done, launch_form="none") == planned  # a clean decode leaves the plan as the upload made it
        if name in PLAN_FACTS:
            assert PLAN_FACTS[name](done), done
    if len(e.comps) == 3 and r.outcome == ps.CLEAN:  # (RGBA of a failing file is not defined: the reference's callers convert after a clean decode)
        decode_and_check([r], jl.FMT_RGBA_U8, stores=False)
    if name in ps.EXTENDED_U16_ENTRIES:
        decode_and_check([r], jl.FMT_EXTENDED_U16, stores=False)


def test_every_plan_fact_names_a_catalogue_entry():
    assert set(PLAN_FACTS) <= set(CLEAN) and set(ps.EXTENDED_U16_ENTRIES) <= set(CLEAN)


# ------------------------------------------------------------------------------------------------ regime 2: unlike scripts side by side

@functools.lru_cache(maxsize=None)
def pipelined_alone():
    """the entries whose own plan is pipelined (asked of the planner, one upload each)"""
    out = []
    for n in CLEAN:
        b = jl.Batch().upload([ref_of(n).data])
        if b.progressive_plan()["pipelined"]:
            out.append(n)
        b.close()
    return out


@pytest.mark.parametrize("order", ["catalogue_order", "reversed"])
def test_whole_catalogue_in_one_batch(order):
    """ordinals, chains and table slots of unlike scripts side by side, with libjpeg's script, the generator's and a baseline
    file between them.  One entry that cannot be pipelined makes the whole batch's plan unpipelined."""
    refs = [ref_of(n) for n in NAMES] + foreign_files()
    if order == "reversed":
        refs = refs[::-1]
    planned, _ = decode_and_check(refs, decodes=3)
    assert not planned["pipelined"] and not planned["chains_ok"] and planned["lane_work"] > 0
    foreign_scans = sum(r.data.count(b"\xff\xda") for r in foreign_files()[:2])
    assert foreign_scans == 10 + 8  # libjpeg's script, the generator's
    assert planned["scans"] == sum(len(ps.CATALOGUE[n].script) for n in NAMES) + foreign_scans
    assert planned["levels"] == 126 and planned["max_deps"] == 6  # the 128-scan file
    decode_and_check([r for r in refs if r.out8.shape[2] == 3 and r.outcome == ps.CLEAN], jl.FMT_RGBA_U8, stores=False)


def _pipelined_mixed_refs(order="catalogue_order"):
    refs = [ref_of(n) for n in pipelined_alone()] + foreign_files()
    return refs[::-1] if order == "reversed" else refs


@pytest.mark.parametrize("order", ["catalogue_order", "reversed"])
def test_entries_with_pipelined_plans_stay_pipelined_together(order):
    names = pipelined_alone()
    assert names == [n for n in CLEAN if pipelinable(n)] and len(names) >= 24, names
    assert set(CLEAN) - set(names) == {"gray_single_bands_refined", "four_separate_bands_then_refinement", "shared_tables_ids_0_to_3",
                                       "dri_changes_between_scans", "dri_divides_in_last_scan"}
    planned, done = decode_and_check(_pipelined_mixed_refs(order), decodes=3)
    assert planned["pipelined"] and planned["max_deps"] == 3 and planned["levels"] == 63 and planned["lane_work"] == 0
    assert planned["pipe_waves"] + planned["wave_tails"] == planned["scans"] and planned["wave_tails"] > 0
    assert done["launch_form"] == "pipelined_gated" and all(n > 0 for n in done["chain_scans"])


# ---------------------------------------------------------------------------------------------------- regime 3: the planner's switches

ENV_REGIMES = {
    # name: (environment, refs, launch form, what else the plan must say)
    "no_pipeline": ({"JPGPU_PROG_NO_PIPELINE": "1"}, "pipelined", "chains", lambda p: not p["pipelined"] and p["chains_ok"]),
    "no_pipeline_no_chains": ({"JPGPU_PROG_NO_PIPELINE": "1", "JPGPU_PROG_NO_CHAINS": "1"}, "pipelined", "by_level", lambda p: not p["pipelined"]),
    "no_chains_alone_changes_nothing_for_a_pipelined_plan": ({"JPGPU_PROG_NO_CHAINS": "1"}, "pipelined", "pipelined_gated", lambda p: p["pipelined"]),
    "force_pipeline": ({"JPGPU_PROG_FORCE_PIPELINE": "1"}, "pipelined", "pipelined_forced", lambda p: p["pipelined"]),
    "every_scan_on_the_lane_kernel": ({"JPGPU_PROG_STREAM_MAX_INTERVALS": "0"}, "clean", "by_level",
                                      lambda p: not p["pipelined"] and not p["chains_ok"] and p["lane_work"] >= p["scans"] and p["pipe_waves"] == 0),
    "every_interval_a_stream": ({"JPGPU_PROG_STREAM_MAX_INTERVALS": "1000000"}, "clean", "chains",
                                lambda p: not p["pipelined"] and p["chains_ok"] and p["lane_work"] == 0 and p["pipe_waves"] > p["scans"]),
    "every_interval_a_stream_level_by_level": ({"JPGPU_PROG_STREAM_MAX_INTERVALS": "1000000", "JPGPU_PROG_NO_CHAINS": "1"}, "clean", "by_level",
                                               lambda p: p["lane_work"] == 0),
}


@pytest.mark.parametrize("regime", list(ENV_REGIMES))
def test_planner_switches(regime, monkeypatch):
    """the same files under each A/B switch of the planner: same statuses, samples and stores, and the launches the switch names
    (all of them are read per upload or per decode)"""
    env, which, form, fact = ENV_REGIMES[regime]
    pipelined = _pipelined_mixed_refs()  # (asked of the planner BEFORE the switches are set)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    refs = pipelined if which == "pipelined" else [ref_of(n) for n in CLEAN] + foreign_files()
    planned, done = decode_and_check(refs, decodes=3)
    assert done["launch_form"] == form and fact(planned), (planned, done)
    # ... and with the failing entry among them (its partial flush re-plans the batch scan by scan: results only)
    decode_and_check([ref_of(n) for n in NAMES] + foreign_files(), decodes=2)


def _no_wave_chains_child():
    refs = _pipelined_mixed_refs()
    planned, done = decode_and_check(refs, decodes=3)
    print("PLAN " + json.dumps(done))


def test_without_wave_chains_every_scan_has_a_wave_of_its_own():
    """JPGPU_PROG_NO_WAVE_CHAINS is read once per process: a child of its own"""
    b = jl.Batch().upload([r.data for r in _pipelined_mixed_refs()])
    here = b.progressive_plan()
    b.close()
    assert here["wave_tails"] > 0  # (what the switch turns off is there by default)
    env = dict(os.environ, JPGPU_PROG_NO_WAVE_CHAINS="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    for k in PLANNER_ENV:
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "no_wave_chains"], env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PLAN ")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    plan = json.loads(lines[0][5:])
    assert plan["wave_tails"] == 0 and plan["pipe_waves"] == plan["scans"] == here["scans"] and plan["launch_form"] == "pipelined_gated", plan


# -------------------------------------------------------------------------------- regime 4: more waves than the machine keeps resident

@pytest.mark.parametrize("force", [False, True])
def test_more_one_wave_streams_than_stay_resident(force, monkeypatch):
    """200 copies each of the 64-scan and the 13-scan file: 15 400 one-wave workgroups against at most 32 x 3/4 x 256 resident
    ones -- chain launches chosen by SIZE, not by script (the plan is pipelined); forced: one pipelined launch without the gate.
    The sources against the checker, the copies against their sources."""
    if force:
        monkeypatch.setenv("JPGPU_PROG_FORCE_PIPELINE", "1")
    srcs = [ref_of("gray_single_coefficient_bands"), ref_of("gray_deep_sa")]
    refs = [srcs[i % 2] for i in range(400)]
    b = jl.Batch().upload([r.data for r in refs])
    planned = b.progressive_plan()
    assert planned["pipelined"] and planned["scans"] == 200 * (64 + 13) and planned["pipe_waves"] > 32 * 3 // 4 * 256
    b.run_entropy().sync()
    check_stores(b, refs[:2])
    first = [b.coefficients(0), b.coefficients(1)]
    assert not [i for i in range(2, 400) if not np.array_equal(b.coefficients(i), first[i % 2])]
    for _ in range(3):
        b.decode().sync()
        check_statuses_and_samples(b, refs[:2])
        outs = [b.output(0), b.output(1)]
        assert not [i for i in range(2, 400) if b.result(i).status != 0 or not np.array_equal(b.output(i), outs[i % 2])]
    done = b.progressive_plan()
    assert done["launch_form"] == ("pipelined_forced" if force else "chains"), done
    assert done["pipelined"] and b.progressive_fallbacks() == 0
    b.close()


# ------------------------------------------------------------------------------------------------- regime 5: a producer that is late

def _undelayed_seconds(data):
    b0 = jl.Batch().upload([data]).decode().sync()  # (first decode: module load, LDS shape ...)
    best = 1e9
    for _ in range(3):  # (the fastest of three: a hiccup here must not pass for the hook being dead)
        t0 = time.perf_counter()
        b0.decode().sync()
        best = min(best, time.perf_counter() - t0)
    b0.close()
    return best


# scan indices in file order: three_[separate_]bands_then_refinement = DC, Cb, Cr, three Y bands, Y 1-63 refinement;
# eob_run_over_32767 = DC, 1-5, 6-63 (one end-of-band run but for two coefficients), 6-63 refinement
@pytest.mark.parametrize("name,slow_scan", [("three_separate_bands_then_refinement", 3), ("three_separate_bands_then_refinement", 4),
                                            ("three_separate_bands_then_refinement", 5), ("three_bands_then_refinement", 3),
                                            ("three_bands_then_refinement", 4), ("three_bands_then_refinement", 5), ("eob_run_over_32767", 1)])
def test_a_follower_waits_for_each_of_its_producers(name, slow_scan, monkeypatch):
    """JPGPU_DEBUG_DELAY_SCAN=k:ms makes scan k slow (it idles at its start and after every progress word), so that its
    followers certainly catch up with it.  The refinement over 1-63 has THREE direct producers (separate bands), each late in
    turn, or one that passes on the progress of the two in front of it (contiguous bands); the refinement of the empty band
    follows a scan of a few bytes, which has to pass on the progress of the scan in front of IT."""
    r = ref_of(name)
    e = ps.CATALOGUE[name]
    assert e.script[slow_scan].ss >= 1 and e.script[slow_scan].ah == 0 and e.script[-1].ah == 1
    undelayed = _undelayed_seconds(r.data)
    monkeypatch.setenv("JPGPU_DEBUG_DELAY_SCAN", "%d:4" % slow_scan)
    # A follower's polls are counted over its whole scan (2^17 by default, about 0.3 s: the bound on waiting for a producer that is
    # stuck).  The slow scan idles 4 ms per progress word on purpose -- 182 block rows here make that 0.7 s -- so the bound is
    # raised to about 10 s: what is tested is that the follower WAITS, in the pipelined launch, not how long it may.
    monkeypatch.setenv("JPGPU_PROG_SPIN_BUDGET", str(1 << 22))
    b = jl.Batch().upload([r.data])
    t0 = time.perf_counter()
    b.decode().sync()
    delayed = time.perf_counter() - t0
    assert delayed > undelayed + 0.002, (undelayed, delayed)  # the hook is live
    check_statuses_and_samples(b, [r])
    plan = b.progressive_plan()
    assert plan["launch_form"] == "pipelined_gated" and plan["pipelined"] and b.progressive_fallbacks() == 0, plan
    b.run_entropy().sync()
    check_stores(b, [r])
    b.close()


# ------------------------------------------------------------------------------------------------- regime 6: one scan per call

SCAN_BY_SCAN = ["ends_on_cb_transformed_twice", "ends_on_chroma_pair_luma_never", "dc_per_component_chroma_first", "dri_changes_between_scans", "cmyk",
                "high_band_before_low"]


@pytest.mark.parametrize("name", SCAN_BY_SCAN)
def test_scan_by_scan_through_the_c_abi_and_the_decoder_mirror(name):
    """jpgpu_progressive_begin / _scan / _dispose with the tables and the restart interval in force at every SOS, and
    JpegDecoder.Decode() into the stock 8-bit sink"""
    from test_per_scan_gpu import _decode_progressive_scan_by_scan

    r = ref_of(name)
    n = len(ps.CATALOGUE[name].comps)

    def deliver(dec, fh):
        return dec.Dispose(fmt=jl.FMT_INTERLEAVED_U8).reshape(fh.NumberOfLines, fh.SamplesPerLine, n)

    out, state = _decode_progressive_scan_by_scan(r.data, deliver)
    assert np.array_equal(out, r.out8), int((out != r.out8).sum())
    assert len(state["dris"]) == len(ps.CATALOGUE[name].script) and state["dris"] == [s.dri for s in ps.CATALOGUE[name].script]

    def deliver_writer(dec, fh):
        buf = np.zeros(fh.SamplesPerLine * fh.NumberOfLines * n, np.uint8)
        dec.Dispose(outputWriter=jl.JpegBufferOutputWriter8Bit(fh.SamplesPerLine, fh.NumberOfLines, n, buf))
        return buf.reshape(fh.NumberOfLines, fh.SamplesPerLine, n)

    out2, _ = _decode_progressive_scan_by_scan(r.data, deliver_writer)
    assert np.array_equal(out2, r.out8)
    d = jl.JpegDecoder()
    d.SetInput(r.data)
    d.Identify()
    assert (d.Width, d.Height, d.NumberOfComponents) == (r.out8.shape[1], r.out8.shape[0], n)
    buf = np.zeros(d.Width * d.Height * n, np.uint8)
    d.SetOutputWriter(jl.JpegBufferOutputWriter8Bit(d.Width, d.Height, n, buf))
    d.Decode()
    assert np.array_equal(buf.reshape(r.out8.shape), r.out8)


def test_the_failing_entry_fails_in_the_decoder_mirror_like_the_checker():
    r = ref_of("dri_divides_in_middle_scan")
    d = jl.JpegDecoder()
    d.SetInput(r.data)
    d.Identify()
    buf = np.zeros(d.Width * d.Height * 3, np.uint8)
    d.SetOutputWriter(jl.JpegBufferOutputWriter8Bit(d.Width, d.Height, 3, buf))
    with pytest.raises(jl.InvalidOperationException):  # (the message is compared through the batch's detail string, above)
        d.Decode()
    assert np.array_equal(buf.reshape(r.out8.shape), r.out8)  # what the reference's writer holds when the exception leaves


if __name__ == "__main__":
    assert sys.argv[1:] == ["no_wave_chains"]
    _no_wave_chains_child()
