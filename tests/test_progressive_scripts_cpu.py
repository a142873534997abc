"""The catalogue of progressive scan scripts (tests/progscript.py) is what it says it is -- checked without a GPU.

For every entry: the checker's coefficient store equals the writer's own model (expected_store) on every block the checker
reports, the blocks it does not report are exactly those of the components Dispose() never transforms, and its outcome is the
one the catalogue STATES; every 8-bit file loads in Pillow (an independent decoder agrees that the file is legal; no sample
comparison: libjpeg's IDCT and chroma upsampling differ from the reference's by design).  So what the GPU tests expect has two
independent sources.  Plus unit checks of the writer itself.
"""
import io

import numpy as np
import pytest

import progscript as ps
from oracle import pyoracle as po

NAMES = list(ps.CATALOGUE)


def checker_outcome(data):
    """-> (outcome as the catalogue states it, the checker's store or {})"""
    try:
        _, blocks, _ = po.decode_progressive_store(data)
        return ps.CLEAN, blocks
    except po.OracleError as e:
        return (e.kind, e.message), {}


@pytest.mark.parametrize("name", NAMES)
def test_checker_store_equals_the_writers_model(name):
    b = ps.build(name)
    e = b.entry
    outcome, blocks = checker_outcome(b.data)
    assert outcome == e.outcome
    if outcome != ps.CLEAN:
        return
    transformed = {s for s in ps.final_slots(e.script, len(e.comps)) if s is not None}
    assert set(blocks) == transformed  # (a component no slot names is never transformed: the checker's tap does not report it)
    for ci in sorted(transformed):
        want = b.expected[ci]
        assert len(blocks[ci]) == want.shape[0] * want.shape[1]
        got = np.stack([blocks[ci][(bx, by)] for by in range(want.shape[0]) for bx in range(want.shape[1])]).reshape(want.shape)
        wrong = np.argwhere((got != want).any(axis=2))
        assert wrong.size == 0, (ci, len(wrong), wrong[:4].tolist())


@pytest.mark.parametrize("name", [n for n in NAMES if ps.CATALOGUE[n].precision == 8])
def test_pillow_loads_every_8bit_entry(name):
    from PIL import Image

    b = ps.build(name)
    im = Image.open(io.BytesIO(b.data))
    im.load()
    assert im.size == (b.entry.width, b.entry.height)
    assert im.mode == {1: "L", 3: "RGB", 4: "CMYK"}[len(b.entry.comps)]


def test_the_catalogue_stays_a_catalogue_of_decodable_files():
    """the GPU test over this catalogue can never quietly turn into an error-status test"""
    clean = [n for n in NAMES if ps.CATALOGUE[n].outcome == ps.CLEAN]
    assert len(clean) >= 0.85 * len(NAMES), (len(clean), len(NAMES))
    for row in ps.ROWS:
        assert any(ps.CATALOGUE[n].row == row for n in clean), row
    assert len(ps.ROWS) >= 19 and len(NAMES) >= 28
    for n in ps.EXTENDED_U16_ENTRIES:
        assert ps.CATALOGUE[n].outcome == ps.CLEAN
    # both kinds of ending of fact 1, and scripts that leave every component transformed exactly once
    endings = {n: ps.final_slots(ps.CATALOGUE[n].script, len(ps.CATALOGUE[n].comps)) for n in NAMES}
    assert endings["ends_on_cb_transformed_twice"] == [1, 1, 2] and endings["ends_on_chroma_pair_luma_never"] == [1, 2, None]
    assert not ps.slots_map_one_to_one(ps.CATALOGUE["ends_on_cb_transformed_twice"].script, 3)
    assert sum(ps.slots_map_one_to_one(ps.CATALOGUE[n].script, len(ps.CATALOGUE[n].comps)) for n in NAMES) >= 15


def test_catalogue_entries_have_the_properties_their_rows_name():
    C = ps.CATALOGUE
    e = C["gray_single_coefficient_bands"]
    assert len(e.script) == 64 and [(s.ss, s.se) for s in e.script[1:]] == [(k, k) for k in range(1, 64)]
    assert len(C["gray_single_bands_refined"].script) == 128
    assert [(s.ah, s.al) for s in C["gray_deep_sa"].script if s.ss] == [(0, 6)] + [(a + 1, a) for a in range(5, -1, -1)]
    assert max(s.al for s in C["precision8_al13"].script) == 13 and C["precision12_al9"].precision == 12
    e = C["three_bands_then_refinement"]
    assert e.width >= 1024 and e.height >= 768 and e.comps == ps.YCC420
    assert [(s.ss, s.se, s.ah) for s in e.script if s.comps == (0,)] == [(1, 5, 0), (6, 20, 0), (21, 63, 0), (1, 63, 1)]
    assert sum(s.comps == (0,) and s.ah == 0 for s in C["five_bands_then_one_refinement"].script) == 5
    # contiguous bands follow each other (a first pass may write up to Se + 15), bands more than 15 apart do not: their
    # refinement has one direct producer per band -- three, and four
    assert ps.planner_model(C["three_bands_then_refinement"].script)["deps"][-1] == [5]
    assert ps.planner_model(C["five_bands_then_one_refinement"].script)["deps"][-1] == [7]
    e = C["three_separate_bands_then_refinement"]
    assert e.width >= 1024 and e.height >= 768 and ps.planner_model(e.script)["deps"][-1] == [3, 4, 5]
    assert ps.planner_model(C["four_separate_bands_then_refinement"].script)["deps"][-1] == [3, 4, 5, 6]
    assert ps.planner_model(C["dc_three_producers"].script)["deps"][-1] == [0, 1, 2]
    for n, gaps in (("three_separate_bands_then_refinement", [(6, 20), (26, 40)]), ("four_separate_bands_then_refinement", [(2, 16), (18, 32), (34, 48)])):
        y = ps.build(n).coefs[0]
        assert all(set(np.unique(y[..., a:b + 1])) == {-1, 0, 1} for a, b in gaps)  # new coefficients for the refinement to bring in
    m = ps.planner_model(C["gray_single_coefficient_bands"].script)
    assert m["levels"] == 63 and m["max_deps"] == 1 and m["deps"][1] == [] and m["deps"][63] == [62]
    m = ps.planner_model(C["gray_single_bands_refined"].script)
    assert m["levels"] == 126 and m["max_deps"] == 6 and m["deps"][64] == [0]
    e = C["dri_changes_between_scans"]
    assert all(a.dri != b.dri for a, b in zip(e.script, e.script[1:])) and e.script[0].dri != 0  # a DRI segment in front of every scan
    units = {(0, 1, 2): 48, (1, 2): 48, (0,): 180, (1,): 48, (2,): 48}  # 120 x 90 4:2:0: MCUs, Y blocks, chroma blocks
    assert all(s.dri == 0 or units[s.comps] % s.dri for s in e.script)  # ... none dividing its scan's unit count
    assert max(-(-units[s.comps] // s.dri) for s in e.script if s.dri) > 16  # ... and one scan of more than 16 intervals
    for n, where in (("dri_divides_in_last_scan", -1), ("dri_divides_in_middle_scan", 1)):
        s = C[n].script[where]
        assert s.dri and units[s.comps] % s.dri == 0
    assert (C["eob_run_over_32767"].width // 8) * (C["eob_run_over_32767"].height // 8) > ps.MAX_EOBRUN
    assert all(s.shape == "long16" for n in ("dense_long16_gray", "dense_long16_420") for s in C[n].script)
    for n in ("dense_long16_gray", "dense_long16_420"):
        assert all((c[..., 1:] != 0).all() for c in ps.build(n).coefs)  # 63 nonzero AC coefficients in every block
    e = C["shared_tables_ids_0_to_3"]
    assert {s.tid for s in e.script if s.ss == 0 and s.ah == 0} == {0, 1, 2, 3} == {s.tid for s in e.script if s.ss and s.ah == 0}
    assert ps.build("shared_tables_ids_0_to_3").data.count(b"\xff\xc4") == 1
    # nonzero values in the padding blocks of the MCU grid (they feed the DC predictor of interleaved scans)
    b = ps.build("one_pixel")
    assert b.coefs[0].shape == (2, 2, 64) and all(b.coefs[0][y, x, 0] != 0 for y, x in ((0, 1), (1, 0), (1, 1)))
    # category limits: AC +-1023, DC differences of category 11
    b = ps.build("category_limits")
    dc = b.coefs[0][..., 0].reshape(-1)
    assert np.abs(b.coefs[0][..., 1:]).max() == 1023 and (np.abs(np.diff(dc)) >= 1024).all() and np.abs(np.diff(dc)).max() < 2048
    assert set(np.unique(np.abs(ps.build("plus_minus_one").coefs[1][..., 1:]))) == {0, 1}


# ---------------------------------------------------------------------------------------------------------- the writer on its own

@pytest.mark.parametrize("seed", range(6))
def test_optimal_tables_obey_kraft_with_the_reserved_code(seed):
    rng = np.random.default_rng(seed)
    n = [1, 2, 3, 40, 200, 256][seed]
    freq = {int(s): int(c) for s, c in zip(rng.choice(256, n, replace=False), np.maximum(1, rng.geometric(0.002 * (seed + 1), n)))}
    if seed == 4:
        freq = {s: 1 << min(40, i // 4) for i, s in enumerate(freq)}  # lengths far beyond 16 before the limiting step
    bits, vals = ps.optimal_table(freq)
    assert sorted(vals) == sorted(freq) and len(bits) == 16 and sum(bits) == len(vals)
    assert sum(b << (16 - ln) for ln, b in enumerate(bits, 1)) <= (1 << 16) - 1  # Kraft, one 16-bit code to spare
    codes = ps.code_map(bits, vals)
    assert all(code != (1 << ln) - 1 for code, ln in codes.values())  # nobody got an all-ones code
    # the commoner symbol never has the longer code
    order = sorted(freq, key=lambda s: -freq[s])
    assert all(codes[a][1] <= codes[b][1] for a, b in zip(order, order[1:]) if freq[a] > freq[b])


def test_long16_table_is_one_short_code_and_16_bit_codes_from_0x8000():
    bits, vals = ps.long16_table({0x00, 0x11, 0xF0}, dc=False)
    codes = ps.code_map(bits, vals)
    assert codes[vals[0]] == (0, 1) and vals[0] not in (0x00, 0x11, 0xF0)
    assert [codes[s] for s in (0x00, 0x11, 0xF0)] == [(0x8000, 16), (0x8001, 16), (0x8002, 16)]
    assert ps.long16_table(set(range(12)), dc=True)[1][0] == 15  # (libjpeg refuses DC symbols above 15)


def _gray_blocks(n_x, n_y):
    return [np.zeros((n_y, n_x, 64), np.int64)], ps.GRAY, 8 * n_x, 8 * n_y


def test_end_of_band_runs_are_split_at_32767():
    coefs, comps, w, h = _gray_blocks(200, 200)  # 40 000 empty blocks, one coefficient in the last
    coefs[0][199, 199, 5] = 3
    tk = ps.scan_symbols(coefs, comps, w, h, ps.S([0], 1, 63, 0, 0))
    # EOB14 with all 14 extra bits set (run 32 767), then the remaining 39 999 - 32 767 = 7 232 blocks (EOB12), then the coefficient
    assert tk[0] == ("S", 0, 14 << 4, 0x3FFF, 14) and tk[1] == ("S", 0, 12 << 4, 7232 - 4096, 12)
    assert tk[2] == ("S", 0, (4 << 4) | 2, 3, 2) and tk[3] == ("S", 0, 0, 0, 0) and len(tk) == 4
    # a refinement scan over the same store: the one coefficient is history (one correction bit, behind its run's symbol)
    tk = ps.scan_symbols(coefs, comps, w, h, ps.S([0], 1, 63, 1, 0))
    assert tk == [("S", 0, 14 << 4, 0x3FFF, 14), ("S", 0, 12 << 4, 7233 - 4096, 12), ("B", 1)]


def test_correction_bits_are_flushed_before_the_buffer_passes_937():
    coefs, comps, w, h = _gray_blocks(40, 1)
    coefs[0][...] = 2  # every coefficient has history at Al = 0, none is new: 63 correction bits per block, no symbol but EOBn
    tk = ps.scan_symbols(coefs, comps, w, h, ps.S([0], 1, 63, 1, 0))
    runs, bits = [], 0
    for t in tk:
        if t[0] == "S":
            assert t[2] & 15 == 0 and t[2] != 0xF0
            runs.append((1 << (t[2] >> 4)) + t[3])
            bits = 0
        else:
            bits += 1
            assert bits <= ps.MAX_CORRECTION_BITS + 63
    assert runs == [15, 15, 10] and sum(t[0] == "B" for t in tk) == 40 * 63  # 15 blocks x 63 bits = 945 > 937


def test_restart_markers_reset_runs_and_predictors():
    coefs, comps, w, h = _gray_blocks(5, 2)
    coefs[0][..., 0] = 100
    tk = ps.scan_symbols(coefs, comps, w, h, ps.S([0], 0, 0, 0, 0, dri=4))
    assert [i for i, t in enumerate(tk) if t == ("R",)] == [4, 9] and len(tk) == 12
    assert [t[2] for t in tk if t[0] == "S"] == [7, 0, 0, 0, 7, 0, 0, 0, 7, 0]  # the predictor starts again behind every marker
    tk = ps.scan_symbols(coefs, comps, w, h, ps.S([0], 0, 0, 0, 0, dri=5))
    assert sum(t == ("R",) for t in tk) == 1  # an interval that divides the unit count: no marker behind the last unit
    tk = ps.scan_symbols(coefs, comps, w, h, ps.S([0], 1, 63, 0, 0, dri=4))
    assert tk == [("S", 0, 2 << 4, 0, 2), ("R",), ("S", 0, 2 << 4, 0, 2), ("R",), ("S", 0, 1 << 4, 0, 1)]  # runs end at the markers
    data = ps.write(w, h, comps, {0: np.ones(64, np.uint16)}, coefs, [ps.S([0], 0, 0, 0, 0, dri=4), ps.S([0], 1, 63, 0, 0, dri=4),
                                                                      ps.S([0], 1, 63, 0, 0, dri=0)])
    assert data.count(b"\xff\xdd") == 2 and data.count(b"\xff\xd0") == 2 and data.count(b"\xff\xd1") == 2 and b"\xff\xd2" not in data


def test_bytes_are_stuffed_and_scans_padded_with_ones():
    bw = ps.Bits()
    bw.put(0xFF, 8)
    bw.put(0b101, 3)
    bw.align()
    assert bytes(bw.out) == b"\xff\x00\xbf"


def test_expected_store_is_the_last_scan_that_covered_a_coefficient():
    coefs = [np.zeros((1, 1, 64), np.int64)]
    coefs[0][0, 0, :4] = [-7, 5, -5, 1]
    script = [ps.S([0], 0, 0, 0, 1), ps.S([0], 1, 2, 0, 2), ps.S([0], 1, 2, 2, 1)]
    exp = ps.expected_store(coefs, ps.GRAY, 8, 8, script)[0]
    assert exp[0, 0, :4].tolist() == [-8, 4, -4, 0]  # DC floors, AC truncates towards zero; coefficient 3 never sent
    exp420 = [np.full((1, 1, 64), 1, np.int16), np.full((1, 1, 64), 2, np.int16), np.full((1, 1, 64), 3, np.int16)]
    m = ps.store_in_mcu_order(exp420, ps.YCC420, 8, 8)
    assert m.shape == (6, 64) and m[:, 0].tolist() == [1, 0, 0, 0, 2, 3]  # the blocks outside a component's grid are zero
