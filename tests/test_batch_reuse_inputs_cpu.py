"""The inputs of test_batch_reuse_gpu.py (tests/reuse_cases.py) are what their names say -- shown on the oracle alone, without a GPU.

A reuse test proves nothing with the wrong inputs: a quiet file that writes its whole slot hides a missing clear, and so does a loud file
that left zeros where the quiet one leaves its hole.  So: every loud sample is at least 16 and every loud block's last coefficient is
nonzero; a truncated file fails in a block strictly inside its scan with at least a quarter of the picture behind it; the missing scan
leaves its component zero in the reference's buffer; the band files never write coefficients 6..63; the black file is end-of-block only;
and every quiet image is no larger than the loud image whose slot it lands in."""
import numpy as np
import pytest

import reuse_cases as rc
from oracle import pyoracle as po

LOUD_BASELINE = [("k2_%d" % k, lambda k=k: rc.loud_k2(k)) for k in range(5)] + [("gray", rc.loud_gray)] + [("k2s_%d" % k, lambda k=k: rc.loud_k2s(k)) for k in range(2)]


@pytest.mark.parametrize("name,make", LOUD_BASELINE, ids=[n for n, _ in LOUD_BASELINE])
def test_loud_baseline_files_are_loud_everywhere(name, make):
    kind, px, coefs = rc.reference(make())
    assert kind == "OK" and px.min() >= rc.LOUD_FLOOR, (name, kind, int(px.min()))
    assert coefs.shape[0] == rc.scan_blocks(make()) and (coefs[:, 63] != 0).all(), (name, int((coefs[:, 63] == 0).sum()))
    assert px.nbytes % 256 == 0  # (the slots of a loud upload lie back to back: no gap that an older upload's bytes could show through)


@pytest.mark.parametrize("k", range(3))
def test_loud_progressive_files_are_loud_everywhere(k):
    f = rc.loud_progressive(k)
    assert rc.is_progressive(f)
    kind, px, _ = rc.reference(f)
    assert kind == "OK" and px.min() >= rc.LOUD_FLOOR and px.nbytes % 256 == 0
    _, blocks, _ = po.decode_progressive_store(f)
    assert sorted(blocks) == [0, 1, 2] and [len(blocks[c]) for c in range(3)] == [48, 12, 12]
    assert all(v[63] != 0 for b in blocks.values() for v in b.values())


def test_the_loud_roads_by_their_bytes():
    """what the planner reads of the loud files: restart intervals for K2's pools, bytes behind the scan header for K2S"""
    for f in rc.loud_k2_upload():
        assert f[f.index(b"\xff\xdd"):][4:6] == b"\x00\x04"
    hist = {len(f) - rc.entropy_start(f) >= rc.K2S_MIN_BYTES for f in (rc.loud_k2s(0), rc.loud_k2s(1), rc.truncated(0))}
    assert hist == {True}
    # the smallest loud 4:4:4 file over the threshold, on a ladder of whole MCUs
    ladder = [(8, 8), (16, 8), (16, 16), (24, 16)]
    over = [len(rc.loud(w, h, "444", seed=120)) - rc.entropy_start(rc.loud(w, h, "444", seed=120)) >= rc.K2S_MIN_BYTES for w, h in ladder]
    assert ladder[over.index(True)] == (16, 16), over
    # one table set through each run of files (a run of consecutive scans with the same tables is what is pooled)
    dht = {bytes(f[f.index(b"\xff\xc4"):f.index(b"\xff\xda")]) for f in rc.loud_k2_upload()[:5]}
    assert len(dht) == 1


@pytest.mark.parametrize("dri", [4, 0])
def test_truncated_files_fail_strictly_inside_their_scan(dri):
    f = rc.truncated(dri)
    assert f[-2:] == b"\xff\xd9"
    kind, px, _ = rc.reference(f)
    at, err = rc.blocks_before_the_error(f)
    total = rc.scan_blocks(f)
    assert err is not None and err.kind == kind != "OK"
    assert 0 < at < total - 1 and (total - at) * 4 >= total, (at, total)
    # ... and the picture says the same: something in front of the block, nothing in the last quarter of the MCU rows
    assert px[:16].any() and not px[-(px.shape[0] // 4) // 16 * 16:].any()


def test_the_missing_scan_leaves_its_component_zero():
    kind, px, _ = rc.reference(rc.missing_last_scan())
    assert kind == "OK"
    assert px[..., 0].any() and px[..., 1].any() and not px[..., 2].any()


def test_the_band_files_never_write_coefficients_6_to_63():
    f = rc.band_1_5()
    assert rc.is_progressive(f) and rc.reference(f)[0] == "OK"
    _, blocks, _ = po.decode_progressive_store(f)
    assert sorted(blocks) == [0, 1, 2]
    for b in blocks.values():
        assert all(not v[6:].any() for v in b.values()) and all(v[1:6].any() for v in b.values())
    # (the coefficients the file was written from do have them: the script leaves them out, not the picture)
    assert all((c[..., 6:] != 0).all() for c in rc._band()[1])
    kind, px, _ = rc.reference(rc.band_1_5_cut())
    assert kind == "InvalidDataException" and px is not None
    assert rc._sos_offsets(rc.band_1_5_cut()) == rc._sos_offsets(f)[:2]  # cut inside the second scan


def test_the_black_file_is_end_of_block_only():
    kind, px, coefs = rc.reference(rc.black_gray())
    assert kind == "OK" and not px.any() and not coefs[:, 1:].any() and coefs.shape[0] == 9 * 6


def test_the_road_files_decode():
    assert [rc.reference(f)[0] for f in rc.road_files()] == ["OK"] * len(rc.road_files())


def test_every_quiet_image_fits_the_loud_image_whose_slot_it_takes():
    """the INTERLEAVED_U8 sequence of test_batch_reuse_gpu.py, from sizes alone: slots start at multiples of 256, the loud slots lie back to
    back, so a quiet upload lands inside the loud bytes when it ends in front of the loud upload's end -- and slot 0 inside loud slot 0"""
    def end(files):
        at = 0
        for f in files:
            at = -(-at // 256) * 256 + rc.output_bytes(f)
        return at

    for quiet, loud in ((rc.quiet_upload(), rc.loud_k2_upload()), ([rc.truncated(0)], [rc.loud_k2s(0), rc.loud_k2s(1)]),
                        (rc.band_upload(), [rc.loud_progressive(k) for k in range(3)])):
        assert rc.output_bytes(quiet[0]) <= rc.output_bytes(loud[0])
        assert end(quiet) <= end(loud) == sum(rc.output_bytes(f) for f in loud)
