"""One OptimizeBatch and one EncodeBatch reused across uploads whose roads differ: restart intervals, DRI = 0 subsequences, the coefficient
road (turned, windowed), its release and its return, an empty upload; the encoder's one-pass and two-kernel entropy forms by turns.  Every
output byte for byte against the oracle, or -- where the oracle has no say (turn, window) -- against a fresh one-shot optimize_batch."""
import numpy as np
import pytest

import jpeglibrary_amd as jl
import transform_cases as tc
from oracle import pyoracle as po
from tools import jpegsynth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files():
    """each with an MCU count that is no multiple of its DRI: 6 MCUs under 4 (the 4:2:0 and grey shapes), 63 under 5 (72 x 56 4:4:4)"""
    return {"420_48x32_dri4": tc.make("420_48x32", dri=4), "420_40x27_dri4": tc.make("420_40x27", dri=4), "420_40x27": tc.make("420_40x27"),
            "grey_20x16_dri4": tc.make("grey_20x16", dri=4), "444_72x56": jpegsynth.encode(72, 56, "444", 75, 0, seed=5),
            "444_72x56_dri5": jpegsynth.encode(72, 56, "444", 75, 5, seed=6)}


def test_one_optimize_batch_through_uploads_whose_roads_differ(files):
    f = files
    a = f["420_48x32_dri4"]
    quarter = (0, 0, 48, 16)  # 3 MCUs of the 6: still no multiple of the restart interval
    # (the oracle has no say on these three: a fresh batch each)
    turned = jl.optimize_batch([a], orientations=[6])[0]
    cut = jl.optimize_batch([a], windows=[quarter])[0]
    large = jl.optimize_batch([f["444_72x56_dri5"], f["444_72x56"]], orientations=[6, 3])
    assert turned != po.optimize(a) and cut != po.optimize(a)  # (189 blocks each in `large`, 36 in `turned`)
    b = jl.OptimizeBatch()
    try:
        # 1. two DRI > 0 files
        b.upload([a, f["420_40x27_dri4"]]).run()
        assert [b.output(i) for i in range(2)] == [po.optimize(a), po.optimize(f["420_40x27_dri4"])]
        assert b.turn_sources() == 0
        # 2. DRI > 0, DRI = 0, turned, windowed
        b.set_orientations([1, 1, 6, 1]).set_windows([(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), quarter])
        b.upload([f["grey_20x16_dri4"], f["444_72x56"], a, a]).run()
        assert [b.output(i) for i in range(4)] == [po.optimize(f["grey_20x16_dri4"]), po.optimize(f["444_72x56"]), turned, cut]
        assert b.turn_sources() == 1 and b.transform(2).orientation == 6 and b.window(3) == quarter
        # 3. DRI = 0 only: nothing is turned, the coefficient road's buffers are released
        b.upload([f["444_72x56"], f["420_40x27"]], strip=False).run()
        assert [b.output(i) for i in range(2)] == [po.optimize(f["444_72x56"], False), po.optimize(f["420_40x27"], False)]
        assert b.turn_sources() == 0 and b.turn_stage_ms() == (0.0, 0.0, 0.0)
        # 4. two turned files, larger than the one of upload 2
        b.set_orientations([6, 3]).upload([f["444_72x56_dri5"], f["444_72x56"]]).run()
        assert [b.output(i) for i in range(2)] == large
        assert b.turn_sources() == 2
        # 5. nothing
        b.upload([]).run()
        assert len(b) == 0 and b.turn_sources() == 0
    finally:
        b.close()


def test_one_encode_batch_through_both_entropy_forms():
    rng = np.random.default_rng(7)
    pair = [rng.integers(0, 256, (32, 48, 3)).astype(np.uint8), rng.integers(0, 256, (27, 40, 3)).astype(np.uint8)]
    want = [po.encode_8bit(im, 2, 2, 75) for im in pair]
    want_dri = [po.encode_8bit(im, 2, 2, 75, restart_interval=3) for im in pair]
    b = jl.EncodeBatch()
    try:
        b.upload(pair)
        for _ in range(2):  # (the second encode() sizes its LDS buffer from the first)
            b.encode()
            assert [b.output(i) for i in range(2)] == want
        one_pass, fell_back = b.emit_passes()
        assert fell_back == 0
        b.upload(pair, restart_interval=3).encode()  # two kernels only
        assert [b.output(i) for i in range(2)] == want_dri
        assert b.emit_passes() == (one_pass, 0)
        b.upload(pair).encode()
        assert [b.output(i) for i in range(2)] == want
        assert b.emit_passes()[1] == 0
    finally:
        b.close()
