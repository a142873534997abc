"""The oracle's block transform held against the mathematical IDCT, no GPU.

po.block_dequant_idct_shift is DequantizeBlockAndUnZigZag + FastFloatingPointDCT.TransformIDCT (float32, a fixed order of
operations) + ShiftDataLevel: (short)(MathF.Round(v) + levelShift).  The model here is T.81 A.3.3 in float64, with the zig-zag
order of T.81 Figure A.6 walked in the test; nothing is taken from the product or the oracle.  The float32 transform's error
grows with the block's magnitude: every mismatch against round(float64) seen over random blocks lay within 1.2e-8 * sum|c*q| of a
rounding tie.  So the rule per sample, with tau = 2^-22 * sum|c_k * q_k| (a 20x margin):
  * exact: where the float64 value lies more than tau from a half-integer, the sample IS (round_half_even(exact) + shift) taken
    mod 2^16 as int16 (the 16-bit wrap of the reference's (short) cast);
  * bound: everywhere, (sample - shift) mod 2^16 is an integer within 0.5 + tau of the float64 value.
The GPU tests (test_idct_stage_gpu.py) apply the same rule to K3's own output."""
import math

import numpy as np
import pytest

from oracle import pyoracle as po


def zigzag_to_natural():
    """T.81 Figure A.6: the zig-zag walk over the anti-diagonals of the 8 x 8 block, starting right from (0, 0); odd diagonals
    run down-left, even ones up-right.  Returns nat[k] = row * 8 + col of zig-zag index k."""
    nat = []
    for d in range(15):
        cells = [(r, d - r) for r in range(max(0, d - 7), min(d, 7) + 1)]  # row increasing = down-left
        nat += [r * 8 + c for r, c in (cells if d % 2 else cells[::-1])]
    return np.array(nat, dtype=np.int64)


NAT = zigzag_to_natural()
# A[u][x] = C(u) / 2 * cos((2x + 1) u pi / 16), C(0) = 1 / sqrt(2), C(u) = 1 otherwise: s = A^T S A (T.81 A.3.3)
_A = np.array([[(1 / math.sqrt(2) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)] for u in range(8)])
TAU_SCALE = 2.0 ** -22


def dequantise_natural(zz, q):
    """int[..., 64] zig-zag coefficients, [..., 64] zig-zag quantisers -> int64[..., 8, 8] in natural order (S[v][u])"""
    zz = np.asarray(zz, np.int64)
    prod = zz * np.broadcast_to(np.asarray(q, np.int64), zz.shape)
    S = np.zeros(zz.shape, np.int64)
    S[..., NAT] = prod
    return S.reshape(zz.shape[:-1] + (8, 8))


def idct_float64(zz, q):
    """The exact samples before the level shift, float64 [..., 8, 8], and tau per block [...]"""
    S = dequantise_natural(zz, q).astype(np.float64)
    exact = np.einsum("vy,...vu,ux->...yx", _A, S, _A)  # s[y][x] = sum_v sum_u A[v][y] S[v][u] A[u][x]
    tau = TAU_SCALE * np.abs(np.asarray(zz, np.int64) * np.asarray(q, np.int64)).sum(axis=-1)
    return exact, tau


def check_tau_rule(got, zz, q, shift, min_exact_fraction=0.0, what=""):
    """got: int16 samples [..., 8, 8] (or [..., 64]) of the blocks zz with tables q; returns the fraction of samples the exact
    rule decided"""
    exact, tau = idct_float64(zz, q)
    got = np.asarray(got, np.int64).reshape(exact.shape)
    t = tau[..., None, None]
    r = np.rint(exact)  # half to even
    decided = np.abs(exact - (np.floor(exact) + 0.5)) > t
    want = ((r.astype(np.int64) + shift + 32768) % 65536) - 32768
    bad = decided & (got != want)
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist(), exact[bad][:5].tolist())
    diff = ((got - shift - r.astype(np.int64) + 32768) % 65536) - 32768
    err = np.abs(diff + (r - exact))
    assert (err <= 0.5 + t).all(), (what, float((err - t).max()))
    frac = float(decided.mean()) if decided.size else 1.0
    assert frac >= min_exact_fraction, (what, frac)
    return frac


def oracle_blocks(zz, q, shift):
    return po.block_dequant_idct_shift(np.asarray(zz, np.int16).reshape(-1, 64), np.asarray(q, np.uint16), shift).reshape(-1, 8, 8)


def sparse_blocks(rng, n, lo, hi, density):
    c = rng.integers(lo, hi + 1, size=(n, 64))
    keep = rng.random((n, 64)) < density
    keep[:, 0] |= rng.random(n) < 0.8
    return np.where(keep, c, 0).astype(np.int16)


def in_envelope(zz, q):
    """blocks whose every sample stays inside int32 for sure: sum|c*q| * 6.98 < 2^31"""
    return np.abs(np.asarray(zz, np.int64) * np.asarray(q, np.int64)).sum(axis=-1) * 6.98 < 2.0 ** 31


def _run(rng, n_tables, per_table, make_q, make_c, shift=128, envelope=False):
    """n_tables x per_table blocks through the oracle; returns (blocks checked, fraction decided by the exact rule)"""
    total, decided = 0, 0.0
    for _ in range(n_tables):
        q = make_q(rng)
        zz = make_c(rng, per_table)
        if envelope:
            zz = zz[in_envelope(zz, q)]
        decided += check_tau_rule(oracle_blocks(zz, q, shift), zz, q, shift) * len(zz)
        total += len(zz)
    return total, decided / max(1, total)


def test_zigzag_walk_is_the_figure():
    assert NAT[:10].tolist() == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24]
    assert NAT[-6:].tolist() == [61, 54, 47, 55, 62, 63]
    assert sorted(NAT.tolist()) == list(range(64))


def test_the_float64_model_inverts_the_forward_transform():
    rng = np.random.default_rng(0)
    s = rng.normal(size=(8, 8))
    S = _A @ s @ _A.T  # F(v, u) = sum_y sum_x A[v][y] s[y][x] A[u][x]
    assert np.allclose(_A.T @ S @ _A, s, atol=1e-12)
    # one coefficient in the model against A.3.3 written out: position (v, u) = (row, column) of the natural order
    zz = np.zeros(64, np.int64)
    zz[4] = 10  # zig-zag 4 = natural 9 = row 1, column 1
    exact, _ = idct_float64(zz, np.ones(64))
    y, x = np.mgrid[0:8, 0:8]
    assert np.allclose(exact, 0.25 * 10 * np.cos((2 * x + 1) * np.pi / 16) * np.cos((2 * y + 1) * np.pi / 16))
    zz[4], zz[1] = 0, 10  # zig-zag 1 = row 0, column 1: varies along x only
    exact, _ = idct_float64(zz, np.ones(64))
    assert np.allclose(exact, 0.25 * 10 / math.sqrt(2) * np.cos((2 * x + 1) * np.pi / 16))


def test_regimes_hold_the_tau_rule_on_two_hundred_thousand_blocks():
    rng = np.random.default_rng(20261016)
    q8 = lambda r: r.integers(1, 256, 64).astype(np.uint16)
    q16 = lambda r: r.integers(1, 65536, 64).astype(np.uint16)
    counts = {}
    # small coefficients with 8-bit tables (what real encoders give): nearly every sample is decided exactly
    n, f = _run(rng, 60, 1000, q8, lambda r, k: sparse_blocks(r, k, -64, 64, 0.3))
    counts["small"] = n
    assert f > 0.9, f
    # full int16 coefficients with 8-bit tables, dense and sparse
    n1, _ = _run(rng, 30, 1000, q8, lambda r, k: r.integers(-32768, 32768, (k, 64)).astype(np.int16))
    n2, _ = _run(rng, 30, 1000, q8, lambda r, k: sparse_blocks(r, k, -32768, 32767, 0.05))
    counts["int16"] = n1 + n2
    # 16-bit tables inside the int32 envelope
    n3, _ = _run(rng, 40, 1500, q16, lambda r, k: sparse_blocks(r, k, -300, 300, 0.1), envelope=True)
    n4, f4 = _run(rng, 20, 1500, q16, lambda r, k: sparse_blocks(r, k, -2, 2, 0.1), envelope=True)
    counts["q16"] = n3 + n4
    assert f4 > 0.5, f4
    assert counts["q16"] > 50000, counts
    assert sum(counts.values()) >= 200000, counts


@pytest.mark.parametrize("shift", [128, 2048, 1, 32768])
def test_single_coefficient_blocks_at_every_position(shift):
    """One coefficient at a time at each of the 64 positions, both signs, several sizes: one wrong IDCT constant or zig-zag
    entry moves samples of some block far beyond tau.  Shifts of precision 8, 12, 1 and 16."""
    for q_val in (1, 3, 255, 4097):
        q = np.full(64, q_val, np.uint16)
        zz = np.zeros((64 * 5 * 2, 64), np.int16)
        i = 0
        for k in range(64):
            for amp in (1, 7, 100, 1000, 32767):
                for sign in (1, -1):
                    zz[i, k] = sign * amp
                    i += 1
        check_tau_rule(oracle_blocks(zz, q, shift), zz, q, shift, min_exact_fraction=0.5, what=(q_val, shift))


def test_dc_only_ties_round_half_to_even():
    """DC-only blocks with |c*q| < 2^24 are exact in float32 (every sample is c*q / 8): at c*q = 8k + 4 every sample is a tie,
    and MathF.Round takes it to the even neighbour, the level shift added after."""
    q1 = np.ones(64, np.uint16)
    for cq, want in ((4, 0), (12, 2), (-4, 0), (-12, -2), (20, 2), (28, 4), (-20, -2), (-28, -4), (8004, 1000), (8012, 1002)):
        z = np.zeros((1, 64), np.int16)
        z[0, 0] = cq
        assert (oracle_blocks(z, q1, 0) == want).all(), cq
        assert (oracle_blocks(z, q1, 128) == want + 128).all(), cq
    for q_val, shift in ((1, 128), (3, 2048), (255, 128), (4095, 1), (65535, 32768)):
        c = np.array([c for c in range(-32768, 32768) if (c * q_val) % 8 == 4 and abs(c * q_val) < 2 ** 24], dtype=np.int64)
        assert len(c) > 0, q_val
        zz = np.zeros((len(c), 64), np.int16)
        zz[:, 0] = c
        got = oracle_blocks(zz, np.full(64, q_val, np.uint16), shift)
        half = c * q_val / 8
        assert (half - np.floor(half) == 0.5).all()
        want = ((np.rint(half).astype(np.int64) + shift + 32768) % 65536) - 32768
        assert np.array_equal(got, np.broadcast_to(want[:, None, None], got.shape)), q_val


def test_the_level_shift_wraps_at_16_bits():
    """(short)(Round + levelShift): DC 32767 with q = 255 is 1 044 448.125 in every sample, + 128, taken mod 2^16 as int16."""
    q = np.full(64, 255, np.uint16)
    for dc in (32767, -32768, 20000):
        z = np.zeros((1, 64), np.int16)
        z[0, 0] = dc
        got = oracle_blocks(z, q, 128)[0]
        r = int(np.rint(dc * 255 / 8))
        want = ((r + 128 + 32768) % 65536) - 32768
        assert want != r + 128
        assert (got == want).all(), dc
        check_tau_rule(got, z, q, 128)


def test_out_of_int32_samples_take_int_min_like_x64():
    """(int)MathF.Round(v) outside int32 is INT_MIN on x64 (cvttss2si): the sample is the low 16 bits of INT_MIN (0) plus the
    shift.  All 64 coefficients at 32767 with q = 65535: sample (0, 0) is about 1.5e10 and comes out as the shift."""
    q = np.full(64, 65535, np.uint16)
    for fill in (32767, -32768):
        z = np.full((1, 64), fill, np.int16)
        exact, _ = idct_float64(z, q)
        assert abs(exact[0, 0, 0]) > 2 ** 33
        far = np.abs(exact[0]) > 2.0 ** 31 * 1.01  # clear of float32's error at the edge
        near = np.abs(exact[0]) < 2.0 ** 31 * 0.99
        for shift in (128, 2048, 1):
            got = oracle_blocks(z, q, shift)[0]
            assert got[0, 0] == shift, (fill, shift)
            assert far.sum() >= 4 and (got[far] == shift).all(), (fill, shift)
            # inside the range the bound rule still holds
            r = np.rint(exact[0][near]).astype(np.int64)
            diff = ((got[near].astype(np.int64) - shift - r + 32768) % 65536) - 32768
            tau = TAU_SCALE * 64 * 65535 * abs(fill)
            assert (np.abs(diff + (r - exact[0][near])) <= 0.5 + tau).all()
