"""tests/softmin_reference64.py without a GPU: the exact inputs' expected values against rational arithmetic, mean64 against
a mean worked out by hand, and the condition on the general inputs that makes the GPU test worth its tolerance - a candidate
dropped, counted twice, or weighted with its neighbour's weight moves the mean by at least 100 tolerances at every shape the
GPU test runs."""
from fractions import Fraction

import numpy as np
import pytest

import acmpc_oracle as orc
import softmin_reference64 as sr
from acmpc_amd import _capi

P = sr.P
LAM = np.float32(sr.LAMBDA)


def _key_cost(d, p):
    return _capi.key_cost(int(d["keys"][p]))


@pytest.mark.parametrize("shape", [(2, 1), (2, 2), (3, 65), (85, 63), (129, 300), (9, 2049)], ids=lambda s: "n%d_N%d" % s)
def test_the_exact_inputs_expect_what_rational_arithmetic_gives(shape):
    n, N = shape
    d = sr.exact_problem(P, N, n)
    assert d["costs"].dtype == np.float32 and d["U"].dtype == np.float32
    k = d["U"].astype(np.float64) / sr.DYADIC
    held = ~np.isnan(k)
    assert np.all(k[held] == np.rint(k[held])) and np.abs(k[held]).max() < 2 ** 15      # dyadic: integers times 2^-8
    for p in range(P):
        finite = np.isfinite(d["costs"][p])
        assert np.array_equal(finite, d["mask"][p]) and np.all(d["costs"][p][finite] == np.float32(sr.EXACT_COST))
        rest = d["costs"][p][~finite]
        assert np.all(np.isnan(rest) | (rest == np.inf)) and (rest.size < 2 or (np.isnan(rest).any() and np.isinf(rest).any()))
        count = int(finite.sum())
        assert (count == 0) == (p == P - 1) and d["weight_sum"][p] == count
        assert _key_cost(d, p) == sr.EXACT_COST or p == P - 1
        rows = np.flatnonzero(finite) if count else np.arange(N)           # all non-finite: the plain mean of all N
        assert not np.isnan(d["U"][p][rows]).any()
        if p < P - 1 and N - count >= 1:
            assert np.isnan(d["U"][p][~finite]).any()                      # NaN controls under a weight of 0
        for e in range(2 * n):
            total = sum((Fraction(float(u)) for u in d["U"][p].reshape(N, 2 * n)[rows, e]), Fraction(0))
            assert Fraction(float(total)) == total                          # the sum is a float64: no order can change it
            assert np.float32(float(total) / len(rows)).tobytes() == d["mean"][p].reshape(-1)[e].tobytes(), (p, e)
        # and mean64 gives the same bits on them
        m, wsum, _ = sr.mean64(d["costs"][p], _key_cost(d, p), d["U"][p], LAM)
        assert wsum == count and np.array_equal(m.astype(np.float32).view(np.uint32), d["mean"][p].view(np.uint32))


def test_the_exact_controls_tell_problems_candidates_and_entries_apart():
    U = sr.exact_controls(P, 2049, 129)
    flat = U.reshape(P, 2049, 258)
    assert np.all(flat[:, 1:] != flat[:, :-1]) and np.all(flat[:, :, 1:] != flat[:, :, :-1]) and np.all(flat[1:] != flat[:-1])
    assert np.all(np.roll(flat, 64, axis=1) != flat) and np.all(np.roll(flat, 1024, axis=1) != flat)     # a wave, a chunk away
    assert np.all(np.roll(flat, 256, axis=2)[:, :, :2] != flat[:, :, :2])                                # a pass away
    sums = flat.astype(np.float64).sum(axis=1)
    assert np.unique(sums[0]).size > 250                                    # entries do not share their sums


def test_mean64_is_the_contract_on_a_hand_sized_problem():
    costs = np.array([1.0, 1.5, np.nan, 3.0, np.inf], dtype=np.float32)
    U = np.array([[[1.0, -2.0]], [[3.0, 0.5]], [[np.nan, np.nan]], [[-1.0, 4.0]], [[100.0, np.nan]]], dtype=np.float32)
    w = [1.0, float(np.exp(-1.0)), 0.0, float(np.exp(-4.0)), 0.0]
    m, wsum, s = sr.mean64(costs, 1.0, U, LAM)
    assert wsum == pytest.approx(w[0] + w[1] + w[3], rel=1e-15)
    for comp in range(2):
        u = [float(v) for v in U[:, 0, comp]]
        want = (w[0] * u[0] + w[1] * u[1] + w[3] * u[3]) / (w[0] + w[1] + w[3])
        assert m[0, comp] == pytest.approx(want, rel=1e-15)
        scale = w[0] * 1 * abs(u[0] - want) + w[1] * 2 * abs(u[1] - want) + w[3] * 5 * abs(u[3] - want)
        assert s[0, comp] == pytest.approx(scale / (w[0] + w[1] + w[3]), rel=1e-14)
    # the key's cost is the minimum the weights are taken against, whatever the costs say
    m2, wsum2, _ = sr.mean64(costs, 0.5, U, LAM)
    assert wsum2 == pytest.approx(wsum * float(np.exp(-1.0)), rel=1e-15) and np.allclose(m2, m, rtol=1e-15)
    # no finite cost: the plain mean over all N, weight sum 0; NaN controls are then in it
    none = np.array([np.nan, np.inf, np.nan], dtype=np.float32)
    m3, wsum3, s3 = sr.mean64(none, float("nan"), U[[0, 1, 3]], LAM)
    assert wsum3 == 0.0 and np.array_equal(m3, [[1.0, 2.5 / 3.0]])
    assert np.isnan(sr.mean64(none, float("nan"), U[[0, 1, 2]], LAM)[0]).all()
    assert np.array_equal(sr.error_r(m3.astype(np.float32), m3, s3) <= 0.5, [[True, True]])


SHAPES = sr.MATRIX_SHAPES + [sr.CAPACITY_SHAPE, sr.SHAPE_AFTER_CAPACITY]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_N%d" % s)
def test_the_general_inputs_discriminate(shape):
    """A condition on the inputs, not a measurement: in units of r, dropping any one candidate that carries at least 1e-3 of the
    largest weight, counting it twice, or pairing the weights with the candidates shifted by one moves some entry of the
    mean by at least 100 R_TOL.  (N = 1 has nothing to drop: its mean is its candidate.  Under the uniform fallback a shift
    of the weights changes nothing, so the last problem is held to the first two.)  And the oracle's float32 weights, summed
    in float64 and rounded once - what the device should be doing - are within R_TOL."""
    n, N = shape
    d = sr.general_problem(P, N, n)
    x = (d["costs"][:P - 1].astype(np.float64) - 1.5) / sr.LAMBDA
    assert np.nanmin(x) >= 0.0 and np.all(x[np.isfinite(x)] <= 6.0 + 1e-6) and not np.isfinite(d["costs"][P - 1]).any()
    assert np.isnan(d["U"][:P - 1]).any() or N < 3
    for p in range(P):
        m, s, removed, doubled, shifted = sr.perturbed_means(d["costs"][p], _key_cost(d, p), d["U"][p], LAM)
        unit = sr.EPS * (s + np.abs(m))
        assert removed.shape[0] == (np.isfinite(d["costs"][p]).sum() if p < P - 1 else N)      # every weight is above the floor
        if N > 1:
            for what, moved in (("dropped", removed), ("counted twice", doubled)):
                r = (np.abs(moved - m) / unit).max(axis=(1, 2))
                assert r.min() >= 100.0 * sr.R_TOL, "%s: candidate %d moves the mean by r = %.1f only" % (what, int(r.argmin()), r.min())
            if p < P - 1:
                assert (np.abs(shifted - m) / unit).max() >= 100.0 * sr.R_TOL
        if p < P - 1:
            w = orc.softmin_weights(d["costs"][p], sr.LAMBDA).astype(np.float64)
            got = (np.tensordot(w, np.where(np.isnan(d["U"][p]), 0.0, d["U"][p]).astype(np.float64), axes=(0, 0)) / w.sum())
            assert sr.error_r(got.astype(np.float32), m, s).max() <= sr.R_TOL
            assert abs(w.sum() - sr.mean64(d["costs"][p], _key_cost(d, p), d["U"][p], LAM)[1]) <= sr.WSUM_RTOL * w.sum()
