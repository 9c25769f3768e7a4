"""The sampler, CPU only: the oracle's bit-for-bit restatement of csrc/acmpc_device.h (log_spec, box_muller_spec,
uniform_open, candidate_normals, sample_segments, sample_candidates - what the kernels equal exactly) against a plain float64
evaluation written from DESIGN.md's definitions (tests/sampler_reference64.py), so that an error the kernel and its
restatement share - a coefficient, a sign, a word of the counter - does not pass; and against what the numbers are meant
to be: standard normal and independent across everything that distinguishes two draws.

`python tests/test_sampler_float64.py` prints the measured maxima and statistics the constants and comments below quote."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "ac-mpc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acmpc_oracle as orc  # noqa: E402
import sampler_reference64 as r64  # noqa: E402

# Tolerances: the largest error of the restatement against the float64 reference on THIS file's inputs (its __main__
# prints them), times 2: the float32 side is exact arithmetic and the same everywhere, the float64 side's libm moves in its
# last place.  Measured (NumPy 2.2, x86-64):
#   log_spec       |l32 - l64| / |l64|   7.827e-8 (u = 0.362588495) over log_inputs(), 283 246 floats
#                  |l32 - l64|           9.386e-7 (u = 4.21468371e-8, ln u = -16.98)
#   box_muller     |z32 - z64|           6.747e-7 over NORMAL_CASES (the 131 072 candidates x 16 of the first; 5.3e-7 to 6.4e-7
#                                        on each set of 32 768, 4.3e-7 on the sets of 300), 3.668e-7 on angle_grid()
#   candidates     (|U32 - U64| - 2^-24 |U64|) / sigma   4.835e-7 over CANDIDATE_CASES
LOG_RTOL = 2 * 7.827e-8
LOG_ATOL = 2 * 9.386e-7
Z_ATOL = 2 * 6.747e-7
U_TOL = 2 * 4.835e-7      # in units of sigma, beside half a float32 ulp of the control itself (the last addition's rounding)
HALF_ULP = 2.0 ** -24

# Seeds, fixed before any statistic was looked at: the one tests/test_gpu_sharded.py draws with, its low word + 1, its
# high word ^ 1.  What the restatement gives at them (this file's __main__; 131 072 candidates = 2 097 152 normals for the
# moments, 32 768 candidates = 524 288 normals per pairing), every figure in standard errors:
#   mean +0.89  variance +2.40  skewness +0.67  excess kurtosis -0.96  Kolmogorov-Smirnov D sqrt M 0.95  largest |z| 4.89
#   pair 0.16  squares of a pair 1.32  block 0.86  neighbouring knots 1.10  any two knots 3.05 (the largest of 112)
#   c / c + 1  0.20   c / c + 8  0.31   problems 0 / 1  1.33   rounds 0 / 1  0.36   seed / low word + 1  0.20
#   seed / high word ^ 1  0.93
SEED = 0x1234567899
SEED_LOW = SEED + 1
SEED_HIGH = SEED ^ (1 << 32)
N_MOMENTS = 1 << 17
N_PAIRING = 1 << 15
SIGMAS = 5.0        # every moment and every correlation within this many standard errors
KS_LIMIT = 2.0      # D sqrt M; the asymptotic tail beyond it is 2 exp(-2 * 2.0^2) = 7e-4

HORIZONS = [1, 2, 3, 7, 8, 9, 15, 49, 50, 128, 1024]
N_SET = 40          # candidates per set: the three special ones and every amplitude level four times over
OFFSETS = [0, 3, (1 << 31) - 5, (1 << 32) - 1 - N_SET]       # the last: the largest acmpc_sample_device accepts
U_LO, U_HI = (5.0, -0.12), (40.0, 0.12)
SIGMA = (3.0, 0.01)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def log_inputs():
    """float32 uniforms: every 61st of the 2^24, the first and the last 4 096 (2^-25 and 1.0 among them), and for every
    binade a uniform reaches the three floats either side of the mantissa break 0x3f3504f3 (where e steps)."""
    k = np.unique(np.concatenate([np.arange(0, 1 << 24, 61), np.arange(4096), np.arange((1 << 24) - 4096, 1 << 24)]))
    u = r64.uniforms64(k.astype(np.uint32) << 8).astype(np.float32)
    e = np.arange(-24, 1, dtype=np.int32)                         # break * 2^e lies in [2^-25, 1] for these
    breaks = (np.int32(0x3F3504F3) + (e[:, None] << 23) + np.arange(-3, 3, dtype=np.int32)[None, :]).astype(np.int32)
    edge = breaks.ravel().view(np.float32)
    assert edge.min() >= 2.0 ** -25 and edge.max() <= 1.0
    return np.concatenate([u, edge, np.float32([1.0, 2.0 ** -25])])


def angle_grid():
    """(u1, u2): u2 at and one float either side of 0, 1/4, 1/2, 3/4 and 1 - where the reduction's k changes and the
    parity flips - against radii from the largest (u1 = 2^-25) to none (u1 = 1)."""
    u2 = np.float32([0.0, 0.25, 0.5, 0.75, 1.0])
    u2 = np.concatenate([np.nextafter(u2, np.float32(-1.0)), u2, np.nextafter(u2, np.float32(2.0))])
    u1 = np.float32([2.0 ** -25, 3.0 * 2.0 ** -25, 1.0e-3, 0.3, 0.5, 0.70710677, 1.0 - 2.0 ** -24, 1.0])
    a, b = np.meshgrid(u1, u2, indexing="ij")
    return a.ravel(), b.ravel()


_CACHE = {}
_PRISTINE = dict(philox=orc.philox4x32_10, box_muller=orc.box_muller_spec, ln2_lo=orc.LN2_LO, amp=orc.candidate_amplitude)


def orc_is_untouched():
    """False while test_a_planted_defect_fails_the_named_checks has a defect in the oracle."""
    return (orc.philox4x32_10 is _PRISTINE["philox"] and orc.box_muller_spec is _PRISTINE["box_muller"]
            and orc.LN2_LO == _PRISTINE["ln2_lo"] and orc.candidate_amplitude is _PRISTINE["amp"])


def restated_normals(N, offset, problem, rnd, seed):
    """oracle.candidate_normals, kept: the tests draw a set once (a shorter set is the head of a longer one)."""
    key = (offset, problem, rnd, seed)
    if key not in _CACHE or _CACHE[key].shape[0] < N:
        _CACHE[key] = orc.candidate_normals(N, offset, problem, rnd, seed)[1]
    return _CACHE[key][:N]


def draw(N, offset, problem, rnd, seed):
    """The restatement's normals z [N, 8, 2] as the oracle stands NOW: from the cache unless a defect is planted."""
    if orc_is_untouched():
        return restated_normals(N, offset, problem, rnd, seed)
    return orc.candidate_normals(N, offset, problem, rnd, seed)[1]


def problem_inputs(n, seed=5):
    """centre, u_ref, u_extra [n, 2] float32 inside and outside the box (the clip has work to do)."""
    rng = np.random.default_rng(seed + n)
    centre = np.column_stack([rng.uniform(4.0, 41.0, n), rng.uniform(-0.13, 0.13, n)]).astype(np.float32)
    u_ref = np.column_stack([rng.uniform(4.0, 41.0, n), rng.uniform(-0.13, 0.13, n)]).astype(np.float32)
    u_extra = np.column_stack([rng.uniform(4.0, 41.0, n), rng.uniform(-0.13, 0.13, n)]).astype(np.float32)
    return centre, u_ref, u_extra


# (n, offset, problem, round, seed, with u_ref, with u_extra): every horizon with and without the given candidates at every
# offset; problems, rounds and both key words away from zero
CANDIDATE_CASES = [(n, off, (3 * i + j) % 5, (i + 2 * j) % 4, (SEED, SEED_HIGH + 77)[(i + j) % 2], given, given)
                   for i, n in enumerate(HORIZONS) for j, off in enumerate(OFFSETS) for given in (True, False)]
CANDIDATE_CASES += [(49, 0, 1, 1, SEED, True, False), (8, 0, 2, 0, SEED, False, True)]


# ---- the checks, each usable on a planted defect ------------------------------------------------------------------------------
def log_errors():
    u = log_inputs()
    l32 = orc.log_spec(u).astype(np.float64)
    l64 = np.log(u.astype(np.float64))
    err = np.abs(l32 - l64)
    zero = l64 == 0.0
    return dict(u=u, err=err, rel=np.where(zero, 0.0, err / np.where(zero, 1.0, np.abs(l64))), at_one=l32[zero])


def check_log():
    f = log_errors()
    assert f["at_one"].size >= 2 and np.all(f["at_one"] == 0.0), "log_spec(1) is not 0"
    assert f["rel"].max() <= LOG_RTOL, "log_spec: relative error %.3e at u = %.9g" % (f["rel"].max(), f["u"][np.argmax(f["rel"])])
    assert f["err"].max() <= LOG_ATOL, "log_spec: absolute error %.3e at u = %.9g" % (f["err"].max(), f["u"][np.argmax(f["err"])])


def box_muller_errors(u1, u2):
    got = np.stack(orc.box_muller_spec(u1, u2)).astype(np.float64)
    return np.abs(got - np.stack(r64.box_muller64(u1, u2)))


def check_box_muller_grid():
    err = box_muller_errors(*angle_grid())
    assert err.max() <= Z_ATOL, "box_muller_spec on the grid: %.3e" % err.max()


def check_normals(N, offset, problem, rnd, seed):
    """oracle.candidate_normals against the float64 normals: the transform AND the counter, the key and the word order."""
    z32 = draw(N, offset, problem, rnd, seed)
    gidx, z64 = r64.normals64(N, offset, problem, rnd, seed)
    err = np.abs(z32.astype(np.float64) - z64)
    assert err.max() <= Z_ATOL, "normals at offset %d problem %d round %d seed %#x: %.3e" % (offset, problem, rnd, seed, err.max())
    assert np.abs(z32).max() <= r64.Z_MAX + Z_ATOL
    return float(err.max())


def check_moments(N=N_MOMENTS):
    z = draw(N, 0, 0, 0, SEED)
    f = r64.moment_figures(z)
    for name in ("mean", "variance", "skewness", "kurtosis"):
        assert abs(f[name]) <= SIGMAS, "%s is %.2f standard errors off" % (name, f[name])
    assert f["largest"] <= r64.Z_MAX + Z_ATOL
    ks = r64.ks_figure(z)
    assert ks <= KS_LIMIT, "Kolmogorov-Smirnov D sqrt M = %.2f" % ks
    return dict(f, ks=ks)


def pairing_figures(N=N_PAIRING):
    """|rho| sqrt M of everything that tells two draws apart."""
    z = draw(N, 0, 0, 0, SEED)
    out = r64.within_candidate_figures(z)
    out["c / c + 1"] = r64.correlation_figure(z[:-1], z[1:])
    out["c / c + 8"] = r64.correlation_figure(z[:-8], z[8:])
    out["problems"] = r64.correlation_figure(z, draw(N, 0, 1, 0, SEED))
    out["rounds"] = r64.correlation_figure(z, draw(N, 0, 0, 1, SEED))
    out["key low word"] = r64.correlation_figure(z, draw(N, 0, 0, 0, SEED_LOW))
    out["key high word"] = r64.correlation_figure(z, draw(N, 0, 0, 0, SEED_HIGH))
    return out


def check_pairings(N=N_PAIRING, only=None):
    for name, figure in pairing_figures(N).items():
        if only is None or name in only:
            assert figure <= SIGMAS, "correlation across %s: |rho| sqrt M = %.2f" % (name, figure)


def candidate_sides(case, N=N_SET):
    n, offset, problem, rnd, seed, with_ref, with_extra = case
    centre, u_ref, u_extra = problem_inputs(n)
    args = (centre, u_ref if with_ref else None, N, offset, problem, rnd, seed, SIGMA, U_LO, U_HI)
    extra = u_extra if with_extra else None
    return (orc.sample_candidates(*args, u_extra=extra), r64.candidates64(*args, u_extra=extra), centre,
            u_ref if with_ref else None, extra)


def candidate_excess(U32, U64, sigma):
    """(|U32 - U64| - half a float32 ulp of the control) / sigma per component, at least 0: what U_TOL bounds."""
    err = np.abs(U32.astype(np.float64) - U64) - HALF_ULP * np.abs(U64)
    return np.maximum(err, 0.0) / np.asarray(sigma, dtype=np.float32).astype(np.float64)


def check_candidates(case, N=N_SET):
    U32, U64, centre, u_ref, u_extra = candidate_sides(case, N)
    n, offset = case[0], case[1]
    assert U32.shape == (N, n, 2) and U32.dtype == np.float32 and np.all(np.isfinite(U32)), case
    excess = candidate_excess(U32, U64, SIGMA)
    assert excess.max() <= U_TOL, "%r: %.3e sigma at %s" % (case, excess.max(), np.unravel_index(np.argmax(excess), excess.shape))
    lo, hi = np.float32(U_LO), np.float32(U_HI)
    assert np.all(U32 >= lo) and np.all(U32 <= hi), case
    if offset == 0:
        assert np.array_equal(U32[0], np.clip(centre, lo, hi)), case
        if u_ref is not None:
            assert np.array_equal(U32[1], np.clip(u_ref, lo, hi)), case
        if u_extra is not None:
            assert np.array_equal(U32[2], np.clip(u_extra, lo, hi)), case
    return float(excess.max())


SPREAD_N, SPREAD_CANDIDATES = 49, 1 << 16


def spread_figures(N=SPREAD_CANDIDATES):
    """n = 49 in a box that never clips: per amplitude level and step, (s - sigma amp sqrt(w0^2 + w1^2)) in standard errors
    of s, with s^2 the mean square about the centre and SE(s) = s / sqrt(2 M) for M normal deviates."""
    n = SPREAD_N
    centre = np.zeros((n, 2), dtype=np.float32)
    sigma = (1.0, 0.25)
    U = orc.sample_candidates(centre, None, N, 8, 0, 0, SEED, sigma, (-100.0, -100.0), (100.0, 100.0)).astype(np.float64)
    gidx = 8 + np.arange(N)
    factor = r64.spread_factor(n)
    worst = 0.0
    for level in range(8):
        rows = U[(gidx & 7) == level]
        M = rows.shape[0]
        s = np.sqrt(np.mean(rows * rows, axis=0))                                   # [n, 2]
        want = np.float32(sigma).astype(np.float64)[None, :] * ((level + 1) / 8.0) * factor[:, None]
        worst = max(worst, float(np.max(np.abs(s - want) / (want / np.sqrt(2.0 * M)))))
    return worst


def check_spread(N=SPREAD_CANDIDATES):
    worst = spread_figures(N)
    assert worst <= SIGMAS, "a step's spread is %.2f standard errors from sigma amp sqrt(w0^2 + w1^2)" % worst


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_uniform_open_is_the_rounded_midpoint_in_0_1_closed():
    """Every one of the 2^24 values: the float32 nearest (k + 1/2) 2^-24; 1.0 for k = 2^24 - 1 alone, 2^-25 the smallest,
    never 0; the low 8 bits of the word do not matter.  Hence |z| <= sqrt(-2 ln 2^-25) = sqrt(50 ln 2) = 5.8871."""
    k = np.arange(1 << 24, dtype=np.uint32)
    u = orc.uniform_open(k << 8)
    assert u.dtype == np.float32
    assert np.array_equal(u, ((k.astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32))
    assert np.array_equal(u, orc.uniform_open((k << 8) | np.uint32(0xFF)))
    assert np.array_equal(np.flatnonzero(u == 1.0), [(1 << 24) - 1])
    assert u.min() == np.float32(2.0 ** -25) and np.argmin(u) == 0 and u.max() == 1.0
    assert abs(r64.Z_MAX - 5.8871) < 5e-5
    # the two ends through the transform: u = 1 gives ln = +0, a radius of -0 and normals of +-0; u = 2^-25 the largest radius
    z0, z1 = orc.box_muller_spec(np.float32([1.0, 1.0, 1.0]), np.float32([0.1, 0.4, 0.9]))
    assert np.all(z0 == 0.0) and np.all(z1 == 0.0) and orc.log_spec(np.float32(1.0))[0] == 0.0
    u2 = orc.uniform_open(np.arange(0, 1 << 32, 1 << 14, dtype=np.uint64).astype(np.uint32))
    z0, z1 = orc.box_muller_spec(np.full(u2.shape, 2.0 ** -25, dtype=np.float32), u2)
    radius = np.hypot(z0.astype(np.float64), z1.astype(np.float64))
    assert radius.max() <= r64.Z_MAX + Z_ATOL and radius.min() >= r64.Z_MAX - Z_ATOL
    assert max(np.abs(z0).max(), np.abs(z1).max()) <= r64.Z_MAX + Z_ATOL


def test_log_spec_against_the_library_logarithm():
    check_log()


def test_box_muller_spec_against_library_functions():
    check_box_muller_grid()
    _, u = r64.block_uniforms(1 << 14, 0, 0, 0, SEED)          # Philox-drawn: the float32 uniforms of 16 384 candidates
    u = u.astype(np.float32)
    err = np.concatenate([box_muller_errors(u[..., 0], u[..., 1]), box_muller_errors(u[..., 2], u[..., 3])])
    assert err.max() <= Z_ATOL


# (N, offset, problem, round, seed): the sets the statistics below use, and the ends of every word of counter and key
NORMAL_CASES = [(N_MOMENTS, 0, 0, 0, SEED), (N_PAIRING, 0, 1, 0, SEED), (N_PAIRING, 0, 0, 1, SEED),
                (N_PAIRING, 0, 0, 0, SEED_LOW), (N_PAIRING, 0, 0, 0, SEED_HIGH), (300, (1 << 32) - 301, 3, 2, SEED_LOW),
                (300, (1 << 31) - 5, 7, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF)]


@pytest.mark.parametrize("N,offset,problem,rnd,seed", NORMAL_CASES)
def test_restated_normals_against_float64(N, offset, problem, rnd, seed):
    check_normals(N, offset, problem, rnd, seed)


def test_restated_normals_are_standard_normal():
    check_moments()


def test_restated_normals_are_uncorrelated_across_everything_that_tells_two_draws_apart():
    check_pairings()


@pytest.mark.parametrize("n", HORIZONS)
def test_candidate_sets_against_float64(n):
    cases = [c for c in CANDIDATE_CASES if c[0] == n]
    assert len(cases) >= 2 * len(OFFSETS)
    for case in cases:
        check_candidates(case)


def test_one_step_horizon_is_knot_zero():
    """n = 1: upload_segments puts the step on knot 0 with weight 1, so a candidate is centre + sigma amp z_0."""
    assert np.array_equal(orc.sample_segments(1), np.float32([[0.0, 1.0]]))
    k, w0 = r64.knots64(1)
    assert k.tolist() == [0] and w0.tolist() == [1.0]
    centre = np.float32([[20.0, 0.01]])
    U = orc.sample_candidates(centre, None, 16, 0, 0, 0, SEED, SIGMA, U_LO, U_HI)
    z = restated_normals(N_MOMENTS, 0, 0, 0, SEED)[:16, 0, :]
    want = centre + (np.float32(SIGMA)[None, :] * orc.candidate_amplitude(np.arange(16))[:, None]) * z
    assert np.array_equal(U[:, 0, :], np.clip(want, np.float32(U_LO), np.float32(U_HI)))


def knot_table_worst_last_weight():
    worst = 0.0
    for n in range(2, 1025):
        seg = orc.sample_segments(n)
        k, w0 = seg[:, 0], seg[:, 1]
        assert seg.dtype == np.float32 and seg.shape == (n, 2), n
        assert np.all(k == np.floor(k)) and np.all(np.diff(k) >= 0) and k.min() == 0 and k.max() <= 6, n
        assert np.all(w0 >= 0.0) and np.all(w0 <= 1.0), n
        assert k[0] == 0 and w0[0] == 1.0, n
        assert k[-1] == 6, n                                    # the last step: knot 7 = the right knot of segment 6
        worst = max(worst, float(w0[-1]))
        k64, w64 = r64.knots64(n)
        # the positions are quotients rounded in float64: where one lands a rounding below a knot the restatement holds the
        # previous segment with a weight of ~0 for the reference's next segment with a weight of 1 - the same blend
        same = k == k64
        assert np.all(np.abs(w0[same] - w64[same]) <= 2.0 ** -24), n
        assert np.all((k[~same] == k64[~same] - 1) & (w0[~same] <= 2.0 ** -24) & (w64[~same] >= 1.0 - 2.0 ** -24)), n
    return worst


def test_knot_table_for_every_horizon():
    """n = 2 .. 1 024: left knots whole, non-decreasing and at most 6, weights in [0, 1], weight 1 at step 0, the last step
    on knot 7.  Its weight is exactly 0 at every n (measured maximum 0.0: cos of a float64 within 2^-52 of pi is -1)."""
    assert knot_table_worst_last_weight() == 0.0
    assert np.array_equal(orc.sample_segments(8), np.float32([[0, 1], [1, 1], [2, 1], [3, 1], [4, 1], [5, 1], [6, 1], [6, 0]]))


def test_spread_per_step_and_amplitude_level():
    """A step's noise is w0 z_k + (1 - w0) z_{k+1}: standard deviation sigma amp sqrt(w0^2 + (1 - w0)^2), down to 0.71 sigma
    amp midway between two knots.  Measured: the worst of 49 steps x 8 levels x 2 controls is 3.67 standard errors off."""
    factor = r64.spread_factor(SPREAD_N)
    assert factor.max() == 1.0 and abs(factor.min() - np.sqrt(0.5)) < 1e-3
    check_spread()


# ---- the tests have teeth ---------------------------------------------------------------------------------------------------
def _without_parity(u1, u2):
    """box_muller_spec with the sign of the angle's half-turn count ignored"""
    z0, z1 = _PRISTINE["box_muller"](u1, u2)
    t = orc.fma32(np.atleast_1d(np.asarray(u2, dtype=np.float32)), np.float32(2.0), np.float32(orc.ROUND_MAGIC))
    odd = (np.atleast_1d(t).view(np.int32) & 1) != 0
    return np.where(odd, -z0, z0).astype(np.float32), np.where(odd, -z1, z1).astype(np.float32)


def _philox_without(counter_word=None, key_word=None):
    def philox(counter, key):
        counter, key = np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32)
        if counter_word is not None:
            counter[..., counter_word] = 0
        if key_word is not None:
            key[..., key_word] = 0
        return _PRISTINE["philox"](counter, key)
    return philox


def _amplitude_from_two_bits(gidx):
    gidx = np.asarray(gidx, dtype=np.uint32)
    amp = ((gidx & 3) + 1).astype(np.float32) * np.float32(0.125)
    amp[gidx == 0] = np.float32(0.0)
    return amp


SMALL = 1 << 12
# defect -> (attribute of the oracle, its replacement, the checks that must fail: name -> call)
DEFECTS = {
    "the sign parity of the angle ignored": ("box_muller_spec", _without_parity, {
        "box_muller_spec on the grid": check_box_muller_grid,
        "the normals against float64": lambda: check_normals(SMALL, 0, 0, 0, SEED),
        "the moments (mean)": lambda: check_moments(SMALL)}),
    "LN2_LO dropped": ("LN2_LO", 0.0, {
        "log_spec against the library logarithm": check_log,
        "the normals against float64": lambda: check_normals(SMALL, 0, 0, 0, SEED)}),
    "the draw index q left out of the counter": ("philox4x32_10", _philox_without(counter_word=3), {
        "the normals against float64": lambda: check_normals(SMALL, 0, 0, 0, SEED),
        "the correlation of any two knots": lambda: check_pairings(SMALL, only=("knots",))}),
    "the key's high word ignored": ("philox4x32_10", _philox_without(key_word=1), {
        "the normals against float64": lambda: check_normals(SMALL, 0, 0, 0, SEED),
        "the correlation across the key's high word": lambda: check_pairings(SMALL, only=("key high word",))}),
    "the problem index ignored": ("philox4x32_10", _philox_without(counter_word=1), {
        "the normals against float64": lambda: check_normals(SMALL, 0, 1, 0, SEED),
        "the correlation across problems": lambda: check_pairings(SMALL, only=("problems",))}),
    "the round ignored": ("philox4x32_10", _philox_without(counter_word=2), {
        "the normals against float64": lambda: check_normals(SMALL, 0, 0, 1, SEED),
        "the correlation across rounds": lambda: check_pairings(SMALL, only=("rounds",))}),
    "amp taken from c & 3": ("candidate_amplitude", _amplitude_from_two_bits, {
        "the candidate set against float64": lambda: check_candidates((49, 0, 1, 1, SEED, True, False)),
        "the spread per amplitude level": lambda: check_spread(SMALL)}),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_a_planted_defect_fails_the_named_checks(defect, monkeypatch):
    """Each defect is planted in the oracle's restatement for the length of this test (nothing in the tree changes) and
    must fail every check named beside it; the same checks pass on the restatement as it stands."""
    attribute, replacement, checks = DEFECTS[defect]
    for check in checks.values():
        check()
    monkeypatch.setattr(orc, attribute, replacement)
    assert not orc_is_untouched()
    for name, check in checks.items():
        try:
            check()
        except AssertionError:
            continue
        pytest.fail("%s: not noticed by %s" % (defect, name))
    monkeypatch.undo()
    assert orc_is_untouched()


if __name__ == "__main__":
    f = log_errors()
    i, j = int(np.argmax(f["rel"])), int(np.argmax(f["err"]))
    print("log_spec over %d inputs: relative %.3e (u = %.9g)  absolute %.3e (u = %.9g, ln u = %.2f)"
          % (f["u"].size, f["rel"][i], f["u"][i], f["err"][j], f["u"][j], np.log(float(f["u"][j]))))
    print("box_muller_spec on the grid of %d: %.3e" % (angle_grid()[0].size, box_muller_errors(*angle_grid()).max()))
    for case in NORMAL_CASES:
        print("normals, %6d candidates x 16 at offset %d problem %d round %d seed %#x: %.3e" % (*case, check_normals(*case)))
    worst = max(float(candidate_excess(*candidate_sides(case)[:2], SIGMA).max()) for case in CANDIDATE_CASES)
    print("candidates over %d cases: (|U32 - U64| - 2^-24 |U64|) / sigma %.3e" % (len(CANDIDATE_CASES), worst))
    m = check_moments()
    print("moments of %d normals, in standard errors: mean %+.2f variance %+.2f skewness %+.2f excess kurtosis %+.2f  "
          "KS D sqrt M %.2f  largest |z| %.2f" % (m["M"], m["mean"], m["variance"], m["skewness"], m["kurtosis"], m["ks"], m["largest"]))
    print("pairings, |rho| sqrt M: " + "  ".join("%s %.2f" % kv for kv in pairing_figures().items()))
    print("spread at n = %d, worst of steps x levels x controls: %.2f standard errors" % (SPREAD_N, spread_figures()))
    print("knot table, n = 2 .. 1024: largest weight of the last step %.3e" % knot_table_worst_last_weight())
