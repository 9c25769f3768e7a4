"""The softmin (MPPI) mean in float64, and the inputs its GPU tests run on (tests/test_gpu_softmin_float64.py; checked
without a GPU by tests/test_softmin_reference64.py).  A helper of the tests, not a test file; it runs no device code.

The contract, as csrc/acmpc_softmin.hip's comments state it: for one problem with costs c [N] float32, the cost c_min held in
its key, controls u [N, n, 2] float32 and lambda float32,

    w_c = exp(-(c_c - c_min) / lambda), 0 for a non-finite cost
    m   = sum_c w_c u_c / sum_c w_c     over the candidates with w_c != 0 only: a zero-weight candidate is excluded even when
                                        its controls are NaN
    the plain mean sum_c u_c / N over ALL candidates when sum_c w_c is not positive

and the weight sum.  `mean64` evaluates that in float64 on the float32 inputs.

Two kinds of input:

    exact      one finite cost repeated on an irregular subset of the candidates, NaN and +inf alternating on the rest: every
               weight is exactly 1 or 0.  Controls are integers of magnitude below 2^15 times 2^-8 that depend on (p, c, e), so
               every float64 sum of at most 2^11 of them is exact in any order, the mean is float32(float64(sum) / count) and
               the weight sum is the count.  No tolerance.
    general    costs seeded in c_min + lambda [0, 6], NaN / +inf planted as test_gpu_dynamic_softmin._synthetic_costs plants
               them, the last problem all non-finite; controls arbitrary floats of magnitude about 1 that differ by about 1
               from candidate to candidate.  The error of a result is measured per entry in units of what float32 can hold:

                   x_c = (c_c - c_min) / lambda,  s = sum_c w_c (1 + x_c) |u_c - m| / sum_c w_c
                   r   = |got - m| / (2^-24 (s + |m|))

               A float32 exp of a float32 quotient carries a relative error of about (1 + x_c) 2^-24 in w_c, which moves m by
               at most about 2^-24 s; rounding m to float32 adds 2^-24 |m| / 2: r of a few units is what that arithmetic
               gives, and r far above that is another computation.
"""
from __future__ import annotations

import numpy as np

T = np.float32
EPS = 2.0 ** -24
LAMBDA = 0.5            # the handles' softmin_lambda
EXACT_COST = 2.75       # the one finite cost of the exact inputs
DYADIC = 2.0 ** -8

# The shapes (n, N) acmpc_softmin_device runs at in tests/test_gpu_softmin_float64.py, P = 3 problems each, the last all
# non-finite.  n: a row of 2n floats fits the 256-thread workgroup 64 times | twice | once with 86 threads idle | with 2 idle |
# exactly | takes a second pass of 2 entries | two full passes | four; every n with N = 1025 (a chunk of one candidate behind
# a full one) and N = 1.  N at n = 129: a lone candidate, two, round the wavefront, round the chunk of 1 024, three chunks.
# n = 1 cannot be run: the tables a call's n must match have at least two steps (acmpc_set_paths, acmpc_set_coefficients).
P = 3
STEPS = (2, 64, 85, 127, 128, 129, 256, 512)
CANDIDATES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
MATRIX_SHAPES = sorted({(n, N) for n in STEPS for N in (1025, 1)} | {(129, N) for N in CANDIDATES})
CAPACITY_SHAPE = (1024, 1025)      # mode S only (mode D ends at 512 steps): eight passes, on a handle of exactly this capacity
SHAPE_AFTER_CAPACITY = (129, 65)   # ... and a smaller call on that handle behind it

# max r of acmpc_softmin_device against mean64 over the general inputs of every shape above, both layouts, handles of mode S
# and mode D, and the matrix side of the sampled shapes, measured on the MI355X; the tests hold 4 x that (the margin of the
# project's other float64 mirrors).  The weight sum: its relative error, in units of 2^-24.
R_MEASURED = 0.933          # at (n, N) = (129, 2): with two candidates the final rounding of m is most of it
R_TOL = 4.0 * R_MEASURED
WSUM_MEASURED = 0.260 * EPS
WSUM_RTOL = 4.0 * WSUM_MEASURED


def mean64(costs, key_cost, U, lam):
    """(m [n, 2], weight sum, s [n, 2]) in float64 for one problem: costs [N] float32, `key_cost` the cost in the problem's
    key, U [N, n, 2] float32, `lam` float32(lambda).  s is the scale of r above."""
    c = np.asarray(costs, dtype=T).astype(np.float64)
    U = np.asarray(U, dtype=T)
    N = c.shape[0]
    finite = np.isfinite(c)
    x = np.zeros(N)
    x[finite] = (c[finite] - float(T(key_cost))) / float(T(lam))
    w = np.where(finite, np.exp(-x), 0.0)
    keep = w != 0.0
    wsum = float(w[keep].sum())
    if wsum > 0.0:
        Uk, wk, xk = U[keep].astype(np.float64), w[keep], x[keep]
        m = np.tensordot(wk, Uk, axes=(0, 0)) / wsum
        s = np.tensordot(wk * (1.0 + xk), np.abs(Uk - m), axes=(0, 0)) / wsum
    else:
        U64 = U.astype(np.float64)
        m = U64.sum(axis=0) / N
        s = np.abs(U64 - m).sum(axis=0) / N
    return m, wsum, s


def error_r(got, m, s):
    """r per entry: |got - m| in units of 2^-24 (s + |m|)."""
    return np.abs(np.asarray(got, dtype=np.float64) - m) / (EPS * (s + np.abs(m)))


def keys_of(costs):
    """The packed key of every problem's minimum (ties to the lower index, non-finite costs last): what a rollout's
    finalize would leave for these costs [P, N]."""
    import acmpc_oracle as orc
    from acmpc_amd import _capi
    out = np.empty(costs.shape[0], dtype=np.int64)
    for p, c in enumerate(costs):
        best = orc.pick_best(c)[0]
        out[p] = _capi.pack_key(float(c[best]), best)
    return out


def _nonfinite(N):
    return np.where(np.arange(N) % 2 == 0, np.nan, np.inf).astype(T)


# ---- exact inputs ------------------------------------------------------------------------------------------------------
def exact_finite(P, N, seed=0):
    """mask [P, N]: the candidates that carry the finite cost - an irregular subset, never empty but in the LAST problem,
    where it is empty (the uniform fallback)."""
    rng = np.random.default_rng(7000 + 31 * N + seed)
    mask = rng.random((P, N)) < 0.6
    mask[:, rng.integers(0, N)] = True
    if N >= 2:
        mask[0, 0], mask[0, N - 1] = False, True      # the first candidate out, the last one in
    mask[P - 1] = False
    return mask


def exact_controls(P, N, n):
    """U [P, N, n, 2] float32: k 2^-8 with k an integer in (-2^15, 2^15) that changes with the problem, the candidate and
    the entry (its three strides are coprime to the modulus, a prime just below 2^16)."""
    p = np.arange(P, dtype=np.int64)[:, None, None]
    c = np.arange(N, dtype=np.int64)[None, :, None]
    e = np.arange(2 * n, dtype=np.int64)[None, None, :]
    k = (c * 7919 + e * 104729 + p * 15485863 + 12345) % 65521 - 32760
    return (k.astype(np.float64) * DYADIC).astype(T).reshape(P, N, n, 2)


def exact_problem(P, N, n, seed=0):
    """dict(costs [P, N], keys [P], U [P, N, n, 2], mean [P, n, 2] float32, weight_sum [P]): the exact inputs and what
    they must give, bit for bit.  Some zero-weight candidates of the problems before the last carry NaN controls."""
    mask = exact_finite(P, N, seed)
    costs = np.where(mask, T(EXACT_COST), _nonfinite(N)[None, :]).astype(T)
    U = exact_controls(P, N, n)
    k = np.rint(U.astype(np.float64) / DYADIC).astype(np.int64)      # the integers, exactly
    mean = np.empty((P, n, 2), dtype=T)
    wsum = np.empty(P)
    for p in range(P):
        count = int(mask[p].sum())
        rows = mask[p] if count else np.ones(N, dtype=bool)
        total = k[p][rows].sum(axis=0)              # integers: below 2^26, so every float64 partial sum is exact
        mean[p] = (total.astype(np.float64) * DYADIC / float(rows.sum())).astype(T)
        wsum[p] = float(count)
    U = U.copy()
    for p in range(P - 1):
        out = np.flatnonzero(~mask[p])
        U[p, out[::3]] = np.nan       # excluded with their weight of 0
    return dict(costs=costs, keys=keys_of(costs), U=U, mean=mean, weight_sum=wsum, mask=mask)


# ---- general inputs ----------------------------------------------------------------------------------------------------
def general_costs(P, N, seed):
    """costs [P, N] float32 = c_min + lambda x with x in [0, 6] crowded towards 6 (so that no candidate's share of the
    weight sum is negligible: see candidates_discriminate), NaN and +inf planted in the first, a middle and the last
    chunk of 1 024 as _synthetic_costs plants them, the last problem all non-finite."""
    rng = np.random.default_rng(8000 + seed)
    x = 6.0 * (1.0 - rng.random((P, N)) ** 32)
    x[np.arange(P), rng.integers(0, N, P)] = 0.0
    costs = (1.5 + LAMBDA * x).astype(T)
    chunks = (N + 1023) // 1024
    for chunk in sorted({0, chunks // 2, chunks - 1}):
        lo, hi = chunk * 1024, min(N, chunk * 1024 + 1024)
        if hi - lo >= 4:
            costs[:, lo + (hi - lo) // 3] = np.nan
            costs[:, hi - 1] = np.inf
            costs[0, lo] = np.inf
    if N >= 3:
        costs[0, N // 2] = np.nan
    costs[P - 1] = _nonfinite(N)
    return costs


def general_controls(P, N, n, seed, costs):
    """U [P, N, n, 2] float32: per entry a centre in [-0.3, 0.3], per candidate a step of +-(0.75 .. 1.25) away from it - three
    times that in the candidate's own entry, c mod 2n, so that every candidate stands out somewhere; NaN in the controls of
    every third non-finite candidate of the problems before the last."""
    rng = np.random.default_rng(9000 + seed)
    centre = rng.uniform(-0.3, 0.3, (P, 1, n, 2))
    step = rng.choice([-1.0, 1.0], (P, N, n, 2)) * rng.uniform(0.75, 1.25, (P, N, n, 2))
    own = np.arange(N) % (2 * n)
    step.reshape(P, N, 2 * n)[:, np.arange(N), own] *= 3.0
    U = (centre + step).astype(T)
    for p in range(P - 1):
        out = np.flatnonzero(~np.isfinite(costs[p]))
        U[p, out[::3]] = np.nan
    return U


def general_problem(P, N, n, seed=None):
    """dict(costs [P, N], keys [P], U [P, N, n, 2]) of the general inputs of a shape."""
    seed = 131 * n + N if seed is None else seed
    costs = general_costs(P, N, seed)
    return dict(costs=costs, keys=keys_of(costs), U=general_controls(P, N, n, seed, costs))


# ---- do the inputs discriminate? -----------------------------------------------------------------------------------------
def perturbed_means(costs, key_cost, U, lam, floor=1e-3):
    """What three mistakes would make of one problem's mean, from the reference's own input: for EVERY candidate whose
    weight is at least `floor` of the largest, the mean without it and the mean with it counted twice; and the mean with
    the weights paired with the candidates shifted by one.  Returns (m, s, removed [C, n, 2], doubled [C, n, 2], shifted
    [n, 2]); NaN controls (zero weight) count as 0."""
    m, wsum, s = mean64(costs, key_cost, U, lam)
    c = np.asarray(costs, dtype=T).astype(np.float64)
    finite = np.isfinite(c)
    w = np.zeros(c.shape[0])
    w[finite] = np.exp(-(c[finite] - float(T(key_cost))) / float(T(lam)))
    if not wsum > 0.0:          # the uniform fallback: every candidate with the same weight
        w, wsum = np.ones(c.shape[0]), float(c.shape[0])
    U64 = np.where(np.isnan(U), 0.0, U).astype(np.float64)
    heavy = np.flatnonzero(w >= floor * w.max())
    d = w[heavy, None, None] * (U64[heavy] - m)
    with np.errstate(divide="ignore", invalid="ignore"):       # (a lone candidate: nothing is left without it)
        removed = m - d / (wsum - w[heavy])[:, None, None]
    doubled = m + d / (wsum + w[heavy])[:, None, None]
    shifted = np.tensordot(w, np.roll(U64, -1, axis=0), axes=(0, 0)) / wsum
    return m, s, removed, doubled, shifted
