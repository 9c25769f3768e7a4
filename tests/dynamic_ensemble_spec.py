"""Mode D's ensemble restated in NumPy ("Mode D", "Ensembles"): every candidate rolled under each
of K vehicles by tests/dynamic_spec.rollout_dynamic, then the fixed-order combine - MEAN: J = omega_0 c_0, then
J = fma32(omega_k, c_k, J) in k order; MAX: the largest c_k, NaN if any is NaN - the violation max_k V_k (NaN if any is
NaN), and the states of vehicle 0.  A helper of the tests, not a test file."""
from __future__ import annotations

import numpy as np

import dynamic_spec as ds
from acmpc_oracle import fma32

T = np.float32
MEAN, MAX = "mean", "max"


def omegas(K, weights=None):
    """The float32 weights of the combine: w_k / sum_j w_j in float64 (the sum in k order), each rounded once; equal
    weights float32(1 / K) when `weights` is None."""
    if weights is None:
        return np.full(K, T(1.0 / K), dtype=T)
    w = [float(x) for x in weights]
    total = 0.0
    for x in w:
        total += x
    return np.array([T(x / total) for x in w], dtype=T)


def nan_max(a, b):
    """b where b > a or b is NaN, else a: the largest, NaN if either is NaN (a NaN a stays)."""
    return np.where((b > a) | np.isnan(b), b, a).astype(T)


def combine(costs, violations, reduce=MEAN, weights=None):
    """The ensemble's (J, V) from per-vehicle costs [K][N] and violations [K][N], in k order."""
    costs = [np.asarray(c, dtype=T) for c in costs]
    violations = [np.asarray(v, dtype=T) for v in violations]
    K = len(costs)
    om = omegas(K, weights)
    with np.errstate(all="ignore"):
        J = (om[0] * costs[0]).astype(T) if reduce == MEAN else costs[0].copy()
        V = violations[0].copy()
        for k in range(1, K):
            J = fma32(om[k], costs[k], J) if reduce == MEAN else nan_max(J, costs[k])
            V = nan_max(V, violations[k])
    return np.asarray(J, dtype=T), np.asarray(V, dtype=T)


def rollout_ensemble(x0, wp, U, vehicles, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, reduce=MEAN, weights=None,
                     nn_window=None, return_states=False, **kwargs):
    """The ensemble's cost and violation of every candidate (and vehicle 0's states): rollout_dynamic once per vehicle
    block of `vehicles` - with `kwargs`: its settings, u_prev and obstacles - then combine()."""
    per = [ds.rollout_dynamic(x0, wp, U, v, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, nn_window=nn_window,
                              return_states=return_states and k == 0, **kwargs) for k, v in enumerate(vehicles)]
    J, V = combine([r[0] for r in per], [r[1] for r in per], reduce, weights)
    return (J, V, per[0][2]) if return_states else (J, V)


def spec_ensemble(orc, dp, coef, vehicles, reduce=MEAN, weights=None, nn_window=None, U=None, return_states=False, **kwargs):
    """The ensemble specification of problem `dp` (dynamic_spec.make_dynamic_problem) on the packed table `coef`; `kwargs`:
    rollout_dynamic's settings, u_prev and obstacles."""
    kw = dp["kw"]
    return rollout_ensemble(dp["x0"], coef, dp["U"] if U is None else U, vehicles, kw["step_cost"], kw["r_term"],
                            kw["final_cost"], kw["u_min"], kw["u_max"], kw["w_bound"], kw["dt"], kw["wheelbase"],
                            reduce=reduce, weights=weights, nn_window=nn_window, return_states=return_states, **kwargs)
