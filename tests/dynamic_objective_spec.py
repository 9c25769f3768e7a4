"""Mode D's objective restated in NumPy ("Mode D, progress and ceiling"): the rollout of
tests/dynamic_terms_spec.py - its lines, with the rate and slip parts through its own step_terms - plus a per-step speed
ceiling in V and a terminal progress reward in J.  Bit-identical to the TermsObjective kernels of
csrc/acmpc_dynamic_terms.hip.  A helper of the tests, not a test file.

    progress table, from the packed float32 rows (x, y, c = cos psi, s = sin psi), float64 in the order written, no FMA:
      S_0 = 0,  S_m = S_{m-1} + sqrt(dx dx + dy dy),  q_m = float32(S_m - (c_m (x_m - x_0) + s_m (y_m - y_0)))
    nwp = -float32(progress_weight)        cs, co = float32(scale), float32(offset)
    per step i, after the step's cost and after the rate and slip lines, with j that step's nearest waypoint:
      ceiling     cap = fma(cs, v_ref_j, co)        h = fmax(vx - cap, 0)        V = fma(h, h, V)
    finish, with j, X, Y the last control step's:
      progress    s = fma(s_j, Y, fma(c_j, X, q_j))         J = fma(nwp, s, J)   between J = stage + terminal and fma(w_bound, V, J)

The progress part is ON when progress_weight is not 0, the ceiling part when a ceiling is given; a part that is off executes
nothing.  J may be negative.

`setting()` swaps dynamic_spec.rollout_dynamic AND dynamic_terms_spec.rollout_dynamic for the duration of a `with` block:
enter it OUTERMOST, dynamic_terms_spec.setting() and dynamic_integration_spec.setting() inside it (in that order, as they
already compose).  The terms' block then ends in the loop below with its terms and previous control, the integration's block
swaps the step and the constants this loop calls through the dynamic_spec module, and the ensemble, sampled and softmin
restatements, which all end in dynamic_spec.rollout_dynamic, follow."""
from __future__ import annotations

import contextlib
from types import SimpleNamespace

import numpy as np

import dynamic_spec as ds
import dynamic_terms_spec as dts
from acmpc_oracle import fma32, wrap_spec

T = np.float32
NO_TERMS = ((0.0, 0.0), None, 0.0, None)


def progress_table(coef):
    """q [n] float32 of the packed rows `coef` [n, 8] (acmpc_get_progress_table)."""
    rows = np.asarray(coef, dtype=T)
    n = rows.shape[0]
    q = np.empty(n, dtype=T)
    x0, y0 = float(rows[0, 0]), float(rows[0, 1])
    S = 0.0
    for m in range(n):
        x, y, c, s = (float(v) for v in rows[m, :4])
        if m > 0:
            dx, dy = x - float(rows[m - 1, 0]), y - float(rows[m - 1, 1])
            S = S + float(np.sqrt(np.float64(dx * dx + dy * dy)))
        q[m] = T(S - (c * (x - x0) + s * (y - y0)))
    return q


def constants(progress_weight=0.0, speed_ceiling=None):
    """The kernel argument's objective members (csrc/acmpc_dynamic.h: TermsObjective), each rounded once.  A scalar ceiling
    is the scale with offset 0."""
    if speed_ceiling is not None and np.ndim(speed_ceiling) == 0:
        speed_ceiling = (float(speed_ceiling), 0.0)
    return SimpleNamespace(progress=float(progress_weight) != 0.0, ceiling=speed_ceiling is not None,
                           nwp=-T(float(progress_weight)),
                           cs=T(0.0) if speed_ceiling is None else T(float(speed_ceiling[0])),
                           co=T(0.0) if speed_ceiling is None else T(float(speed_ceiling[1])))


def rollout_dynamic(objective, terms, u_prev, x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase,
                    nn_window=None, return_states=False, trace=None):
    """dynamic_terms_spec.rollout_dynamic - the same lines - with the objective `objective` = (progress_weight,
    speed_ceiling).  With `trace` a dict, it receives E [N], the progress s [N] (where that part is on), the nearest index
    of the last step j [N], and `over` [N, n]: float32 vx - cap of every step (where the ceiling part is on)."""
    o = constants(*objective)
    c = dts.constants(dt, *terms)
    k = ds.derived_constants(vehicle)
    U = np.asarray(U, dtype=T)
    wp = np.asarray(wp, dtype=T)
    N, n, _ = U.shape
    Q, R, QN = (np.asarray(a, dtype=T) for a in (Q, R, QN))
    lo, hi = np.asarray(u_lo, dtype=T), np.asarray(u_hi, dtype=T)
    half, zero, wb, dtT = T(0.5), T(0.0), T(w_bound), T(dt)
    hQ, hR, hQN = half * Q, half * R, half * QN
    ox, oy = wp[0, 0], wp[0, 1]
    wx, wy = wp[:, 0] - ox, wp[:, 1] - oy
    key_a, key_b = T(-2.0) * wx, T(-2.0) * wy
    key_c = fma32(wy, wy, wx * wx)
    row_k = fma32(wp[:, 3], wx, -(wp[:, 2] * wy))
    row_ns = -wp[:, 3]
    delta_ref = ds.atan_spec(T(wheelbase) * wp[:, 5])
    q = progress_table(wp)
    x0 = np.asarray(x0, dtype=T)
    st = [np.full(N, x0[0] - ox, dtype=T), np.full(N, x0[1] - oy, dtype=T)] + [np.full(N, x0[m], dtype=T) for m in range(2, 6)]
    S0, S1, S2, S3, V, E = (np.zeros(N, dtype=T) for _ in range(6))
    ey = np.zeros(N, dtype=T)
    ep = np.zeros(N, dtype=T)
    j_prev = np.zeros(N, dtype=np.int64)
    rows = np.arange(N)
    pd = pp = None
    if c.rate and u_prev is not None:
        prev = np.asarray(u_prev, dtype=T)
        pd, pp = np.full(N, prev[0], dtype=T), np.full(N, prev[1], dtype=T)
    X_out = np.zeros((N, n + 1, 3), dtype=T) if return_states else None
    if return_states:
        X_out[:, 0] = np.stack([st[0] + ox, st[1] + oy, st[2]], axis=1)
    over = []
    for i in range(n):
        d, p = U[:, i, 0], U[:, i, 1]
        st = list(ds.dynamic_step(st, d, p, k, dtT))
        X, Y, psi, vx = st[0], st[1], st[2], st[3]
        if nn_window is None:
            w = np.broadcast_to(np.arange(n), (N, n))
        else:
            back, ahead = nn_window
            width = back + ahead + 1
            lo_w = np.maximum(np.minimum(j_prev - back, n - width), 0)
            hi_w = np.minimum(lo_w + width, n) - 1
            w = np.minimum(lo_w[:, None] + np.arange(width)[None, :], hi_w[:, None])
        best = np.full(N, np.inf, dtype=T)
        j = w[:, 0].copy()
        for b in range(0, w.shape[1], ds.SCAN_BLOCK):
            block = w[:, b:b + ds.SCAN_BLOCK]
            dd = fma32(Y[:, None], key_b[block], fma32(X[:, None], key_a[block], key_c[block]))
            first = np.argmin(np.where(np.isnan(dd), T(np.inf), dd), axis=1)
            dd = dd[rows, first]
            better = dd < best
            best = np.where(better, dd, best)
            j = np.where(better, block[rows, first], j)
        j_prev = j
        g = wp[j]
        with np.errstate(all="ignore"):
            ey = fma32(g[:, 2], Y, fma32(row_ns[j], X, row_k[j]))
            ep = wrap_spec(psi - g[:, 4], T)
            dv = vx - g[:, 6]
            dk = d - delta_ref[j]
            S0 = fma32(ey, ey, S0)
            S1 = fma32(ep, ep, S1)
            S2 = fma32(dv, dv, S2)
            S3 = fma32(dk, dk, S3)
            hd = d - np.fmin(np.fmax(d, lo[0]), hi[0])
            V = fma32(hd, hd, V)
            hp = p - np.fmin(np.fmax(p, lo[1]), hi[1])
            V = fma32(hp, hp, V)
            hc = np.fmax(np.abs(ey) - g[:, 7], zero)
            V = fma32(hc, hc, V)
        if i == 0 and pd is None:
            pd, pp = d, p
        E, V = dts.step_terms(c, k, st, d, p, pd, pp, E, V)
        pd, pp = d, p
        if o.ceiling:
            with np.errstate(all="ignore"):
                cap = fma32(o.cs, g[:, 6], o.co)
                excess = np.asarray(vx - cap, dtype=T)
                h = np.fmax(excess, zero)
                V = np.asarray(fma32(h, h, V), dtype=T)
            over.append(excess)
        if return_states:
            X_out[:, i + 1] = np.stack([X + ox, Y + oy, psi], axis=1)
    with np.errstate(all="ignore"):
        tN = T(n) * dtT
        J = hQ[0] * S0
        J = fma32(hQ[1], S1, J)
        J = fma32(hR[0], S2, J)
        J = fma32(hR[1], S3, J)
        if c.rate or c.slip:
            J = J + E
        s = (hQN[0] * ey) * ey
        s = fma32(hQN[1] * ep, ep, s)
        s = fma32(hQN[2] * tN, tN, s)
        J = J + s
        prog = None
        if o.progress:
            g = wp[j_prev]
            prog = np.asarray(fma32(g[:, 3], st[1], fma32(g[:, 2], st[0], q[j_prev])), dtype=T)
            J = fma32(o.nwp, prog, J)
        cost = fma32(wb, V, J)
    cost = np.asarray(cost, dtype=T)
    if trace is not None:
        trace["E"] = np.asarray(E, dtype=T)
        trace["j"] = j_prev.copy()
        if prog is not None:
            trace["s"] = prog
        if over:
            trace["over"] = np.stack(over, axis=1)
    return (cost, V, X_out) if return_states else (cost, V)


@contextlib.contextmanager
def setting(progress_weight=0.0, speed_ceiling=None):
    """Inside the block every dynamic_spec.rollout_dynamic - called directly or through the terms, integration, ensemble,
    sampled and softmin restatements entered INSIDE it - carries this objective.  Yields a handle whose `trace` may be set to
    a dict that then receives the last rollout's E, s, j and over."""
    if ds.rollout_dynamic.__module__ != ds.__name__:
        raise RuntimeError("dynamic_objective_spec.setting() is entered outermost: before the terms' and the integration's")
    handle = SimpleNamespace(objective=(progress_weight, speed_ceiling), trace=None)
    saved = ds.rollout_dynamic, dts.rollout_dynamic

    def plain(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, **kwargs):
        return with_terms(NO_TERMS, None, x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, **kwargs)

    def with_terms(terms, u_prev, x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, **kwargs):
        if handle.trace is not None:
            kwargs["trace"] = handle.trace
        return rollout_dynamic(handle.objective, terms, u_prev, x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt,
                               wheelbase, **kwargs)

    ds.rollout_dynamic, dts.rollout_dynamic = plain, with_terms
    try:
        yield handle
    finally:
        ds.rollout_dynamic, dts.rollout_dynamic = saved


def spec_costs(orc, dp, coef, vehicle, objective, **kwargs):
    """dynamic_spec.spec_costs with the objective `objective` = dict(progress_weight=, speed_ceiling=)."""
    with setting(**objective):
        return ds.spec_costs(orc, dp, coef, vehicle, **kwargs)
