"""Mode D's rate and slip terms restated in NumPy ("Mode D", "Rate and slip terms"): the rollout of
tests/dynamic_spec.py with, per control step and after that step's cost, the squared control rates and the squared rear
slip ratio added to a third cost sum E and their excesses over the limits added to V.  Built from dynamic_spec's pieces
and bit-identical to the kernels of csrc/acmpc_dynamic_terms.hip.  A helper of the tests, not a test file.

    inv_dt = float32(1 / dt)           hwd, hwp, hws = 0.5f * float32(weight)         rd_max, rp_max, b_max = float32(limit)
    per step i, on the state (vx, vy, r) that step's cost saw, (pd, pp) = the controls of step i - 1 - at step 0 u_prev,
    or without one (delta_0, pedal_0) itself:
      rate part   rd = (delta - pd) * inv_dt        rp = (pedal - pp) * inv_dt
                  E = fma(hwd * rd, rd, E)          E = fma(hwp * rp, rp, E)
                  V = fma(h, h, V), h = fmax(|rd| - rd_max, 0), then the same for rp           (after the corridor hinge)
      slip part   b = (r * lr - vy) / (vx + 1e-3f)  E = fma(hws * b, b, E)     V = fma(h, h, V), h = fmax(|b| - b_max, 0)
    finish: stage = stage + E after the four weighted sums, then J = stage + terminal and fma(w_bound, V, J) as ever.

A part is ON when one of its weights is not 0 or one of its limits finite, and a part that is off executes nothing.

`setting()` swaps dynamic_spec.rollout_dynamic for the duration of a `with` block.  The loop below calls the step and the
vehicle's constants through the dynamic_spec module, so dynamic_integration_spec.setting() entered INSIDE this block
(it wraps whatever rollout_dynamic it finds) composes with it, and so do the ensemble, sampled and softmin restatements,
which all end in dynamic_spec.rollout_dynamic."""
from __future__ import annotations

import contextlib
from types import SimpleNamespace

import numpy as np

import dynamic_spec as ds
from acmpc_oracle import fma32, wrap_spec

T = np.float32
INF = float("inf")


def constants(dt, rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=None):
    """The kernel argument (csrc/acmpc_dynamic.h: Terms): every float derived in float64 and rounded once."""
    limits = [INF, INF] if rate_max is None else [INF if v is None else float(v) for v in rate_max]
    b_max = INF if slip_max is None else float(slip_max)
    w = [float(v) for v in rate_weight]
    rate = w[0] != 0.0 or w[1] != 0.0 or np.isfinite(limits[0]) or np.isfinite(limits[1])
    slip = float(slip_weight) != 0.0 or np.isfinite(b_max)
    return SimpleNamespace(rate=bool(rate), slip=bool(slip), inv_dt=T(1.0 / float(dt)), hwd=T(0.5) * T(w[0]),
                           hwp=T(0.5) * T(w[1]), hws=T(0.5) * T(float(slip_weight)), rd_max=T(limits[0]),
                           rp_max=T(limits[1]), b_max=T(b_max))


def step_terms(c, k, state, d, p, pd, pp, E, V):
    """The terms of one control step (csrc/acmpc_dynamic.h: dynamic_terms): the new (E, V)."""
    zero = T(0.0)
    with np.errstate(all="ignore"):
        if c.rate:
            rd = (d - pd) * c.inv_dt
            rp = (p - pp) * c.inv_dt
            E = fma32(c.hwd * rd, rd, E)
            E = fma32(c.hwp * rp, rp, E)
            h = np.fmax(np.abs(rd) - c.rd_max, zero)
            V = fma32(h, h, V)
            h = np.fmax(np.abs(rp) - c.rp_max, zero)
            V = fma32(h, h, V)
        if c.slip:
            vx, vy, r = state[3], state[4], state[5]
            b = (r * k["lr"] - vy) / (vx + T(ds.VX_EPS))
            E = fma32(c.hws * b, b, E)
            h = np.fmax(np.abs(b) - c.b_max, zero)
            V = fma32(h, h, V)
    return np.asarray(E, dtype=T), np.asarray(V, dtype=T)


def rollout_dynamic(terms, u_prev, x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, nn_window=None,
                    return_states=False, trace=None):
    """dynamic_spec.rollout_dynamic - the same lines - with the terms `terms` = (rate_weight, rate_max, slip_weight,
    slip_max) and the previous control `u_prev` = (delta, pedal) or None.  With `trace` a dict, it also receives E [N]."""
    c = constants(dt, *terms)
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
    x0 = np.asarray(x0, dtype=T)
    st = [np.full(N, x0[0] - ox, dtype=T), np.full(N, x0[1] - oy, dtype=T)] + [np.full(N, x0[q], dtype=T) for q in range(2, 6)]
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
            pd, pp = d, p   # (no previous control: step 0's own, an increment of +0 for a finite control)
        E, V = step_terms(c, k, st, d, p, pd, pp, E, V)
        pd, pp = d, p
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
        cost = fma32(wb, V, J)
    cost = np.asarray(cost, dtype=T)
    if trace is not None:
        trace["E"] = np.asarray(E, dtype=T)
    return (cost, V, X_out) if return_states else (cost, V)


@contextlib.contextmanager
def setting(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=None, u_prev=None):
    """Inside the block every dynamic_spec.rollout_dynamic - called directly or through the ensemble, sampled, softmin and
    integration restatements - carries these terms.  Yields a handle whose `u_prev` ((delta, pedal) or None) may be
    changed between calls: one problem's previous control at a time."""
    handle = SimpleNamespace(terms=(tuple(rate_weight), rate_max, slip_weight, slip_max), u_prev=u_prev, trace=None)
    saved = ds.rollout_dynamic

    def with_terms(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, **kwargs):
        if handle.trace is not None:
            kwargs.setdefault("trace", handle.trace)
        return rollout_dynamic(handle.terms, handle.u_prev, x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt,
                               wheelbase, **kwargs)

    ds.rollout_dynamic = with_terms
    try:
        yield handle
    finally:
        ds.rollout_dynamic = saved


def spec_costs(orc, dp, coef, vehicle, terms, u_prev=None, **kwargs):
    """dynamic_spec.spec_costs with the terms `terms` = dict(rate_weight=, rate_max=, slip_weight=, slip_max=)."""
    with setting(u_prev=u_prev, **terms):
        return ds.spec_costs(orc, dp, coef, vehicle, **kwargs)
