"""Mode D's obstacles restated in NumPy ("Mode D, obstacles"): the rollout of
tests/dynamic_objective_spec.py - its lines - plus, per control step and after the ceiling's line, each disc's penetration
depth in V and its depth into the margin in E.  Bit-identical to the WithObstacles kernels of
csrc/acmpc_dynamic_obstacles.hip.  A helper of the tests, not a test file.

    hwo = 0.5f * float32(weight)        mg = float32(margin)        (x_0, y_0) = the first packed row's x, y
    per step i, after the step's cost and after the rate, slip and ceiling lines, for k = 0 .. K - 1 in that order:
      ox = o_x[i][k] - x_0        oy = o_y[i][k] - y_0
      dx = X - ox                 dy = Y - oy                 d = sqrt(fma(dy, dy, dx * dx))
      hard        h = fmax(R_k - d, 0)                V = fma(h, h, V)
      soft        g = fmax((R_k + mg) - d, 0)         E = fma(hwo * g, g, E)
    finish: stage = stage + E when the rate, the slip OR the soft part is on.

The hard part is ON while obstacles are given (K > 0), the soft part while they are given and float32(weight) is not 0; a
part that is off executes nothing.

`setting()` swaps dynamic_objective_spec.rollout_dynamic - the function every composed restatement ends in once
dynamic_objective_spec.setting() is entered (tests/dynamic_fuzz_cases.restatement always enters it) - for the duration of a
`with` block.  It may be entered anywhere round that block; `restatement()` below enters it outermost.  The step and the
constants are called through the dynamic_spec module, so the integration's, the coupling's and the load transfer's blocks
compose with it as they do with the objective's."""
from __future__ import annotations

import contextlib
from types import SimpleNamespace

import numpy as np

import dynamic_objective_spec as dos
import dynamic_spec as ds
import dynamic_terms_spec as dts
from acmpc_oracle import fma32, wrap_spec

T = np.float32


def constants(weight=0.0, margin=0.0):
    """The kernel argument's clearance members (csrc/acmpc_dynamic.h: WithObstacles), each rounded once."""
    return SimpleNamespace(soft=bool(T(float(weight)) != T(0.0)), hwo=T(0.5) * T(float(weight)), mg=T(float(margin)))


def step_obstacles(o, soft, row, radii, x_0, y_0, X, Y, E, V):
    """The discs' lines of one control step (csrc/acmpc_dynamic.h: the second dynamic_terms): the new (E, V).  row [K, 2],
    radii [K] float32."""
    zero = T(0.0)
    with np.errstate(all="ignore"):
        for k in range(row.shape[0]):
            ox, oy = T(row[k, 0] - x_0), T(row[k, 1] - y_0)
            dx, dy = X - ox, Y - oy
            d = np.sqrt(np.asarray(fma32(dy, dy, dx * dx), dtype=T))
            h = np.fmax(radii[k] - d, zero)
            V = np.asarray(fma32(h, h, V), dtype=T)
            if soft:
                g = np.fmax(T(radii[k] + o.mg) - d, zero)
                E = np.asarray(fma32(o.hwo * g, g, E), dtype=T)
    return E, V


def rollout_dynamic(obstacles, objective, terms, u_prev, x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase,
                    nn_window=None, return_states=False, trace=None):
    """dynamic_objective_spec.rollout_dynamic - the same lines - with `obstacles` = (positions [n, K, 2] or None, radii
    [K], weight, margin).  With `trace` a dict, it receives E [N] and `E_added`: whether stage = stage + E was
    executed."""
    pos, radii, weight, margin = obstacles
    K = 0 if pos is None else int(np.asarray(pos).shape[1])
    ob = constants(weight, margin)
    soft = ob.soft and K > 0
    if K > 0:
        pos = np.asarray(pos, dtype=T)
        radii = np.asarray(radii, dtype=T)
    o = dos.constants(*objective)
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
    q = dos.progress_table(wp)
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
                h = np.fmax(np.asarray(vx - cap, dtype=T), zero)
                V = np.asarray(fma32(h, h, V), dtype=T)
        if K > 0:
            E, V = step_obstacles(ob, soft, pos[i], radii, ox, oy, X, Y, E, V)
        if return_states:
            X_out[:, i + 1] = np.stack([X + ox, Y + oy, psi], axis=1)
    with np.errstate(all="ignore"):
        tN = T(n) * dtT
        J = hQ[0] * S0
        J = fma32(hQ[1], S1, J)
        J = fma32(hR[0], S2, J)
        J = fma32(hR[1], S3, J)
        added = bool(c.rate or c.slip or soft)
        if added:
            J = J + E
        s = (hQN[0] * ey) * ey
        s = fma32(hQN[1] * ep, ep, s)
        s = fma32(hQN[2] * tN, tN, s)
        J = J + s
        if o.progress:
            g = wp[j_prev]
            prog = np.asarray(fma32(g[:, 3], st[1], fma32(g[:, 2], st[0], q[j_prev])), dtype=T)
            J = fma32(o.nwp, prog, J)
        cost = fma32(wb, V, J)
    cost = np.asarray(cost, dtype=T)
    V = np.asarray(V, dtype=T)
    if trace is not None:
        trace["E"] = np.asarray(E, dtype=T)
        trace["E_added"] = added
    return (cost, V, X_out) if return_states else (cost, V)


@contextlib.contextmanager
def setting(positions=None, radii=None, weight=0.0, margin=0.0):
    """Inside the block every restatement that ends in dynamic_objective_spec.rollout_dynamic carries these obstacles.
    Yields a handle whose `obstacles` = (positions [n, K, 2] or None, radii [K], weight, margin) may be changed between
    calls - one problem's discs at a time - and whose `trace` may be set to a dict."""
    handle = SimpleNamespace(obstacles=(positions, radii, weight, margin), trace=None)
    saved = dos.rollout_dynamic

    def with_obstacles(objective, terms, u_prev, *args, **kwargs):
        if handle.trace is not None:
            kwargs["trace"] = handle.trace
        else:
            kwargs.pop("trace", None)
        return rollout_dynamic(handle.obstacles, objective, terms, u_prev, *args, **kwargs)

    dos.rollout_dynamic = with_obstacles
    try:
        yield handle
    finally:
        dos.rollout_dynamic = saved


@contextlib.contextmanager
def restatement(c, u_prev=None, obstacles=None, clearance=(0.0, 0.0), without=()):
    """tests/dynamic_fuzz_cases.restatement(c, u_prev, without) with ONE problem's obstacles = (positions [n, K, 2], radii
    [K]) or None and the handle's clearance = (weight, margin)."""
    import dynamic_fuzz_cases as dfc
    pos, radii = (None, None) if obstacles is None else obstacles
    with setting(pos, radii, *clearance) as handle:
        with dfc.restatement(c, u_prev, without):
            yield handle


def make_obstacles(dp, n, K, seed, nan="none"):
    """(positions [n, K, 2], radii [K]) float32 for problem `dp` (dynamic_spec.make_dynamic_problem): K discs round where
    the start state's own velocity carries it - disc k starts (a_k ahead, b_k to the left) of the start and drifts against
    it - so that some candidates of a spread set enter a disc, some only its margin and some neither.  `nan`: "none";
    "some": a few (step, disc) entries are NaN or infinite (discs that do not exist at those steps); "all": every entry is
    NaN."""
    rng = np.random.default_rng([4242, int(seed), int(K)])
    x0 = np.asarray(dp["x0"], dtype=np.float64)
    dt = float(dp["kw"]["dt"])
    heading = np.array([np.cos(x0[2]), np.sin(x0[2])])
    left = np.array([-heading[1], heading[0]])
    t = (np.arange(n) + 1.0) * dt
    radii = rng.uniform(0.3, 2.5, K).astype(T)
    if K > 1:
        radii[K - 1] = T(0.0)                       # (a disc of radius 0 never violates; its margin still costs)
    ahead = rng.uniform(-0.5, 0.5, K)
    aside = rng.choice([-1.0, 1.0], K) * (radii + rng.uniform(-0.3, 0.3, K))   # the rim runs through the bundle of candidates
    drift = rng.uniform(-2.0, 2.0, (K, 2))
    speed = float(x0[3])
    pos = (x0[None, None, :2] + (speed * t)[:, None, None] * heading[None, None, :]
           + ahead[None, :, None] * heading[None, None, :] + aside[None, :, None] * left[None, None, :]
           + t[:, None, None] * drift[None, :, :]).astype(T)
    if nan == "all":
        pos[:] = np.nan
    elif nan == "some":
        pos[rng.integers(0, n), rng.integers(0, K), 0] = np.nan
        pos[rng.integers(0, n), rng.integers(0, K), 1] = np.inf
        pos[n - 1, 0] = np.nan
    return pos, radii
