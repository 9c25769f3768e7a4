"""Mode D's rollout under a surface table (acmpc_set_surface, DESIGN.md section 2 "Mode D, surface") restated in float32 NumPy:
tests/dynamic_spec.py's rollout with the two peak factors of the step replaced, per control step and per candidate, by

    Pf_s = Pf mu_f[j_{i-1}]      Pr_s = Pr mu_r[j_{i-1}]          one float32 multiply each, j_{-1} = 0

where j_{i-1} is the nearest waypoint the step before's cost used (the windowed search starts from the same index).  Composed
from dynamic_spec's own `constants`, `control_step`, `step_terms`, `step_obstacles` and `progress_table`; the search and the cost
lines are its lines.  The step under a table is the top-tier step, whatever the settings: `surface_settings` gives a tier that is
off its neutral value (downforce (0, 0) with a finite v_sat; `constants` then gives c_h = w_max = 0 and rho = +inf).  With no
table nothing is replaced and nothing promoted: the function is dynamic_spec.rollout_dynamic bit for bit.  A helper of the tests,
not a test file."""
from __future__ import annotations

import numpy as np

import dynamic_ensemble_spec as es
import dynamic_spec as ds
from acmpc_oracle import fma32, wrap_spec
from dynamic_spec import Settings, T


def surface_settings(settings):
    """The settings of the step a handle with a table takes: the downforce's tier, with k_f = k_r = 0 while it is off."""
    return settings if settings.downforce is not None else settings.replace(downforce=(0.0, 0.0, ds.V_SAT))


def rollout_surface(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, nn_window=None, return_states=False,
                    trace=None, settings=Settings(), u_prev=None, obstacles=None, surface=None):
    """dynamic_spec.rollout_dynamic with `surface` [n, 2] float32 = (mu_f, mu_r) per waypoint, or None.  The same returns and
    the same `trace` outputs (states, terms, totals, j, e_y, E, E_added, s, over)."""
    c = ds.constants(vehicle, settings if surface is None else surface_settings(settings), dt)
    mu = None if surface is None else np.ascontiguousarray(surface, dtype=T)
    base_Pf, base_Pr = c.k["Pf"], c.k["Pr"]
    pos, radii = (None, None) if obstacles is None else obstacles
    K = 0 if pos is None else int(np.asarray(pos).shape[1])
    soft = c.soft and K > 0
    if K > 0:
        pos, radii = np.asarray(pos, dtype=T), np.asarray(radii, dtype=T)
    U = np.asarray(U, dtype=T)
    wp = np.asarray(wp, dtype=T)
    N, n, _ = U.shape
    assert mu is None or mu.shape == (n, 2)
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
    row = None
    if trace is not None:
        states = np.zeros((N, n + 1, 6), dtype=T)
        states[:, 0] = np.stack([st[0] + ox, st[1] + oy] + st[2:], axis=1)
        terms = np.zeros((N, n, ds.TERM_FLOATS), dtype=T)
        seen = dict(e_y=[], j=[], over=[])
    for i in range(n):
        d, p = U[:, i, 0], U[:, i, 1]
        if mu is not None:   # the scales of the waypoint the candidate was at one control step before
            c.k["Pf"] = np.asarray(base_Pf * mu[j_prev, 0], dtype=T)
            c.k["Pr"] = np.asarray(base_Pr * mu[j_prev, 1], dtype=T)
        st = list(ds.control_step(st, d, p, c))
        X, Y, psi, vx = st[0], st[1], st[2], st[3]
        # dynamic_spec's search: the first minimum of the key under `<` from +inf, in waypoint order
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
        if trace is not None:
            row = terms[:, i]
            row[:, ds.J], row[:, ds.EY], row[:, ds.EPSI], row[:, ds.DV], row[:, ds.DK] = j.astype(T), ey, ep, dv, dk
            row[:, ds.BOX], row[:, ds.BOX + 1], row[:, ds.CORRIDOR] = hd, hp, hc
            seen["e_y"].append(ey.copy())
            seen["j"].append(j.copy())
        if c.rate or c.slip:
            if i == 0 and pd is None:
                pd, pp = d, p
            E, V = ds.step_terms(c, st, d, p, pd, pp, E, V, row)
            pd, pp = d, p
        if c.ceiling:
            with np.errstate(all="ignore"):
                cap = fma32(c.cs, g[:, 6], c.co)
                excess = np.asarray(vx - cap, dtype=T)
                h = np.fmax(excess, zero)
                V = np.asarray(fma32(h, h, V), dtype=T)
            if trace is not None:
                row[:, ds.CEILING] = h
                seen["over"].append(excess)
        if K > 0:
            E, V = ds.step_obstacles(c, soft, pos[i], radii, ox, oy, X, Y, E, V, row)
        if trace is not None:
            row[:, ds.V_SLOT], row[:, ds.E_SLOT] = V, E
            states[:, i + 1] = np.stack([X + ox, Y + oy] + st[2:], axis=1)
        if return_states:
            X_out[:, i + 1] = np.stack([X + ox, Y + oy, psi], axis=1)
    with np.errstate(all="ignore"):
        tN = T(n) * dtT
        Jc = hQ[0] * S0
        Jc = fma32(hQ[1], S1, Jc)
        Jc = fma32(hR[0], S2, Jc)
        Jc = fma32(hR[1], S3, Jc)
        added = bool(c.rate or c.slip or soft)
        if added:
            Jc = Jc + E
        s = (hQN[0] * ey) * ey
        s = fma32(hQN[1] * ep, ep, s)
        s = fma32(hQN[2] * tN, tN, s)
        Jc = Jc + s
        if c.progress:
            q = ds.progress_table(wp)
            g = wp[j_prev]
            prog = np.asarray(fma32(g[:, 3], st[1], fma32(g[:, 2], st[0], q[j_prev])), dtype=T)
            Jc = fma32(c.nwp, prog, Jc)
        cost = fma32(wb, V, Jc)
    cost = np.asarray(cost, dtype=T)
    V = np.asarray(V, dtype=T)
    if trace is not None:
        trace.update(e_y=np.stack(seen["e_y"], axis=1), j=np.stack(seen["j"], axis=1), E=np.asarray(E, dtype=T), E_added=added,
                     states=states, terms=terms, totals=np.stack([cost, V], axis=1))
        if c.progress:
            trace["s"] = prog
        if c.ceiling:
            trace["over"] = np.stack(seen["over"], axis=1)
    return (cost, V, X_out) if return_states else (cost, V)


def spec_costs(orc, dp, coef, vehicle, nn_window=None, U=None, return_states=False, **kwargs):
    """dynamic_spec.spec_costs with `surface=` among the keywords."""
    kw = dp["kw"]
    return rollout_surface(dp["x0"], coef, dp["U"] if U is None else U, vehicle, kw["step_cost"], kw["r_term"],
                           kw["final_cost"], kw["u_min"], kw["u_max"], kw["w_bound"], kw["dt"], kw["wheelbase"],
                           nn_window=nn_window, return_states=return_states, **kwargs)


def spec_ensemble(orc, dp, coef, vehicles, reduce=es.MEAN, weights=None, nn_window=None, U=None, return_states=False, **kwargs):
    """The ensemble under a table: every vehicle block rolled on its own trajectory's j with its own peaks, the table shared;
    then dynamic_ensemble_spec.combine.  States: vehicle 0's."""
    per = [spec_costs(orc, dp, coef, v, nn_window=nn_window, U=U, return_states=return_states and k == 0, **kwargs)
           for k, v in enumerate(vehicles)]
    Jc, V = es.combine([r[0] for r in per], [r[1] for r in per], reduce, weights)
    return (Jc, V, per[0][2]) if return_states else (Jc, V)


def trace_plans(dp, coef, U, vehicles, settings=Settings(), nn_window=None, u_prev=None, obstacles=None, surface=None):
    """dynamic_spec.trace_plans under a table: dict(states [M, K, n + 1, 6], totals [M, K, 2], terms [M, K, n, 22])."""
    per = []
    for block in vehicles:
        per.append({})
        spec_costs(None, dp, coef, block, nn_window=nn_window, U=U, settings=settings, u_prev=u_prev, obstacles=obstacles,
                   surface=surface, trace=per[-1])
    return {name: np.stack([t[name] for t in per], axis=1) for name in ("states", "totals", "terms")}


def make_dense_problem(orc, H, N, seed, vx0=None):
    """dynamic_spec.make_dynamic_problem on test_support.local_path(H, seed, length=1.5 * (H - 1)): waypoints 1.5 m apart, so
    that a plan of a dozen steps at the path's speed crosses several of them."""
    import test_support
    local_path = test_support.local_path
    test_support.local_path = lambda h, s: local_path(h, s, length=1.5 * (H - 1))
    try:
        return ds.make_dynamic_problem(orc, "monza", H, N, seed, vx0=vx0)
    finally:
        test_support.local_path = local_path


def random_table(n, seed, lo=0.4, hi=1.0):
    """[n, 2] float32 drawn uniformly from [lo, hi]."""
    return np.random.default_rng([9100, int(seed)]).uniform(lo, hi, (n, 2)).astype(T)
