"""Mode D's rollout under a road table (acmpc_set_road, DESIGN.md section 2 "Mode D, road") restated in float32 NumPy.

The table is road [n, 3] float32 = (a_x, a_y, n_z) per waypoint: gravity's acceleration along the body's forward and left axes
and the factor on the normal load.  With j_{i-1} the nearest waypoint the step before's cost used (j_{-1} = 0, the surface
table's lag), at the top of control step i, once, in float32 with nothing fused:

    Pf_r = Pf_s n_z[j_{i-1}]      Pr_r = Pr_s n_z[j_{i-1}]          Pf_s, Pr_s: the peaks under the surface table, else the vehicle's

and in every Euler sub-step of that control step, after xd3 and xd4 are formed and before the multiply by the step:

    xd3 = xd3 + a_x[j_{i-1}]      xd4 = xd4 + a_y[j_{i-1}]

`road_step` restates dynamic_spec.dynamic_step with those two lines (its peaks come in through c.k, as there).  The rest is
composed, unedited: dynamic_surface_spec.rollout_surface makes exactly one call of dynamic_spec.control_step per control step,
after it has put the surface's peaks into c.k, and control_step calls dynamic_spec.dynamic_step per sub-step - so for the length of
one rollout `control_step` is replaced by `on_road`, which multiplies n_z into the peaks that are there, lets the real control
step run on `road_step` with the row's accelerations, and then finds the nearest waypoint of the state it returns with the
search's own lines (restated below, and checked against the j that rollout_surface recorded, in every call).  The actuator lag
composes on top: dynamic_actuator_spec.rollout_actuator replaces whatever control_step it finds, here `on_road`.  The step under
a table is the top-tier step (dynamic_surface_spec.surface_settings).  With no table the function is rollout_actuator bit for
bit.  A helper of the tests, not a test file."""
from __future__ import annotations

import numpy as np

import dynamic_actuator_spec as das
import dynamic_ensemble_spec as es
import dynamic_spec as ds
import dynamic_surface_spec as dss
from acmpc_oracle import fma32, sincos_spec
from dynamic_spec import Settings, T, VX_EPS, aero_peaks, atan_spec, couple_axle, loaded_peaks, pacejka


def road_step(state, delta, pedal, c, a_x, a_y, h=None):
    """dynamic_spec.dynamic_step with gravity's two accelerations: `a_x`, `a_y` float32, scalars or one per element."""
    X, Y, yaw, vx, vy, r = (np.asarray(s, dtype=T) for s in state)
    delta = np.asarray(delta, dtype=T)
    pedal = np.asarray(pedal, dtype=T)
    a_x, a_y = np.asarray(a_x, dtype=T), np.asarray(a_y, dtype=T)
    k = c.k
    dt = T(c.h if h is None else h)
    with np.errstate(all="ignore"):
        den = vx + T(VX_EPS)
        qf = (r * k["lf"] + vy) / den
        qr = (r * k["lr"] - vy) / den
        a_f = delta - atan_spec(qf)
        a_r = atan_spec(qr)
        if c.peaks == "static":
            F_fy = pacejka(a_f, k["Bf"], k["Cf"], k["Ef"], k["Pf"])
            F_ry = pacejka(a_r, k["Br"], k["Cr"], k["Er"], k["Pr"])
        vx2 = vx * vx
        F_fric = (k["fric0"] - k["Cfric2"] * vx) - k["Cfric3"] * vx2
        brake = (k["Cb1"] - k["Cb2"] * vx) - k["Cb3"] * vx2
        motor = (k["Cm1"] - k["Cm2"] * vx) - k["Cm3"] * vx2
        p_neg = np.fmin(pedal, T(0.0))
        p_pos = np.fmax(pedal, T(0.0))
        F_rx = (brake * k["bias_rear"]) * p_neg + motor * p_pos
        F_fx = (brake * k["bias_front"]) * p_neg
        if c.peaks == "static":
            if c.rho is not None:
                F_fx, F_fy = couple_axle(F_fx, F_fy, c.rho[0], k["Pf"])
                F_rx, F_ry = couple_axle(F_rx, F_ry, c.rho[1], k["Pr"])
        else:
            if c.peaks == "loaded":
                Pf, Pr = loaded_peaks(F_fx, F_rx, c.rho[0], c.rho[1], k)[:2]
            else:
                Pf, Pr = aero_peaks(vx, F_fx, F_rx, c.rho[0], c.rho[1], k)[:2]
            F_fy = pacejka(a_f, k["Bf"], k["Cf"], k["Ef"], Pf)
            F_ry = pacejka(a_r, k["Br"], k["Cr"], k["Er"], Pr)
            F_fx, F_fy = couple_axle(F_fx, F_fy, c.rho[0], Pf)
            F_rx, F_ry = couple_axle(F_rx, F_ry, c.rho[1], Pr)
        sd, cd = sincos_spec(delta, T)
        sy, cy = sincos_spec(yaw, T)
        xd0 = vx * cy - vy * sy
        xd1 = vx * sy + vy * cy
        xd3 = k["inv_mass"] * ((((F_rx + F_fx) + F_fric) - F_fy * sd) + (k["mass"] * vy) * r)
        xd4 = k["inv_mass"] * ((F_ry + F_fy * cd) - (k["mass"] * vx) * r)
        xd3 = np.asarray(xd3, dtype=T) + a_x          # the road: one float32 add each, before the * dt
        xd4 = np.asarray(xd4, dtype=T) + a_y
        xd5 = k["inv_Iz"] * ((F_fy * k["lf"]) * cd - F_ry * k["lr"])
        Xn = X + xd0 * dt
        Yn = Y + xd1 * dt
        yawn = yaw + r * dt
        vxn = np.fmax(vx + xd3 * dt, T(0.0))
        vyn = vy + xd4 * dt
        rn = r + xd5 * dt
    return tuple(np.asarray(a, dtype=T) for a in (Xn, Yn, yawn, vxn, vyn, rn))


def nearest(X, Y, wp, j_prev, nn_window):
    """The nearest waypoint of every candidate's (X, Y) (the path's own frame), with rollout_surface's lines: the first minimum
    of the key under `<` from +inf, in waypoint order, over all waypoints or the window from j_prev."""
    wp = np.asarray(wp, dtype=T)
    n, N = wp.shape[0], X.shape[0]
    wx, wy = wp[:, 0] - wp[0, 0], wp[:, 1] - wp[0, 1]
    key_a, key_b = T(-2.0) * wx, T(-2.0) * wy
    key_c = fma32(wy, wy, wx * wx)
    rows = np.arange(N)
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
    return j


def rollout_road(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, settings=Settings(), surface=None,
                 actuator=None, a0=None, road=None, nn_window=None, trace=None, **kwargs):
    """dynamic_actuator_spec.rollout_actuator with `road` [n, 3] float32 = (a_x, a_y, n_z) per waypoint, or None (then that
    function, bit for bit).  The same returns and `trace` outputs; trace["road_j"] [N, n] is the waypoint whose row each control
    step used."""
    if road is None:
        return das.rollout_actuator(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, settings=settings,
                                    surface=surface, actuator=actuator, a0=a0, nn_window=nn_window, trace=trace, **kwargs)
    rows = np.ascontiguousarray(road, dtype=T)
    N, n = np.asarray(U).shape[:2]
    assert rows.shape == (n, 3)
    real_control, real_step = ds.control_step, ds.dynamic_step
    seen = dict(j=np.zeros(N, dtype=np.int64), used=[], found=[])

    def on_road(state, delta, pedal, c):
        j = seen["j"]
        seen["used"].append(j.copy())
        Pf_s, Pr_s = c.k["Pf"], c.k["Pr"]
        c.k["Pf"] = np.asarray(Pf_s * rows[j, 2], dtype=T)      # Pf_r = Pf_s n_z: one float32 multiply each
        c.k["Pr"] = np.asarray(Pr_s * rows[j, 2], dtype=T)
        ds.dynamic_step = lambda st, d, p, cc, h=None: road_step(st, d, p, cc, rows[j, 0], rows[j, 1], h)
        try:
            out = real_control(state, delta, pedal, c)
        finally:
            ds.dynamic_step = real_step
            c.k["Pf"], c.k["Pr"] = Pf_s, Pr_s
        seen["j"] = nearest(out[0], out[1], wp, j, nn_window)
        seen["found"].append(seen["j"].copy())
        return out

    record = {} if trace is None else trace
    ds.control_step = on_road
    try:
        got = das.rollout_actuator(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase,
                                   settings=dss.surface_settings(settings), surface=surface, actuator=actuator, a0=a0,
                                   nn_window=nn_window, trace=record, **kwargs)
    finally:
        ds.control_step = real_control
    # the search restated above is the one the rollout ran
    assert np.array_equal(np.stack(seen["found"], axis=1), record["j"])
    record["road_j"] = np.stack(seen["used"], axis=1)
    return got


def spec_costs(orc, dp, coef, vehicle, nn_window=None, U=None, return_states=False, **kwargs):
    """dynamic_actuator_spec.spec_costs with `road=` among the keywords."""
    kw = dp["kw"]
    return rollout_road(dp["x0"], coef, dp["U"] if U is None else U, vehicle, kw["step_cost"], kw["r_term"],
                        kw["final_cost"], kw["u_min"], kw["u_max"], kw["w_bound"], kw["dt"], kw["wheelbase"],
                        nn_window=nn_window, return_states=return_states, **kwargs)


def spec_ensemble(orc, dp, coef, vehicles, reduce=es.MEAN, weights=None, nn_window=None, U=None, return_states=False, **kwargs):
    """The ensemble on a road: every vehicle block rolled on its own trajectory's j, the table shared; then
    dynamic_ensemble_spec.combine.  States: vehicle 0's."""
    per = [spec_costs(orc, dp, coef, v, nn_window=nn_window, U=U, return_states=return_states and k == 0, **kwargs)
           for k, v in enumerate(vehicles)]
    Jc, V = es.combine([r[0] for r in per], [r[1] for r in per], reduce, weights)
    return (Jc, V, per[0][2]) if return_states else (Jc, V)


def trace_plans(dp, coef, U, vehicles, settings=Settings(), nn_window=None, u_prev=None, obstacles=None, surface=None,
                actuator=None, a0=None, road=None):
    """dynamic_actuator_spec.trace_plans on a road: dict(states [M, K, n + 1, 6], totals [M, K, 2], terms [M, K, n, 22])."""
    per = []
    for block in vehicles:
        per.append({})
        spec_costs(None, dp, coef, block, nn_window=nn_window, U=U, settings=settings, u_prev=u_prev, obstacles=obstacles,
                   surface=surface, actuator=actuator, a0=a0, road=road, trace=per[-1])
    return {name: np.stack([t[name] for t in per], axis=1) for name in ("states", "totals", "terms")}


def road_rows(grade, bank, g=9.81):
    """[n, 3] float32 of acmpc_set_road from grade and bank in radians: the float64 formulas, each value rounded once."""
    theta, beta = np.asarray(grade, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    return np.stack([-g * np.sin(theta), g * np.cos(theta) * np.sin(beta), np.cos(theta) * np.cos(beta)], axis=1).astype(T)


def random_road(n, seed, grade=0.10, bank=0.12):
    """[n, 3] float32: grade drawn uniformly within +-`grade` rad and bank within +-`bank` rad per waypoint."""
    rng = np.random.default_rng([9200, int(seed)])
    return road_rows(rng.uniform(-grade, grade, n), rng.uniform(-bank, bank, n))
