"""Mode D's cost in plain float64, written from the definitions of DESIGN.md section 2 ("Mode D", "Mode D ensembles") and
of mode T's cost - NOT from the kernel's operation order: library arctan / sin / cos, the true squared distance to every
waypoint, e_y and e_psi in the caller's frame, a modulo for the wrap, plain sums.  tests/test_dynamic_cost_float64.py holds
the float32 specification (tests/dynamic_spec.py, which the kernels equal bit for bit) against it.  A helper of the tests,
not a test file.

Inputs are data: the packed float32 table [n, 8] = [x, y, cos psi, sin psi, psi, k_ref, v_ref, w/2 - margin]
(oracle coefficients_temporal; of it only x, y, psi, k_ref, v_ref and the half width are read - cos and sin are taken of
psi here), the float32 x0 = (X, Y, yaw, vx, vy, r) and controls U [N, n, 2] = (delta, pedal), dt, the weights and the 26
doubles of a vehicle block (acmpc_amd.dynamic_model.FIELDS order)."""
from __future__ import annotations

import numpy as np

FIELDS = ("F_z0", "Bf", "Cf", "Df", "Ef", "epsf", "Br", "Cr", "Dr", "Er", "epsr", "mass", "Iz", "g", "lf", "lr",
          "brake_bias", "Cm1", "Cm2", "Cm3", "Cb1", "Cb2", "Cb3", "Cfric1", "Cfric2", "Cfric3")
COL_X, COL_Y, COL_PSI, COL_KREF, COL_VREF, COL_HALF = 0, 1, 4, 5, 6, 7
VX_EPS = 1.0e-3


def step64(state, delta, pedal, vehicle, dt, coupling=None, load_transfer=None):
    """One explicit Euler step of the dynamic bicycle on arrays, then vx = max(vx, 0): state [..., 6] float64.  `coupling` =
    rho or (rho_f, rho_r) and `load_transfer` = h_cg or (h_cg, w_frac) are DynamicBicycleParams.predict_next_state's (DESIGN.md
    section 2, "tyre coupling", "load transfer"): the load moved to the rear w = h_cg / (lf + lr) (e_f + e_r), the demands e
    clipped at the static caps and w at +-w_frac min(F_zf, F_zr), gives the axle loads both the side force's peak and the
    coupling's cap take; per axle F_x is clipped at +-rho P and F_y scaled by sqrt(1 - (F_x / (rho P))^2)."""
    v = dict(zip(FIELDS, (float(x) for x in vehicle)))
    X, Y, yaw, vx, vy, r = (state[..., q] for q in range(6))
    F_zf = v["mass"] * v["g"] * v["lr"] / (v["lr"] + v["lf"])
    F_zr = v["mass"] * v["g"] * v["lf"] / (v["lr"] + v["lf"])

    def peak(D, eps, F_z):
        return D * (1.0 + eps * F_z / v["F_z0"]) * F_z / v["F_z0"]

    def lateral(alpha, B, C, D, E, eps, F_z):
        return peak(D, eps, F_z) * np.sin(C * np.arctan(B * alpha - E * (B * alpha - np.arctan(B * alpha))))

    def pair(setting, second):
        return (float(setting), second) if np.ndim(setting) == 0 else tuple(float(x) for x in setting)

    with np.errstate(all="ignore"):
        alpha_f = delta - np.arctan((r * v["lf"] + vy) / (vx + VX_EPS))
        alpha_r = np.arctan((r * v["lr"] - vy) / (vx + VX_EPS))
        brake = v["Cb1"] - v["Cb2"] * vx - v["Cb3"] * vx ** 2
        motor = v["Cm1"] - v["Cm2"] * vx - v["Cm3"] * vx ** 2
        F_fric = -v["Cfric1"] - v["Cfric2"] * vx - v["Cfric3"] * vx ** 2
        F_rx = brake * (1.0 - v["brake_bias"]) * np.minimum(pedal, 0.0) + motor * np.maximum(pedal, 0.0)
        F_fx = brake * v["brake_bias"] * np.minimum(pedal, 0.0)
        rho_f, rho_r = (np.inf, np.inf) if coupling is None else pair(coupling, float(np.ravel(coupling)[0]))
        load_f, load_r = F_zf, F_zr
        if load_transfer is not None:
            h_cg, w_frac = pair(load_transfer, 0.9)
            e_f = np.clip(F_fx, -rho_f * peak(v["Df"], v["epsf"], F_zf), rho_f * peak(v["Df"], v["epsf"], F_zf))
            e_r = np.clip(F_rx, -rho_r * peak(v["Dr"], v["epsr"], F_zr), rho_r * peak(v["Dr"], v["epsr"], F_zr))
            w_max = w_frac * min(F_zf, F_zr)
            w = np.clip(h_cg / (v["lf"] + v["lr"]) * (e_f + e_r), -w_max, w_max)
            load_f, load_r = F_zf - w, F_zr + w
        F_fy = lateral(alpha_f, v["Bf"], v["Cf"], v["Df"], v["Ef"], v["epsf"], load_f)
        F_ry = lateral(alpha_r, v["Br"], v["Cr"], v["Dr"], v["Er"], v["epsr"], load_r)
        if coupling is not None:
            cap_f, cap_r = rho_f * peak(v["Df"], v["epsf"], load_f), rho_r * peak(v["Dr"], v["epsr"], load_r)
            F_fx = np.clip(F_fx, -cap_f, cap_f)
            F_rx = np.clip(F_rx, -cap_r, cap_r)
            F_fy = F_fy * np.sqrt(1.0 - (F_fx / cap_f) ** 2)
            F_ry = F_ry * np.sqrt(1.0 - (F_rx / cap_r) ** 2)
        x_dot = np.stack([vx * np.cos(yaw) - vy * np.sin(yaw),
                          vx * np.sin(yaw) + vy * np.cos(yaw),
                          r,
                          (F_rx + F_fx + F_fric - F_fy * np.sin(delta) + v["mass"] * vy * r) / v["mass"],
                          (F_ry + F_fy * np.cos(delta) - v["mass"] * vx * r) / v["mass"],
                          (F_fy * v["lf"] * np.cos(delta) - F_ry * v["lr"]) / v["Iz"]], axis=-1)
        nxt = state + x_dot * dt
    nxt[..., 3] = np.maximum(nxt[..., 3], 0.0)
    return nxt


def control_step64(state, delta, pedal, vehicle, dt, substeps=1, low_speed_blend=None, coupling=None, load_transfer=None):
    """One control step as DynamicBicycleParams.rollout takes it ("sub-steps and the low-speed blend"):
    `substeps` Euler steps of dt / substeps under the same control, and after each of them (vy, r) blended towards the kinematic
    bicycle's r_k = vx tan(delta) / (lf + lr), vy_k = lr r_k by lam = clamp((vx - v_lo) / (v_hi - v_lo), 0, 1)."""
    if substeps == 1 and low_speed_blend is None:
        return step64(state, delta, pedal, vehicle, dt, coupling, load_transfer)
    v = dict(zip(FIELDS, (float(x) for x in vehicle)))
    h = dt / int(substeps)
    for _ in range(int(substeps)):
        state = step64(state, delta, pedal, vehicle, h, coupling, load_transfer)
        if low_speed_blend is not None:
            v_lo, v_hi = (float(x) for x in low_speed_blend)
            with np.errstate(all="ignore"):
                r_k = state[..., 3] * np.tan(delta) / (v["lf"] + v["lr"])
                lam = np.clip((state[..., 3] - v_lo) / (v_hi - v_lo), 0.0, 1.0)
                state[..., 4] = lam * state[..., 4] + (1.0 - lam) * (r_k * v["lr"])
                state[..., 5] = lam * state[..., 5] + (1.0 - lam) * r_k
    return state


def rollout64(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, nn_window=None, substeps=1,
              low_speed_blend=None, coupling=None, load_transfer=None, terms=None, u_prev=None, objective=None):
    """Every candidate's cost under one vehicle.  Returns a dict: cost = J + w_bound V, J, V [N]; e_y [N, n] (the lateral
    error at every step), j [N, n] (the nearest waypoint), gap [N] (the smallest difference, over the steps, between the
    two smallest squared distances of the search: a near-tie is where float32 may pick the other waypoint), states
    [N, n + 1, 6].

    The settings of the handle, each off by default (and the outputs then what they were without them, bit for bit):
    `substeps`, `low_speed_blend`, `coupling`, `load_transfer` are control_step64's; `terms` = dict(rate_weight=, rate_max=,
    slip_weight=, slip_max=) with the previous control `u_prev` = (delta, pedal) or None, and `objective` =
    dict(progress_weight=, speed_ceiling=), add the lines of DESIGN.md section 2 ("rate and slip terms", "progress and
    ceiling") in float64:
        rd_i = (delta_i - delta_{i-1}) / dt, rp_i likewise (step 0 against u_prev, or a zero increment), b_i = (r lr - vy) /
        (vx + 1e-3) on the state after control step i;   E = 1/2 sum_i (w_d rd_i^2 + w_p rp_i^2 + w_s b_i^2) joins J and the
        squared excesses of |rd|, |rp|, |b| over their limits join V;
        cap_i = scale v_ref_j + offset at step i's nearest waypoint j: the squared excess of vx over it joins V;
        s = (the polyline's length up to the last step's nearest waypoint j) + cos psi_j (X - x_j) + sin psi_j (Y - y_j) of the
        last state: J loses progress_weight s.
    A part that is off adds nothing and reads nothing (a NaN u_prev beside a rate part that is off).  The dict then also holds
    E, s [N] (0 where the part is off) and, per hard limit that is on, `slack`[name] [N, n]: the hinge's argument (negative:
    inside the limit) for name in rate_delta, rate_pedal, slip, ceiling - what a test needs to except the candidates that
    come within the float32 side's drift of a limit."""
    wp = np.asarray(wp, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    N, n, _ = U.shape
    px, py, psi = wp[:, COL_X], wp[:, COL_Y], wp[:, COL_PSI]
    delta_ref = np.arctan(float(wheelbase) * wp[:, COL_KREF])
    Q, R, QN = (np.asarray(a, dtype=np.float64) for a in (Q, R, QN))
    lo, hi = np.asarray(u_lo, dtype=np.float64), np.asarray(u_hi, dtype=np.float64)
    state = np.tile(np.asarray(x0, dtype=np.float64), (N, 1))
    states = np.empty((N, n + 1, 6))
    states[:, 0] = state
    J = np.zeros(N)
    V = np.zeros(N)
    e_y_all = np.empty((N, n))
    j_all = np.empty((N, n), dtype=np.int64)
    gap = np.full(N, np.inf)
    j_prev = np.zeros(N, dtype=np.int64)
    e_y = e_psi = np.zeros(N)
    plain_step = substeps == 1 and low_speed_blend is None and coupling is None and load_transfer is None
    INF = float("inf")
    t = dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=None)
    t.update(terms or {})
    o = dict(progress_weight=0.0, speed_ceiling=None)
    o.update(objective or {})
    w_rate = [float(x) for x in t["rate_weight"]]
    rate_max = [INF, INF] if t["rate_max"] is None else [INF if x is None else float(x) for x in t["rate_max"]]
    w_slip, slip_max = float(t["slip_weight"]), INF if t["slip_max"] is None else float(t["slip_max"])
    rate_on = any(x != 0.0 for x in w_rate) or any(np.isfinite(x) for x in rate_max)
    slip_on = w_slip != 0.0 or np.isfinite(slip_max)
    ceiling = o["speed_ceiling"]
    if ceiling is not None:
        ceiling = (float(ceiling), 0.0) if np.ndim(ceiling) == 0 else tuple(float(x) for x in ceiling)
    lr = float(dict(zip(FIELDS, vehicle))["lr"])
    E = np.zeros(N)
    slack = {}
    prev_u = None
    if rate_on and u_prev is not None:
        prev_u = np.tile(np.asarray(u_prev, dtype=np.float64), (N, 1))
    for i in range(n):
        delta, pedal = U[:, i, 0], U[:, i, 1]
        if plain_step:
            state = step64(state, delta, pedal, vehicle, float(dt))
        else:
            state = control_step64(state, delta, pedal, vehicle, float(dt), substeps, low_speed_blend, coupling, load_transfer)
        states[:, i + 1] = state
        X, Y, yaw, vx = state[:, 0], state[:, 1], state[:, 2], state[:, 3]
        d2 = (X[:, None] - px[None, :]) ** 2 + (Y[:, None] - py[None, :]) ** 2          # [N, n]
        if nn_window is not None:   # only the back + ahead + 1 waypoints from clamp(j_prev - back, 0, n - width)
            back, ahead = nn_window
            width = back + ahead + 1
            first = np.clip(j_prev - back, 0, max(n - width, 0))
            m = np.arange(n)[None, :]
            d2 = np.where((m >= first[:, None]) & (m < first[:, None] + width), d2, np.inf)
        j = np.argmin(d2, axis=1)                                                        # the first minimum
        if n > 1:
            two = np.partition(d2, 1, axis=1)[:, :2]
            gap = np.minimum(gap, two[:, 1] - two[:, 0])
        j_prev = j
        e_y = np.cos(psi[j]) * (Y - py[j]) - np.sin(psi[j]) * (X - px[j])
        e_psi = np.mod(yaw - psi[j] + np.pi, 2.0 * np.pi) - np.pi
        dv = vx - wp[j, COL_VREF]
        dk = delta - delta_ref[j]
        J += 0.5 * (Q[0] * e_y ** 2 + Q[1] * e_psi ** 2 + R[0] * dv ** 2 + R[1] * dk ** 2)
        V += np.maximum(np.maximum(lo[0] - delta, delta - hi[0]), 0.0) ** 2
        V += np.maximum(np.maximum(lo[1] - pedal, pedal - hi[1]), 0.0) ** 2
        V += np.maximum(np.abs(e_y) - wp[j, COL_HALF], 0.0) ** 2
        e_y_all[:, i] = e_y
        j_all[:, i] = j
        with np.errstate(all="ignore"):
            if rate_on:
                rates = (U[:, i] - (U[:, i] if prev_u is None else prev_u)) / float(dt)
                prev_u = U[:, i]
                for q, name in enumerate(("rate_delta", "rate_pedal")):
                    E += 0.5 * w_rate[q] * rates[:, q] ** 2
                    over = np.abs(rates[:, q]) - rate_max[q]
                    V += np.maximum(over, 0.0) ** 2
                    if np.isfinite(rate_max[q]):
                        slack.setdefault(name, np.empty((N, n)))[:, i] = over
            if slip_on:
                b = (state[:, 5] * lr - state[:, 4]) / (vx + VX_EPS)
                E += 0.5 * w_slip * b ** 2
                V += np.maximum(np.abs(b) - slip_max, 0.0) ** 2
                if np.isfinite(slip_max):
                    slack.setdefault("slip", np.empty((N, n)))[:, i] = np.abs(b) - slip_max
            if ceiling is not None:
                over = vx - (ceiling[0] * wp[j, COL_VREF] + ceiling[1])
                V += np.maximum(over, 0.0) ** 2
                slack.setdefault("ceiling", np.empty((N, n)))[:, i] = over
    J += 0.5 * (QN[0] * e_y ** 2 + QN[1] * e_psi ** 2 + QN[2] * (n * float(dt)) ** 2)
    out = dict(e_y=e_y_all, j=j_all, gap=gap, states=states)
    if terms is not None or objective is not None:
        s = np.zeros(N)
        if rate_on or slip_on:
            J = J + E
        if float(o["progress_weight"]) != 0.0:
            arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(px), np.diff(py)))])
            s = arc[j] + np.cos(psi[j]) * (state[:, 0] - px[j]) + np.sin(psi[j]) * (state[:, 1] - py[j])
            J = J - float(o["progress_weight"]) * s
        out.update(E=E, s=s, slack=slack)
    out.update(cost=J + float(w_bound) * V, J=J, V=V)
    return out


def combine64(costs, violations, reduce="mean", weights=None):
    """The ensemble's cost - the normalised weighted mean or the max of the K costs - and violation, the max."""
    costs = np.asarray(costs, dtype=np.float64)
    K = costs.shape[0]
    if reduce == "mean":
        w = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64) / np.sum(weights)
        cost = np.tensordot(w, costs, axes=(0, 0))
    else:
        cost = costs.max(axis=0)
    return cost, np.asarray(violations, dtype=np.float64).max(axis=0)


def reference_costs(dp, coef, vehicle, nn_window=None, U=None, **settings):
    """rollout64 of problem `dp` (dynamic_spec.make_dynamic_problem) on the packed table `coef`; `settings`: rollout64's."""
    kw = dp["kw"]
    return rollout64(dp["x0"], coef, dp["U"] if U is None else U, vehicle, kw["step_cost"], kw["r_term"],
                     kw["final_cost"], kw["u_min"], kw["u_max"], kw["w_bound"], kw["dt"], kw["wheelbase"],
                     nn_window=nn_window, **settings)
