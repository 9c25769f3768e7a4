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


def step64(state, delta, pedal, vehicle, dt):
    """One explicit Euler step of the dynamic bicycle on arrays, then vx = max(vx, 0): state [..., 6] float64."""
    v = dict(zip(FIELDS, (float(x) for x in vehicle)))
    X, Y, yaw, vx, vy, r = (state[..., q] for q in range(6))
    F_zf = v["mass"] * v["g"] * v["lr"] / (v["lr"] + v["lf"])
    F_zr = v["mass"] * v["g"] * v["lf"] / (v["lr"] + v["lf"])

    def lateral(alpha, B, C, D, E, eps, F_z):
        peak = D * (1.0 + eps * F_z / v["F_z0"]) * F_z / v["F_z0"]
        return peak * np.sin(C * np.arctan(B * alpha - E * (B * alpha - np.arctan(B * alpha))))

    with np.errstate(all="ignore"):
        alpha_f = delta - np.arctan((r * v["lf"] + vy) / (vx + VX_EPS))
        alpha_r = np.arctan((r * v["lr"] - vy) / (vx + VX_EPS))
        F_fy = lateral(alpha_f, v["Bf"], v["Cf"], v["Df"], v["Ef"], v["epsf"], F_zf)
        F_ry = lateral(alpha_r, v["Br"], v["Cr"], v["Dr"], v["Er"], v["epsr"], F_zr)
        brake = v["Cb1"] - v["Cb2"] * vx - v["Cb3"] * vx ** 2
        motor = v["Cm1"] - v["Cm2"] * vx - v["Cm3"] * vx ** 2
        F_fric = -v["Cfric1"] - v["Cfric2"] * vx - v["Cfric3"] * vx ** 2
        F_rx = brake * (1.0 - v["brake_bias"]) * np.minimum(pedal, 0.0) + motor * np.maximum(pedal, 0.0)
        F_fx = brake * v["brake_bias"] * np.minimum(pedal, 0.0)
        x_dot = np.stack([vx * np.cos(yaw) - vy * np.sin(yaw),
                          vx * np.sin(yaw) + vy * np.cos(yaw),
                          r,
                          (F_rx + F_fx + F_fric - F_fy * np.sin(delta) + v["mass"] * vy * r) / v["mass"],
                          (F_ry + F_fy * np.cos(delta) - v["mass"] * vx * r) / v["mass"],
                          (F_fy * v["lf"] * np.cos(delta) - F_ry * v["lr"]) / v["Iz"]], axis=-1)
        nxt = state + x_dot * dt
    nxt[..., 3] = np.maximum(nxt[..., 3], 0.0)
    return nxt


def rollout64(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, nn_window=None):
    """Every candidate's cost under one vehicle.  Returns a dict: cost = J + w_bound V, J, V [N]; e_y [N, n] (the lateral
    error at every step), j [N, n] (the nearest waypoint), gap [N] (the smallest difference, over the steps, between the
    two smallest squared distances of the search: a near-tie is where float32 may pick the other waypoint), states
    [N, n + 1, 6]."""
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
    for i in range(n):
        delta, pedal = U[:, i, 0], U[:, i, 1]
        state = step64(state, delta, pedal, vehicle, float(dt))
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
    J += 0.5 * (QN[0] * e_y ** 2 + QN[1] * e_psi ** 2 + QN[2] * (n * float(dt)) ** 2)
    return dict(cost=J + float(w_bound) * V, J=J, V=V, e_y=e_y_all, j=j_all, gap=gap, states=states)


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


def reference_costs(dp, coef, vehicle, nn_window=None, U=None):
    """rollout64 of problem `dp` (dynamic_spec.make_dynamic_problem) on the packed table `coef`."""
    kw = dp["kw"]
    return rollout64(dp["x0"], coef, dp["U"] if U is None else U, vehicle, kw["step_cost"], kw["r_term"],
                     kw["final_cost"], kw["u_min"], kw["u_max"], kw["w_bound"], kw["dt"], kw["wheelbase"],
                     nn_window=nn_window)
