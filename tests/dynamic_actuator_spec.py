"""Mode D's rollout under the actuator lag (acmpc_set_dynamics_actuator, DESIGN.md section 2 "Mode D, actuator") restated in
float32 NumPy.

The setting is tau = (tau_d, tau_p) seconds for the steering and the pedal channel, each finite and >= 0.  With dt the control
step, per channel, in float64 and rounded to float32 once each:

    k_c = exp(-dt / tau_c)             what is left of an error after one control step      (tau_c = 0:  k_c = 0)
    m_c = (tau_c / dt) (1 - k_c)       the mean of what is left over the step's interval    (tau_c = 0:  m_c = 0)

A candidate carries the two actuator positions (a_d, a_p).  At the top of control step i, before anything of the step runs, in
float32 with nothing fused (the pedal channel likewise with k_p, m_p, a_p):

    e       = delta_i - a_d
    delta_x = delta_i - m_d * e        what the vehicle is driven on during step i
    a_d     = delta_i - k_d * e        the position at the end of the step

The control step - the control's terms, every sub-step, the blend's tan(delta) - reads (delta_x, pedal_x); dynamic_cost (the input
box, dk), the rate terms, the records' u and the sampler stay on the command.  a0 = (a_d, a_p) at the start of the plan, or None:
step 0's own command then stands for it (e = +0).  The step under the setting is the top-tier step whatever else is set
(dynamic_surface_spec.surface_settings: a tier that is off gets its neutral value).

Composed over dynamic_surface_spec.rollout_surface, unedited: that loop makes exactly one call of dynamic_spec.control_step per
control step, with the command, and reads the command everywhere else - so for the length of one rollout `control_step` is
replaced by `lagged`, which carries the positions, applies the three lines and hands the applied control to the real step.  A
helper of the tests, not a test file."""
from __future__ import annotations

import numpy as np

import dynamic_ensemble_spec as es
import dynamic_spec as ds
import dynamic_surface_spec as dss
from dynamic_spec import Settings, T


def coefficients(tau, dt):
    """((k_d, k_p), (m_d, m_p)) as the float32 the kernels get: derived in float64, each rounded once."""
    k, m = [], []
    for t in tau:
        t = float(t)
        assert np.isfinite(t) and t >= 0.0
        kc = np.exp(-float(dt) / t) if t > 0.0 else 0.0
        mc = (t / float(dt)) * (1.0 - kc) if t > 0.0 else 0.0
        k.append(T(kc))
        m.append(T(mc))
    return tuple(k), tuple(m)


def filter_controls(U, a0, tau, dt):
    """The three lines over commands U [..., n, 2] in float32: (applied [..., n, 2], positions [..., n + 1, 2])."""
    U = np.asarray(U, dtype=T)
    k, m = coefficients(tau, dt)
    n = U.shape[-2]
    a = U[..., 0, :].copy() if a0 is None else np.broadcast_to(np.asarray(a0, dtype=T), U[..., 0, :].shape).copy()
    applied, positions = np.empty_like(U), np.empty(U.shape[:-2] + (n + 1, 2), dtype=T)
    positions[..., 0, :] = a
    for i in range(n):
        for ch in range(2):
            u = U[..., i, ch]
            e = np.asarray(u - a[..., ch], dtype=T)
            applied[..., i, ch] = np.asarray(u - np.asarray(m[ch] * e, dtype=T), dtype=T)
            a[..., ch] = np.asarray(u - np.asarray(k[ch] * e, dtype=T), dtype=T)
        positions[..., i + 1, :] = a
    return applied, positions


def rollout_actuator(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, settings=Settings(), surface=None,
                     actuator=None, a0=None, **kwargs):
    """dynamic_surface_spec.rollout_surface with `actuator` = (tau_d, tau_p) or None (then that function, bit for bit) and `a0` =
    (a_d, a_p) or None.  The same returns and `trace` outputs: states are the lagged trajectory, every term is on the command."""
    if actuator is None:
        return dss.rollout_surface(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, settings=settings,
                                   surface=surface, **kwargs)
    k, m = coefficients(actuator, dt)
    real = ds.control_step
    pos = {}

    def lagged(state, delta, pedal, c):
        delta, pedal = np.asarray(delta, dtype=T), np.asarray(pedal, dtype=T)
        if not pos:
            pos["d"] = delta if a0 is None else np.full(delta.shape, a0[0], dtype=T)
            pos["p"] = pedal if a0 is None else np.full(pedal.shape, a0[1], dtype=T)
        with np.errstate(all="ignore"):
            ed = np.asarray(delta - pos["d"], dtype=T)
            ep = np.asarray(pedal - pos["p"], dtype=T)
            dx = np.asarray(delta - np.asarray(m[0] * ed, dtype=T), dtype=T)
            px = np.asarray(pedal - np.asarray(m[1] * ep, dtype=T), dtype=T)
            pos["d"] = np.asarray(delta - np.asarray(k[0] * ed, dtype=T), dtype=T)
            pos["p"] = np.asarray(pedal - np.asarray(k[1] * ep, dtype=T), dtype=T)
        return real(state, dx, px, c)

    ds.control_step = lagged
    try:
        return dss.rollout_surface(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase,
                                   settings=dss.surface_settings(settings), surface=surface, **kwargs)
    finally:
        ds.control_step = real


def spec_costs(orc, dp, coef, vehicle, nn_window=None, U=None, return_states=False, **kwargs):
    """dynamic_surface_spec.spec_costs with `actuator=` and `a0=` among the keywords."""
    kw = dp["kw"]
    return rollout_actuator(dp["x0"], coef, dp["U"] if U is None else U, vehicle, kw["step_cost"], kw["r_term"],
                            kw["final_cost"], kw["u_min"], kw["u_max"], kw["w_bound"], kw["dt"], kw["wheelbase"],
                            nn_window=nn_window, return_states=return_states, **kwargs)


def spec_ensemble(orc, dp, coef, vehicles, reduce=es.MEAN, weights=None, nn_window=None, U=None, return_states=False, **kwargs):
    """The ensemble under the lag: every vehicle carries the same filter; then dynamic_ensemble_spec.combine.  States: vehicle 0's."""
    per = [spec_costs(orc, dp, coef, v, nn_window=nn_window, U=U, return_states=return_states and k == 0, **kwargs)
           for k, v in enumerate(vehicles)]
    Jc, V = es.combine([r[0] for r in per], [r[1] for r in per], reduce, weights)
    return (Jc, V, per[0][2]) if return_states else (Jc, V)


def trace_plans(dp, coef, U, vehicles, settings=Settings(), nn_window=None, u_prev=None, obstacles=None, surface=None,
                actuator=None, a0=None):
    """dynamic_surface_spec.trace_plans under the lag: dict(states [M, K, n + 1, 6], totals [M, K, 2], terms [M, K, n, 22])."""
    per = []
    for block in vehicles:
        per.append({})
        spec_costs(None, dp, coef, block, nn_window=nn_window, U=U, settings=settings, u_prev=u_prev, obstacles=obstacles,
                   surface=surface, actuator=actuator, a0=a0, trace=per[-1])
    return {name: np.stack([t[name] for t in per], axis=1) for name in ("states", "totals", "terms")}
