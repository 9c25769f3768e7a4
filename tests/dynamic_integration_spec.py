"""Mode D's integration setting restated in NumPy ("Mode D", "Sub-steps and the low-speed blend"):
a control step of dt as M Euler steps of h = float32(dt / M) under the same control, and after each of them the blend
of (vy, r) towards the kinematic bicycle's.  Built from tests/dynamic_spec.py - its dynamic_step is the sub-step, its
derived_constants the vehicle's floats, its sincos_spec the tangent's two halves - and bit-identical to the FINE kernels
of csrc/acmpc_dynamic.hip.  A helper of the tests, not a test file.

    h        = float32(dt / M), the quotient in float64 (M = 1: h == float32(dt))
    per sub-step: (X, Y, yaw, vx', vy', r') = dynamic_step(state, delta, pedal, k, h)          (vx' clipped at 0)
      td     = sd / cd                  sincos_spec(delta), IEEE division; the same for all M sub-steps
      r_k    = (vx' * td) * inv_L       inv_L = float32(1 / (lf + lr)), the sum and the quotient in float64
      vy_k   = r_k * lr
      lam    = fmax(fmin((vx' - v_lo) * inv_span, 1), 0)        inv_span = float32(1 / (v_hi - v_lo)), in float64
      vy     = lam * vy' + (1 - lam) * vy_k                     two multiplies and an add each, no fused multiply-add
      r      = lam * r'  + (1 - lam) * r_k

Everything round the step - nearest waypoint, cost, bounds, states, terminal cost - is dynamic_spec.rollout_dynamic's
own code, run once per control step on the state after the M-th sub-step: `setting()` swaps the step inside that module
for the duration of a `with` block, so the ensemble, sampled and softmin restatements (which all end in
dynamic_spec.rollout_dynamic) compose with this one by running inside the block."""
from __future__ import annotations

import contextlib

import numpy as np

import dynamic_spec as ds
from acmpc_oracle import sincos_spec

T = np.float32
MAX_SUBSTEPS = 16


def step_size(dt, substeps):
    """h = float32(dt / M): the quotient in float64, rounded once."""
    return T(float(dt) / int(substeps))


def blend_constants(low_speed_blend):
    """(v_lo, inv_span) as float32, each derived in float64 and rounded once; None when the blend is off."""
    if low_speed_blend is None:
        return None
    lo, hi = (float(v) for v in low_speed_blend)
    return T(lo), T(1.0 / (hi - lo))


def inverse_wheelbase(coef):
    """inv_L = float32(1 / (lf + lr)) of the vehicle block `coef`, in float64, rounded once."""
    v = dict(zip(ds.FIELDS, (float(x) for x in coef)))
    return T(1.0 / (v["lf"] + v["lr"]))


def fine_step(state, delta, pedal, k, inv_L, h, substeps, blend, sub_step=ds.dynamic_step):
    """One control step: `substeps` times dynamic_step with step h, the blend (`blend` = blend_constants(...) or None)
    after each.  Returns the state after the last sub-step."""
    delta = np.asarray(delta, dtype=T)
    st = tuple(np.asarray(s, dtype=T) for s in state)
    if blend is not None:
        v_lo, inv_span = blend
        sd, cd = sincos_spec(delta, T)
        with np.errstate(all="ignore"):
            td = (sd / cd).astype(T)
    for _ in range(int(substeps)):
        X, Y, yaw, vx, vy, r = sub_step(st, delta, pedal, k, h)
        if blend is not None:
            with np.errstate(all="ignore"):
                r_k = (vx * td) * inv_L
                vy_k = r_k * k["lr"]
                lam = np.fmax(np.fmin((vx - v_lo) * inv_span, T(1.0)), T(0.0))
                mu = T(1.0) - lam
                vy = lam * vy + mu * vy_k
                r = lam * r + mu * r_k
        st = tuple(np.asarray(a, dtype=T) for a in (X, Y, yaw, vx, vy, r))
    return st


@contextlib.contextmanager
def setting(substeps=1, low_speed_blend=None):
    """Inside the block every dynamic_spec.rollout_dynamic - called directly or through the ensemble, sampled and
    softmin restatements - integrates with this setting.  (1, None) runs the same machinery with one sub-step of
    h = float32(dt) and must then give dynamic_spec's own bits (tests/test_dynamic_integration.py holds it to that)."""
    substeps = int(substeps)
    if not 1 <= substeps <= MAX_SUBSTEPS:
        raise ValueError("substeps is 1 .. %d" % MAX_SUBSTEPS)
    blend = blend_constants(low_speed_blend)
    saved = ds.rollout_dynamic, ds.dynamic_step, ds.derived_constants
    rollout0, step0, constants0 = saved
    current = {}

    def derived_constants(coef):
        k = constants0(coef)
        k["inv_L"] = inverse_wheelbase(coef)
        return k

    def dynamic_step(state, delta, pedal, k, dt):   # (dt is the rollout's float32(dt): h comes from the float64 dt)
        return fine_step(state, delta, pedal, k, k["inv_L"], current["h"], substeps, blend, sub_step=step0)

    def rollout_dynamic(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, **kwargs):
        current["h"] = step_size(dt, substeps)
        return rollout0(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, **kwargs)

    ds.rollout_dynamic, ds.dynamic_step, ds.derived_constants = rollout_dynamic, dynamic_step, derived_constants
    try:
        yield
    finally:
        ds.rollout_dynamic, ds.dynamic_step, ds.derived_constants = saved


def rollout_dynamic(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, substeps=1, low_speed_blend=None,
                    **kwargs):
    """dynamic_spec.rollout_dynamic under the integration setting (substeps, low_speed_blend)."""
    with setting(substeps, low_speed_blend):
        return ds.rollout_dynamic(x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase, **kwargs)


def spec_costs(orc, dp, coef, vehicle, substeps=1, low_speed_blend=None, **kwargs):
    """dynamic_spec.spec_costs under the integration setting."""
    with setting(substeps, low_speed_blend):
        return ds.spec_costs(orc, dp, coef, vehicle, **kwargs)


def rollout_states(x0, U, vehicle, dt, substeps=1, low_speed_blend=None):
    """The six float32 states [B, n + 1, 6] of the control sequences U [B, n, 2] from the states x0 [B, 6], with no
    path: the float32 counterpart of DynamicBicycleParams.rollout (positions in the caller's frame, as given)."""
    k = ds.derived_constants(vehicle)
    inv_L, h, blend = inverse_wheelbase(vehicle), step_size(dt, substeps), blend_constants(low_speed_blend)
    x0, U = np.asarray(x0, dtype=T), np.asarray(U, dtype=T)
    st = tuple(x0[:, q].copy() for q in range(6))
    out = [np.stack(st, axis=1)]
    for i in range(U.shape[1]):
        st = fine_step(st, U[:, i, 0], U[:, i, 1], k, inv_L, h, substeps, blend)
        out.append(np.stack(st, axis=1))
    return np.stack(out, axis=1)
