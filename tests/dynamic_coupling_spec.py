"""Mode D's tyre coupling restated in NumPy ("Mode D, tyre coupling"): dynamic_spec's Euler step with
the friction-ellipse block between its longitudinal forces and its accelerations, built from dynamic_spec's pieces
(atan_spec, sin_spec, sincos_spec, derived_constants) and bit-identical to the coupled kernels of
csrc/acmpc_dynamic_coupled.hip and csrc/acmpc_identify.hip.  A helper of the tests, not a test file.

    rho_f, rho_r = float32(ratio)             each rounded once; +inf: no coupling on that axle
    after F_rx, F_fx and before xd3, everything float32 in this order, nothing fused, min / max = minNum / maxNum:
      cap_f = rho_f * Pf ;  cap_r = rho_r * Pr                 Pf, Pr the peaks THIS step uses (k["Pf"], k["Pr"]: the vehicle's,
                                                               or one per hypothesis in the identification)
      F_fx  = fmax(fmin(F_fx, cap_f), -cap_f) ;  F_rx likewise
      u_f   = F_fx / cap_f ;  u_r = F_rx / cap_r               IEEE division
      g_f   = sqrt(1 - u_f * u_f) ;  g_r likewise              one multiply, one subtraction, one correctly rounded sqrt
      F_fy  = F_fy * g_f ;  F_ry = F_ry * g_r
    xd3, xd4, xd5 use the clipped F_fx, F_rx and the scaled F_fy, F_ry; F_fric is left alone.

`setting(ratio)` swaps dynamic_spec.dynamic_step for the duration of a `with` block.  It is the OUTERMOST of the step-level
settings: dynamic_integration_spec.setting() entered inside it takes the coupled step as its sub-step.  The objective's and
the terms' settings swap the rollout, not the step, and go where they always go (the objective's outermost of all: before or
after this one).  The ensemble, sampled and softmin restatements end in dynamic_spec.rollout_dynamic and follow.

Where an existing helper bound the step when it was imported - dynamic_integration_spec.fine_step's default sub-step, and
through it rollout_states and grip_spec's segment loop - those few lines are restated here with the step looked up when it
is called."""
from __future__ import annotations

import contextlib

import numpy as np

import dynamic_integration_spec as dis
import dynamic_spec as ds
import grip_spec as gs
from acmpc_oracle import fma32, pick_best, sincos_spec

T = np.float32


def ratios(ratio):
    """(rho_f, rho_r) as float32, each rounded once; a scalar is both axles'."""
    pair = (ratio, ratio) if np.ndim(ratio) == 0 else tuple(ratio)
    with np.errstate(over="ignore"):
        rho_f, rho_r = T(float(pair[0])), T(float(pair[1]))
    assert rho_f > 0 and rho_r > 0, "a coupling ratio is > 0 (inf: none)"
    return rho_f, rho_r


def couple_axle(F_x, F_y, rho, P):
    """One axle: (clipped F_x, scaled F_y)."""
    with np.errstate(all="ignore"):
        cap = np.asarray(rho * P, dtype=T)
        F_x = np.fmax(np.fmin(F_x, cap), -cap)
        u = F_x / cap
        g = np.sqrt(T(1.0) - u * u)
        return np.asarray(F_x, dtype=T), np.asarray(F_y * g, dtype=T)


def coupled_step(ratio):
    """dynamic_spec.dynamic_step - its lines - with the coupling block of `ratio`."""
    rho_f, rho_r = ratios(ratio)

    def dynamic_step(state, delta, pedal, k, dt):
        X, Y, yaw, vx, vy, r = (np.asarray(s, dtype=T) for s in state)
        delta = np.asarray(delta, dtype=T)
        pedal = np.asarray(pedal, dtype=T)
        dt = T(dt)
        with np.errstate(all="ignore"):
            den = vx + T(ds.VX_EPS)
            qf = (r * k["lf"] + vy) / den
            qr = (r * k["lr"] - vy) / den
            a_f = delta - ds.atan_spec(qf)
            a_r = ds.atan_spec(qr)
            bf = k["Bf"] * a_f
            yf = bf - k["Ef"] * (bf - ds.atan_spec(bf))
            F_fy = k["Pf"] * ds.sin_spec(k["Cf"] * ds.atan_spec(yf))
            br = k["Br"] * a_r
            yr = br - k["Er"] * (br - ds.atan_spec(br))
            F_ry = k["Pr"] * ds.sin_spec(k["Cr"] * ds.atan_spec(yr))
            vx2 = vx * vx
            F_fric = (k["fric0"] - k["Cfric2"] * vx) - k["Cfric3"] * vx2
            brake = (k["Cb1"] - k["Cb2"] * vx) - k["Cb3"] * vx2
            motor = (k["Cm1"] - k["Cm2"] * vx) - k["Cm3"] * vx2
            p_neg = np.fmin(pedal, T(0.0))
            p_pos = np.fmax(pedal, T(0.0))
            F_rx = (brake * k["bias_rear"]) * p_neg + motor * p_pos
            F_fx = (brake * k["bias_front"]) * p_neg
            F_fx, F_fy = couple_axle(F_fx, F_fy, rho_f, k["Pf"])
            F_rx, F_ry = couple_axle(F_rx, F_ry, rho_r, k["Pr"])
            sd, cd = sincos_spec(delta, T)
            sy, cy = sincos_spec(yaw, T)
            xd0 = vx * cy - vy * sy
            xd1 = vx * sy + vy * cy
            xd3 = k["inv_mass"] * ((((F_rx + F_fx) + F_fric) - F_fy * sd) + (k["mass"] * vy) * r)
            xd4 = k["inv_mass"] * ((F_ry + F_fy * cd) - (k["mass"] * vx) * r)
            xd5 = k["inv_Iz"] * ((F_fy * k["lf"]) * cd - F_ry * k["lr"])
            Xn = X + xd0 * dt
            Yn = Y + xd1 * dt
            yawn = yaw + r * dt
            vxn = np.fmax(vx + xd3 * dt, T(0.0))
            vyn = vy + xd4 * dt
            rn = r + xd5 * dt
        return tuple(np.asarray(a, dtype=T) for a in (Xn, Yn, yawn, vxn, vyn, rn))

    return dynamic_step


@contextlib.contextmanager
def setting(ratio):
    """Inside the block dynamic_spec.dynamic_step is the coupled step of `ratio` (None: the block changes nothing), for
    every restatement that looks the step up in that module - dynamic_spec's, the terms' and the objective's rollouts, and
    dynamic_integration_spec.setting() entered INSIDE this block."""
    if ratio is None:
        yield
        return
    if ds.dynamic_step.__module__ != ds.__name__:
        raise RuntimeError("dynamic_coupling_spec.setting() is the outermost of the step-level settings: before the integration's")
    saved = ds.dynamic_step
    ds.dynamic_step = coupled_step(ratio)
    try:
        yield
    finally:
        ds.dynamic_step = saved


def fine_step(state, delta, pedal, k, inv_L, h, substeps, blend):
    """dynamic_integration_spec.fine_step with the sub-step that dynamic_spec holds NOW (its own default was bound when the
    module was imported)."""
    return dis.fine_step(state, delta, pedal, k, inv_L, h, substeps, blend, sub_step=ds.dynamic_step)


def rollout_states(ratio, x0, U, vehicle, dt, substeps=1, low_speed_blend=None):
    """dynamic_integration_spec.rollout_states - its lines - under the coupling `ratio`: the six float32 states
    [B, n + 1, 6], the float32 counterpart of DynamicBicycleParams.rollout(..., coupling=ratio)."""
    with setting(ratio):
        k = ds.derived_constants(vehicle)
        inv_L, h, blend = dis.inverse_wheelbase(vehicle), dis.step_size(dt, substeps), dis.blend_constants(low_speed_blend)
        x0, U = np.asarray(x0, dtype=T), np.asarray(U, dtype=T)
        st = tuple(x0[:, q].copy() for q in range(6))
        out = [np.stack(st, axis=1)]
        for i in range(U.shape[1]):
            st = fine_step(st, U[:, i, 0], U[:, i, 1], k, inv_L, h, substeps, blend)
            out.append(np.stack(st, axis=1))
        return np.stack(out, axis=1)


def segment_errors(ratio, vehicle0, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0), substeps=1,
                   low_speed_blend=None):
    """grip_spec.segment_errors - its lines - under the coupling `ratio`: hypothesis k is capped by its own Pf_k, Pr_k."""
    states, controls = np.asarray(states, dtype=T), np.asarray(controls, dtype=T)
    W, L = controls.shape[0], int(segment)
    assert states.shape == (W + 1, 3) and 1 <= W <= gs.MAX_LOG_STEPS and 1 <= L <= W
    k = gs.hypothesis_constants(vehicle0, scales)
    K = k["Pf"].size
    inv_L, h, blend = dis.inverse_wheelbase(vehicle0), dis.step_size(dt, substeps), dis.blend_constants(low_speed_blend)
    w = [T(float(v)) for v in weights]
    starts = np.arange(0, W, L)
    S = starts.size
    st = tuple(np.zeros((S, K), dtype=T) for _ in range(3)) + tuple(np.repeat(states[starts, q][:, None], K, axis=1) for q in range(3))
    e = np.zeros((S, K), dtype=T)
    out = np.zeros((S, K), dtype=T)
    with setting(ratio):
        for i in range(L):
            if starts[-1] + i >= W:          # the last segment is over
                out[-1] = e[-1]
                starts, e, st = starts[:-1], e[:-1], tuple(a[:-1] for a in st)
                if starts.size == 0:
                    break
            j = starts + i
            ones = np.ones((1, K), dtype=T)
            st = fine_step(st, controls[j, 0][:, None] * ones, controls[j, 1][:, None] * ones, k, inv_L, h, substeps, blend)
            with np.errstate(all="ignore"):
                for q in range(3):
                    d = st[3 + q] - states[j + 1, q][:, None]
                    e = fma32(w[q] * d, d, e)
    out[:starts.size] = e
    return out


def score(ratio, vehicle0, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0), substeps=1, low_speed_blend=None):
    """(errors [K] float32, best index) of the identification under the coupling `ratio` (grip_spec.score's sum and pick)."""
    e = segment_errors(ratio, vehicle0, states, controls, dt, scales, segment, weights, substeps, low_speed_blend)
    E = e[0].copy()
    with np.errstate(all="ignore"):
        for s in range(1, e.shape[0]):
            E = (E + e[s]).astype(T)
    return E, int(pick_best(E)[0])


def braking_log(plant, coupling, steps=40, dt=0.05, vx0=40.0, pedal=-1.0):
    """A straight-line braking log driven on `plant` (the float64 mirror under `coupling`): delta = 0, a constant pedal,
    rounded to float32.  (states [W + 1, 3], controls [W, 2])"""
    controls = np.stack([np.zeros(steps), np.full(steps, pedal)], axis=1).astype(T)
    traj = plant.rollout(np.array([0.0, 0.0, 0.0, vx0, 0.0, 0.0]), controls.astype(np.float64), dt, coupling=coupling)
    return traj[:, 3:].astype(T), controls
