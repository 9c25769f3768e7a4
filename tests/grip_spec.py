"""Mode D's grip identification restated in NumPy ("Mode D, grip identification"): K hypothetical
vehicles - vehicle 0 with its two axle peaks scaled - rolled over a logged window of (vx, vy, r) under the logged (delta,
pedal) and scored by their prediction error, bit-identical to csrc/acmpc_identify.hip.  Nothing is specified here about
the step itself: it is dynamic_spec's control_step under the handle's `settings` (sub-steps, blend, coupling, load transfer,
downforce), with a peak per hypothesis where a rollout has the vehicle's.  A helper of the tests, not a test file.

    hypothesis k   vehicle 0's block with Df sf_k and Dr sr_k, derived as any block: Pf_k, Pr_k in float64, rounded once;
                   every other constant vehicle 0's own float ((1, 1) is vehicle 0 bit for bit) - the load transfer's six
                   scalars and the caps' ratios among them: hypothesis k is capped by its own Pf_k, Pr_k
    log            states [W + 1, 3] = (vx, vy, r) float32, controls [W, 2] = (delta, pedal) float32; control j between
                   state j and state j + 1
    step           control_step(state, delta, pedal, c) with h = float32(dt / M) of THIS call's dt
    segment s      steps [s L, min((s + 1) L, W)): starts from the logged state s L, rolls open-loop; e = +0, then per step j
                     d = rolled - logged[j + 1];  e = fma(w0 dvx, dvx, e); e = fma(w1 dvy, dvy, e); e = fma(w2 dr, dr, e)
    score          E_k = e_0, then E_k + e_s in segment order (plain float32 adds)
    answer         errors [K], best = min_k pack_key(E_k, k): ties to the lower index, NaN and inf last

Also the float64 mirror of the same score (DynamicBicycleParams.predict_next_state's arithmetic over an array of
hypotheses) that the float32 restatement is compared with."""
from __future__ import annotations

import numpy as np

import dynamic_spec as ds
from acmpc_oracle import fma32, pick_best
from dynamic_spec import Settings

T = np.float32
MAX_LOG_STEPS = 512
MAX_HYPOTHESES = 65536


def hypothesis_block(vehicle0, front, rear):
    """The float64 block of a hypothesis: vehicle 0's with Df * front and Dr * rear."""
    coef = np.array(vehicle0, dtype=np.float64).ravel().copy()
    coef[ds.FIELDS.index("Df")] *= float(front)
    coef[ds.FIELDS.index("Dr")] *= float(rear)
    return coef


def hypothesis_constants(vehicle0, scales, dt, settings=Settings()):
    """constants(vehicle 0, settings, dt) with Pf, Pr replaced by the [K] float32 peaks of the hypotheses `scales` [K, 2]."""
    c = ds.constants(vehicle0, settings, dt)
    peaks = [ds.derived_constants(hypothesis_block(vehicle0, f, r)) for f, r in np.asarray(scales, dtype=np.float64)]
    c.k["Pf"] = np.array([p["Pf"] for p in peaks], dtype=T)
    c.k["Pr"] = np.array([p["Pr"] for p in peaks], dtype=T)
    return c


def segment_errors(vehicle0, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0), settings=Settings()):
    """e [S, K] float32: every segment's error of every hypothesis."""
    states, controls = np.asarray(states, dtype=T), np.asarray(controls, dtype=T)
    W, L = controls.shape[0], int(segment)
    assert states.shape == (W + 1, 3) and 1 <= W <= MAX_LOG_STEPS and 1 <= L <= W
    c = hypothesis_constants(vehicle0, scales, dt, settings)
    K = c.k["Pf"].size
    w = [T(float(v)) for v in weights]
    # the segments are independent: all of them advance together, [segments, K] arrays, the ragged last one leaving early
    starts = np.arange(0, W, L)
    S = starts.size
    st = tuple(np.zeros((S, K), dtype=T) for _ in range(3)) + tuple(np.repeat(states[starts, q][:, None], K, axis=1) for q in range(3))
    e = np.zeros((S, K), dtype=T)
    out = np.zeros((S, K), dtype=T)
    for i in range(L):
        if starts[-1] + i >= W:          # the last segment is over
            out[-1] = e[-1]
            starts, e, st = starts[:-1], e[:-1], tuple(a[:-1] for a in st)
            if starts.size == 0:
                break
        j = starts + i
        ones = np.ones((1, K), dtype=T)
        st = ds.control_step(st, controls[j, 0][:, None] * ones, controls[j, 1][:, None] * ones, c)
        with np.errstate(all="ignore"):
            for q in range(3):
                d = st[3 + q] - states[j + 1, q][:, None]
                e = fma32(w[q] * d, d, e)
    out[:starts.size] = e
    return out


def score(vehicle0, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0), settings=Settings()):
    """(errors [K] float32, best index) of the specification."""
    e = segment_errors(vehicle0, states, controls, dt, scales, segment, weights, settings)
    E = e[0].copy()
    with np.errstate(all="ignore"):
        for s in range(1, e.shape[0]):
            E = (E + e[s]).astype(T)
    return E, int(pick_best(E)[0])


def rollout_states(x0, U, vehicle, dt, settings=Settings()):
    """The six float32 states [B, n + 1, 6] of the control sequences U [B, n, 2] from the states x0 [B, 6], with no
    path: the float32 counterpart of DynamicBicycleParams.rollout (positions in the caller's frame, as given)."""
    c = ds.constants(vehicle, settings, dt)
    x0, U = np.asarray(x0, dtype=T), np.asarray(U, dtype=T)
    st = tuple(x0[:, q].copy() for q in range(6))
    out = [np.stack(st, axis=1)]
    for i in range(U.shape[1]):
        st = ds.control_step(st, U[:, i, 0], U[:, i, 1], c)
        out.append(np.stack(st, axis=1))
    return np.stack(out, axis=1)


# ---- the float64 mirror ---------------------------------------------------------------------------------------------
def mirror_step(params, Df, Dr, vx, vy, r, delta, pedal, dt):
    """DynamicBicycleParams.predict_next_state's velocity rows in float64 over arrays of (Df, Dr): the next (vx, vy, r), vx
    clipped at 0 as the reference's loop clips it."""
    p = params
    den = vx + 1e-3
    alpha_f = delta - np.arctan((r * p.lf + vy) / den)
    alpha_r = np.arctan((r * p.lr - vy) / den)

    def lateral(alpha, B, C, D, E, eps, F_z):
        ba = B * alpha
        return D * (1 + eps * F_z / p.F_z0) * F_z / p.F_z0 * np.sin(C * np.arctan(ba - E * (ba - np.arctan(ba))))

    F_fy = lateral(alpha_f, p.Bf, p.Cf, Df, p.Ef, p.epsf, p.F_zf)
    F_ry = lateral(alpha_r, p.Br, p.Cr, Dr, p.Er, p.epsr, p.F_zr)
    brake = p.Cb1 - p.Cb2 * vx - p.Cb3 * vx ** 2
    motor = p.Cm1 - p.Cm2 * vx - p.Cm3 * vx ** 2
    F_fric = -p.Cfric1 - p.Cfric2 * vx - p.Cfric3 * vx ** 2
    braking = min(0.0, pedal)
    F_rx = brake * (1 - p.brake_bias) * braking + motor * max(0.0, pedal)
    F_fx = brake * p.brake_bias * braking
    sd, cd = np.sin(delta), np.cos(delta)
    ax = (F_rx + F_fx + F_fric - F_fy * sd + p.mass * vy * r) / p.mass
    ay = (F_ry + F_fy * cd - p.mass * vx * r) / p.mass
    rd = (F_fy * p.lf * cd - F_ry * p.lr) / p.Iz
    return np.maximum(vx + ax * dt, 0.0), vy + ay * dt, r + rd * dt


def mirror_score(params, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0)):
    """errors [K] float64 of the same score with the float64 mirror as the step (one Euler step per control step)."""
    states, controls = np.asarray(states, dtype=np.float64), np.asarray(controls, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64)
    Df, Dr = params.Df * scales[:, 0], params.Dr * scales[:, 1]
    W, L = controls.shape[0], int(segment)
    E = np.zeros(scales.shape[0])
    for j0 in range(0, W, L):
        vx, vy, r = (np.full(scales.shape[0], states[j0, q]) for q in range(3))
        for j in range(j0, min(j0 + L, W)):
            vx, vy, r = mirror_step(params, Df, Dr, vx, vy, r, float(controls[j, 0]), float(controls[j, 1]), dt)
            for q, v in enumerate((vx, vy, r)):
                E = E + float(weights[q]) * (v - states[j + 1, q]) ** 2
    return E


# ---- logs -----------------------------------------------------------------------------------------------------------
def steering_log(plant, amplitude, steps=40, dt=0.05, vx0=30.0, pedal=0.2, noise=None, seed=0):
    """A log driven on `plant` (the float64 mirror): `steps` steps of `dt` from `vx0`, steering a sin(2 pi 0.5 t) + a / 2,
    rounded to float32; `noise` = sigmas on (vx, vy, r) added to the logged states.  (states [W + 1, 3], controls [W, 2])"""
    t = np.arange(steps) * dt
    controls = np.stack([amplitude * np.sin(2.0 * np.pi * 0.5 * t) + amplitude / 2.0, np.full(steps, pedal)], axis=1)
    controls = controls.astype(T)
    state = np.array([0.0, 0.0, 0.0, vx0, 0.0, 0.0])
    out = [state[3:].copy()]
    for u in controls.astype(np.float64):
        state = plant.predict_next_state(state, u, dt)[0]
        state[3] = max(state[3], 0.0)
        out.append(state[3:].copy())
    states = np.stack(out)
    if noise is not None:
        states = states + np.random.default_rng(seed).standard_normal(states.shape) * np.asarray(noise, dtype=np.float64)
    return states.astype(T), controls


def braking_log(plant, coupling=None, load_transfer=None, steps=40, dt=0.05, vx0=40.0, pedal=-1.0):
    """A straight-line braking log driven on `plant` (the float64 mirror under `coupling` and `load_transfer`): delta = 0, a
    constant pedal, rounded to float32.  (states [W + 1, 3], controls [W, 2])"""
    controls = np.stack([np.zeros(steps), np.full(steps, pedal)], axis=1).astype(T)
    traj = plant.rollout(np.array([0.0, 0.0, 0.0, vx0, 0.0, 0.0]), controls.astype(np.float64), dt, coupling=coupling,
                         load_transfer=load_transfer)
    return traj[:, 3:].astype(T), controls
