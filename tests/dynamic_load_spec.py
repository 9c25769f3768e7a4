"""Mode D's longitudinal load transfer restated in NumPy ("Mode D, load transfer"): dynamic_spec's Euler
step with the loaded peaks and the friction-ellipse block between its longitudinal forces and its accelerations, built from
dynamic_spec's pieces (atan_spec, sin_spec, sincos_spec, derived_constants) and dynamic_coupling_spec's axle, and bit-identical
to the loaded kernels of csrc/acmpc_dynamic_loaded.hip and csrc/acmpc_identify.hip.  A helper of the tests, not a test file.

    setting = (h_cg, w_frac), float64.  Per vehicle the host derives in float64, each rounded to float32 once:
      c_h   = h_cg / (lf + lr)
      w_max = w_frac * min(F_zf, F_zr)            F_zf = mass g lr / (lf + lr), F_zr = mass g lf / (lf + lr)
      e_a   = eps_a / F_z0 ;  N_a = F_za + e_a F_za^2 ;  a1_a = (1 + 2 e_a F_za) / N_a ;  a2_a = e_a / N_a       a = f, r
    after F_rx, F_fx and before anything uses a peak, everything float32 in this order, nothing fused, min / max = minNum /
    maxNum; Pf, Pr the peaks THIS step would otherwise use (k["Pf"], k["Pr"]), rho the coupling's ratios (+inf: off):
      e_f  = fmax(fmin(F_fx, rho_f * Pf), -(rho_f * Pf)) ;  e_r likewise          the demands clipped at the STATIC caps
      w    = c_h * (e_f + e_r) ;  w = fmax(fmin(w, w_max), -w_max)                the load moved to the rear
      x_f  = -w ;  x_r = w
      phi_a = 1 + x_a * (a1_a + a2_a * x_a)                                       multiply, add, multiply, add
      Pf'  = Pf * phi_f ;  Pr' = Pr * phi_r
      F_fy = Pf' * sin_spec(Cf * atan_spec(y_f)) ;  F_ry likewise
      the coupling block on the ORIGINAL F_fx, F_rx with Pf', Pr' in place of Pf, Pr

`setting(ratio, load)` swaps dynamic_spec.dynamic_step and dynamic_spec.derived_constants (which then carries the six scalars of
the vehicle it is given) for the duration of a `with` block.  It takes the place of dynamic_coupling_spec.setting as the
OUTERMOST of the step-level settings: dynamic_integration_spec.setting() entered inside it takes the loaded step as its
sub-step; entered the other way round it is refused.  load = None is dynamic_coupling_spec.setting(ratio)."""
from __future__ import annotations

import contextlib

import numpy as np

import dynamic_coupling_spec as dcs
import dynamic_integration_spec as dis
import dynamic_spec as ds
import grip_spec as gs
from acmpc_oracle import fma32, pick_best, sincos_spec

T = np.float32
KEYS = ("c_h", "w_max", "a1_f", "a2_f", "a1_r", "a2_r")


def load_setting(load):
    """(h_cg, w_frac) as two floats; a scalar is the height with w_frac = 0.9."""
    h_cg, w_frac = (load, 0.9) if np.ndim(load) == 0 else tuple(load)
    h_cg, w_frac = float(h_cg), float(w_frac)
    assert np.isfinite(h_cg) and h_cg >= 0.0 and 0.0 < w_frac < 1.0, "h_cg >= 0 and finite, 0 < w_frac < 1"
    return h_cg, w_frac


def constants64(vehicle, load):
    """The six scalars of the vehicle block `vehicle` under `load` in float64, in KEYS' order."""
    h_cg, w_frac = load_setting(load)
    v = dict(zip(ds.FIELDS, (float(x) for x in vehicle)))
    L = v["lf"] + v["lr"]
    F_z = (v["mass"] * v["g"] * v["lr"] / (v["lr"] + v["lf"]), v["mass"] * v["g"] * v["lf"] / (v["lr"] + v["lf"]))
    out = [h_cg / L, w_frac * min(F_z)]
    for F, eps in zip(F_z, (v["epsf"], v["epsr"])):
        e = eps / v["F_z0"]
        N = F + e * F * F
        out += [(1 + 2 * e * F) / N, e / N]
    return dict(zip(KEYS, out))


def constants(vehicle, load):
    """The same as the float32 the kernels get, each rounded once."""
    return {key: T(x) for key, x in constants64(vehicle, load).items()}


def ratios(ratio):
    """dynamic_coupling_spec.ratios, with None (the coupling off) as +inf on both axles."""
    return (T(np.inf), T(np.inf)) if ratio is None else dcs.ratios(ratio)


def loaded_peaks(F_fx, F_rx, rho_f, rho_r, k):
    """(Pf', Pr', w) of one step: k holds Pf, Pr and the six scalars."""
    with np.errstate(all="ignore"):
        cap_f = np.asarray(rho_f * k["Pf"], dtype=T)
        cap_r = np.asarray(rho_r * k["Pr"], dtype=T)
        e_f = np.fmax(np.fmin(F_fx, cap_f), -cap_f)
        e_r = np.fmax(np.fmin(F_rx, cap_r), -cap_r)
        w = k["c_h"] * (e_f + e_r)
        w = np.fmax(np.fmin(w, k["w_max"]), -k["w_max"])
        x_f, x_r = -w, w
        phi_f = T(1.0) + x_f * (k["a1_f"] + k["a2_f"] * x_f)
        phi_r = T(1.0) + x_r * (k["a1_r"] + k["a2_r"] * x_r)
        Pf = k["Pf"] * phi_f
        Pr = k["Pr"] * phi_r
    return np.asarray(Pf, dtype=T), np.asarray(Pr, dtype=T), np.asarray(w, dtype=T)


def couple_axle(F_x, F_y, rho, P):
    """dynamic_coupling_spec.couple_axle with a peak per element."""
    return dcs.couple_axle(F_x, F_y, rho, P)


def loaded_step(ratio, load):
    """dynamic_spec.dynamic_step - its lines - with the load transfer and the coupling block of (`ratio`, `load`).  k is
    what derived_constants gives INSIDE setting(): the vehicle's floats and its six scalars."""
    rho_f, rho_r = ratios(ratio)
    load_setting(load)

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
            vx2 = vx * vx
            F_fric = (k["fric0"] - k["Cfric2"] * vx) - k["Cfric3"] * vx2
            brake = (k["Cb1"] - k["Cb2"] * vx) - k["Cb3"] * vx2
            motor = (k["Cm1"] - k["Cm2"] * vx) - k["Cm3"] * vx2
            p_neg = np.fmin(pedal, T(0.0))
            p_pos = np.fmax(pedal, T(0.0))
            F_rx = (brake * k["bias_rear"]) * p_neg + motor * p_pos
            F_fx = (brake * k["bias_front"]) * p_neg
            Pf, Pr, _ = loaded_peaks(F_fx, F_rx, rho_f, rho_r, k)
            bf = k["Bf"] * a_f
            yf = bf - k["Ef"] * (bf - ds.atan_spec(bf))
            F_fy = Pf * ds.sin_spec(k["Cf"] * ds.atan_spec(yf))
            br = k["Br"] * a_r
            yr = br - k["Er"] * (br - ds.atan_spec(br))
            F_ry = Pr * ds.sin_spec(k["Cr"] * ds.atan_spec(yr))
            F_fx, F_fy = couple_axle(F_fx, F_fy, rho_f, Pf)
            F_rx, F_ry = couple_axle(F_rx, F_ry, rho_r, Pr)
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
def setting(ratio, load):
    """Inside the block dynamic_spec.dynamic_step is the loaded step of (`ratio`, `load`) and dynamic_spec.derived_constants
    carries the six scalars of its vehicle, for every restatement that looks them up in that module.  load = None: the block
    is dynamic_coupling_spec.setting(ratio)."""
    if load is None:
        with dcs.setting(ratio):
            yield
        return
    if ds.dynamic_step.__module__ != ds.__name__ or ds.derived_constants.__module__ != ds.__name__:
        raise RuntimeError("dynamic_load_spec.setting() is the outermost of the step-level settings: before the integration's, "
                           "and in place of the coupling's")
    saved = ds.dynamic_step, ds.derived_constants
    constants0 = ds.derived_constants

    def derived_constants(coef):
        k = constants0(coef)
        k.update(constants(coef, load))
        return k

    ds.dynamic_step, ds.derived_constants = loaded_step(ratio, load), derived_constants
    try:
        yield
    finally:
        ds.dynamic_step, ds.derived_constants = saved


def rollout_states(ratio, load, x0, U, vehicle, dt, substeps=1, low_speed_blend=None):
    """dynamic_coupling_spec.rollout_states - its lines - under (`ratio`, `load`): the six float32 states [B, n + 1, 6], the
    float32 counterpart of DynamicBicycleParams.rollout(..., coupling=ratio, load_transfer=load)."""
    with setting(ratio, load):
        k = ds.derived_constants(vehicle)
        inv_L, h, blend = dis.inverse_wheelbase(vehicle), dis.step_size(dt, substeps), dis.blend_constants(low_speed_blend)
        x0, U = np.asarray(x0, dtype=T), np.asarray(U, dtype=T)
        st = tuple(x0[:, q].copy() for q in range(6))
        out = [np.stack(st, axis=1)]
        for i in range(U.shape[1]):
            st = dcs.fine_step(st, U[:, i, 0], U[:, i, 1], k, inv_L, h, substeps, blend)
            out.append(np.stack(st, axis=1))
        return np.stack(out, axis=1)


def segment_errors(ratio, load, vehicle0, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0), substeps=1,
                   low_speed_blend=None):
    """dynamic_coupling_spec.segment_errors - its lines - under (`ratio`, `load`): hypothesis k has its own Pf_k, Pr_k and the
    base vehicle's six scalars."""
    states, controls = np.asarray(states, dtype=T), np.asarray(controls, dtype=T)
    W, L = controls.shape[0], int(segment)
    assert states.shape == (W + 1, 3) and 1 <= W <= gs.MAX_LOG_STEPS and 1 <= L <= W
    inv_L, h, blend = dis.inverse_wheelbase(vehicle0), dis.step_size(dt, substeps), dis.blend_constants(low_speed_blend)
    w = [T(float(v)) for v in weights]
    starts = np.arange(0, W, L)
    S = starts.size
    with setting(ratio, load):
        k = gs.hypothesis_constants(vehicle0, scales)
        K = k["Pf"].size
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
            st = dcs.fine_step(st, controls[j, 0][:, None] * ones, controls[j, 1][:, None] * ones, k, inv_L, h, substeps, blend)
            with np.errstate(all="ignore"):
                for q in range(3):
                    d = st[3 + q] - states[j + 1, q][:, None]
                    e = fma32(w[q] * d, d, e)
    out[:starts.size] = e
    return out


def score(ratio, load, vehicle0, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0), substeps=1,
          low_speed_blend=None):
    """(errors [K] float32, best index) of the identification under (`ratio`, `load`) (grip_spec.score's sum and pick)."""
    e = segment_errors(ratio, load, vehicle0, states, controls, dt, scales, segment, weights, substeps, low_speed_blend)
    E = e[0].copy()
    with np.errstate(all="ignore"):
        for s in range(1, e.shape[0]):
            E = (E + e[s]).astype(T)
    return E, int(pick_best(E)[0])


def braking_log(plant, coupling, load, steps=40, dt=0.05, vx0=40.0, pedal=-1.0):
    """dynamic_coupling_spec.braking_log on the loaded mirror: (states [W + 1, 3], controls [W, 2]) as float32."""
    controls = np.stack([np.zeros(steps), np.full(steps, pedal)], axis=1).astype(T)
    traj = plant.rollout(np.array([0.0, 0.0, 0.0, vx0, 0.0, 0.0]), controls.astype(np.float64), dt, coupling=coupling,
                         load_transfer=load)
    return traj[:, 3:].astype(T), controls
