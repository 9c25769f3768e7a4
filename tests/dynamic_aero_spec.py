"""Mode D's aerodynamic downforce restated in NumPy ("Mode D, downforce"): dynamic_load_spec's step with
the downforce of the sub-step's incoming speed under the load moved, built from dynamic_spec's pieces, dynamic_load_spec's
constants and dynamic_coupling_spec's axle, and bit-identical to the aero kernels of csrc/acmpc_dynamic_aero.hip and
csrc/acmpc_identify.hip.  A helper of the tests, not a test file.

    aero = (k_f, k_r) or (k_f, k_r, v_sat = 100), each rounded to float32 once.  Per vehicle a1_a, a2_a are the load
    transfer's (dynamic_load_spec.constants); c_h = w_max = 0 while the load transfer is off.
    after F_rx, F_fx and before anything uses a peak, everything float32 in this order, nothing fused, min / max = minNum /
    maxNum; vx the step's incoming speed, Pf, Pr the peaks THIS step would otherwise use, rho the coupling's ratios (+inf: off):
      va   = fmin(vx, v_sat) ;  q = va * va
      d_f  = k_f * q ;  d_r = k_r * q
      psi_a = 1 + d_a * (a1_a + a2_a * d_a)                                       multiply, add, multiply, add
      Pf0  = Pf * psi_f ;  Pr0 = Pr * psi_r
      e_f  = fmax(fmin(F_fx, rho_f * Pf0), -(rho_f * Pf0)) ;  e_r likewise        the demands clipped at the caps AT THIS SPEED
      w    = c_h * (e_f + e_r) ;  w = fmax(fmin(w, w_max), -w_max)
      x_f  = d_f - w ;  x_r = d_r + w
      phi_a = 1 + x_a * (a1_a + a2_a * x_a)
      Pf'  = Pf * phi_f ;  Pr' = Pr * phi_r
      then the loaded step: the side forces on Pf', Pr', the coupling block on the ORIGINAL F_fx, F_rx with Pf', Pr'

`setting(ratio, load, aero)` takes dynamic_load_spec.setting's place as the OUTERMOST of the step-level settings; aero = None is
dynamic_load_spec.setting(ratio, load)."""
from __future__ import annotations

import contextlib

import numpy as np

import dynamic_coupling_spec as dcs
import dynamic_integration_spec as dis
import dynamic_load_spec as dls
import dynamic_spec as ds
import grip_spec as gs
from acmpc_oracle import fma32, pick_best, sincos_spec

T = np.float32
V_SAT = 100.0


def aero_setting(aero):
    """(k_f, k_r, v_sat) as float32, each rounded once; a pair takes v_sat = 100 m/s."""
    aero = tuple(float(v) for v in aero)
    assert len(aero) in (2, 3), "the downforce is (k_f, k_r) or (k_f, k_r, v_sat)"
    k_f, k_r, v_sat = (T(v) for v in (aero + (V_SAT,) if len(aero) == 2 else aero))
    assert np.isfinite(k_f) and k_f >= 0 and np.isfinite(k_r) and k_r >= 0 and np.isfinite(v_sat) and v_sat > 0
    return k_f, k_r, v_sat


def constants(vehicle, load, aero):
    """The load transfer's six float32 scalars of the vehicle block (c_h = w_max = 0 while `load` is None) and the downforce's
    three."""
    if load is None:
        k = dls.constants(vehicle, (0.0, 0.5))
        k["c_h"], k["w_max"] = T(0.0), T(0.0)
    else:
        k = dls.constants(vehicle, load)
    k["k_f"], k["k_r"], k["v_sat"] = aero_setting(aero)
    return k


def aero_peaks(vx, F_fx, F_rx, rho_f, rho_r, k):
    """(Pf', Pr', w, d_f, d_r) of one step: k holds Pf, Pr, the six scalars and the downforce's three."""
    with np.errstate(all="ignore"):
        va = np.fmin(vx, k["v_sat"])
        q = va * va
        d_f = k["k_f"] * q
        d_r = k["k_r"] * q
        psi_f = T(1.0) + d_f * (k["a1_f"] + k["a2_f"] * d_f)
        psi_r = T(1.0) + d_r * (k["a1_r"] + k["a2_r"] * d_r)
        cap_f = np.asarray(rho_f * (k["Pf"] * psi_f), dtype=T)
        cap_r = np.asarray(rho_r * (k["Pr"] * psi_r), dtype=T)
        e_f = np.fmax(np.fmin(F_fx, cap_f), -cap_f)
        e_r = np.fmax(np.fmin(F_rx, cap_r), -cap_r)
        w = k["c_h"] * (e_f + e_r)
        w = np.fmax(np.fmin(w, k["w_max"]), -k["w_max"])
        x_f = d_f - w
        x_r = d_r + w
        phi_f = T(1.0) + x_f * (k["a1_f"] + k["a2_f"] * x_f)
        phi_r = T(1.0) + x_r * (k["a1_r"] + k["a2_r"] * x_r)
        Pf = k["Pf"] * phi_f
        Pr = k["Pr"] * phi_r
    return tuple(np.asarray(a, dtype=T) for a in (Pf, Pr, w, d_f, d_r))


def aero_step(ratio, load, aero):
    """dynamic_load_spec's step - its lines - with aero_peaks in loaded_peaks' place.  k is what derived_constants gives INSIDE
    setting()."""
    rho_f, rho_r = dls.ratios(ratio)
    aero_setting(aero)

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
            Pf, Pr = aero_peaks(vx, F_fx, F_rx, rho_f, rho_r, k)[:2]
            bf = k["Bf"] * a_f
            yf = bf - k["Ef"] * (bf - ds.atan_spec(bf))
            F_fy = Pf * ds.sin_spec(k["Cf"] * ds.atan_spec(yf))
            br = k["Br"] * a_r
            yr = br - k["Er"] * (br - ds.atan_spec(br))
            F_ry = Pr * ds.sin_spec(k["Cr"] * ds.atan_spec(yr))
            F_fx, F_fy = dcs.couple_axle(F_fx, F_fy, rho_f, Pf)
            F_rx, F_ry = dcs.couple_axle(F_rx, F_ry, rho_r, Pr)
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
def setting(ratio, load, aero):
    """Inside the block dynamic_spec.dynamic_step is the aero step of (`ratio`, `load`, `aero`) and
    dynamic_spec.derived_constants carries the nine scalars of its vehicle.  aero = None: the block is
    dynamic_load_spec.setting(ratio, load)."""
    if aero is None:
        with dls.setting(ratio, load):
            yield
        return
    if ds.dynamic_step.__module__ != ds.__name__ or ds.derived_constants.__module__ != ds.__name__:
        raise RuntimeError("dynamic_aero_spec.setting() is the outermost of the step-level settings: before the integration's, "
                           "and in place of the load transfer's and the coupling's")
    saved = ds.dynamic_step, ds.derived_constants
    constants0 = ds.derived_constants

    def derived_constants(coef):
        k = constants0(coef)
        k.update(constants(coef, load, aero))
        return k

    ds.dynamic_step, ds.derived_constants = aero_step(ratio, load, aero), derived_constants
    try:
        yield
    finally:
        ds.dynamic_step, ds.derived_constants = saved


def rollout_states(ratio, load, aero, x0, U, vehicle, dt, substeps=1, low_speed_blend=None):
    """dynamic_load_spec.rollout_states - its lines - under (`ratio`, `load`, `aero`): the six float32 states [B, n + 1, 6], the
    float32 counterpart of DynamicBicycleParams.rollout(..., coupling=ratio, load_transfer=load, downforce=aero)."""
    with setting(ratio, load, aero):
        k = ds.derived_constants(vehicle)
        inv_L, h, blend = dis.inverse_wheelbase(vehicle), dis.step_size(dt, substeps), dis.blend_constants(low_speed_blend)
        x0, U = np.asarray(x0, dtype=T), np.asarray(U, dtype=T)
        st = tuple(x0[:, q].copy() for q in range(6))
        out = [np.stack(st, axis=1)]
        for i in range(U.shape[1]):
            st = dcs.fine_step(st, U[:, i, 0], U[:, i, 1], k, inv_L, h, substeps, blend)
            out.append(np.stack(st, axis=1))
        return np.stack(out, axis=1)


def segment_errors(ratio, load, aero, vehicle0, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0), substeps=1,
                   low_speed_blend=None):
    """dynamic_load_spec.segment_errors - its lines - under (`ratio`, `load`, `aero`): hypothesis k has its own Pf_k, Pr_k, the
    base vehicle's six scalars and the handle's downforce."""
    states, controls = np.asarray(states, dtype=T), np.asarray(controls, dtype=T)
    W, L = controls.shape[0], int(segment)
    assert states.shape == (W + 1, 3) and 1 <= W <= gs.MAX_LOG_STEPS and 1 <= L <= W
    inv_L, h, blend = dis.inverse_wheelbase(vehicle0), dis.step_size(dt, substeps), dis.blend_constants(low_speed_blend)
    w = [T(float(v)) for v in weights]
    starts = np.arange(0, W, L)
    S = starts.size
    with setting(ratio, load, aero):
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


def score(ratio, load, aero, vehicle0, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0), substeps=1,
          low_speed_blend=None):
    """(errors [K] float32, best index) of the identification under (`ratio`, `load`, `aero`) (grip_spec.score's sum and pick)."""
    e = segment_errors(ratio, load, aero, vehicle0, states, controls, dt, scales, segment, weights, substeps, low_speed_blend)
    E = e[0].copy()
    with np.errstate(all="ignore"):
        for s in range(1, e.shape[0]):
            E = (E + e[s]).astype(T)
    return E, int(pick_best(E)[0])
