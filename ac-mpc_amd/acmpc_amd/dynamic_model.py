"""Mode D's vehicle: the six-state dynamic bicycle with Pacejka lateral tyre forces of the reference
(src/acmpc/control/dynamic_bicycle_model.py) - its parameters as the ABI's vehicle block, and a float64 host mirror of
its Euler step.

The reference's fitted drive, brake and friction maps are in newtons while its tyre forces come out in kilonewtons (mass
1.160 t, F_z0 = 3): taken literally, 20 m/s at pedal 0.5 becomes 145 m/s after one 50 ms step.  The coefficients are
therefore data ("Mode D"): `DynamicBicycleParams.reference(literal=True)` is the reference's block bit
for bit (the parity tests use it), `reference()` - the default vehicle - the same block with the nine longitudinal
coefficients in kilonewtons.

`stage_terms` and `objective_terms` are float64 mirrors of what acmpc_set_dynamics_terms and acmpc_set_dynamics_objective add
to a candidate's cost and violation - rates, rear slip; the progress made good and the excess over a speed ceiling - over
one trajectory of `DynamicBicycleParams.rollout`: what the float32 specification is measured against.

`surface_table` makes the per-waypoint grip scales of acmpc_set_surface from patches along the arc length ("wet from 40 m to
70 m"); `trace(..., surface=)` and the `grip=` argument of `predict_next_state` / `rollout` are its float64 mirror.

`actuator_coefficients` and `actuator_response` are the float64 mirror of acmpc_set_dynamics_actuator - first-order lags on the
steering and the pedal: the vehicle is driven on the mean of each actuator's response over the control step - and `actuator=` of
`rollout` and `trace` rolls a plan on that applied control while every cost line stays on the command.

`road_table` makes the per-waypoint rows (a_x, a_y, n_z) of acmpc_set_road from the grade and the bank of a path - or from patches
along the arc length ("6 % downhill from 40 m to 120 m"); `trace(..., road=)` and the `road=` argument of `predict_next_state` /
`rollout` are its float64 mirror."""
from __future__ import annotations

import dataclasses
from typing import Tuple

import numpy as np

# ABI order of the vehicle block (include/acmpc.h: acmpc_set_dynamics)
FIELDS = ("F_z0", "Bf", "Cf", "Df", "Ef", "epsf", "Br", "Cr", "Dr", "Er", "epsr", "mass", "Iz", "g", "lf", "lr",
          "brake_bias", "Cm1", "Cm2", "Cm3", "Cb1", "Cb2", "Cb3", "Cfric1", "Cfric2", "Cfric3")
LONGITUDINAL = ("Cm1", "Cm2", "Cm3", "Cb1", "Cb2", "Cb3", "Cfric1", "Cfric2", "Cfric3")

# what the reference's two curve_fit calls return (dynamic_bicycle_model.py:57-77; recorded in tests/golden/dynamic_bicycle.npz)
_FITTED = dict(Cm1=6634.272598708605, Cm2=-44.729701293631884, Cm3=1.789313054496502, Cb1=16807.528158800185,
               Cb2=-15.288256364280713, Cb3=0.3838603329874931, Cfric1=22.272598708604782, Cfric2=13.412206693199884,
               Cfric3=0.5405221569587206)


@dataclasses.dataclass
class DynamicBicycleParams:
    """The vehicle block, fields named as the reference names them (dynamic_bicycle_model.py:7-77)."""
    F_z0: float = 3.0
    Bf: float = 9.62
    Cf: float = 2.59
    Df: float = 4.120
    Ef: float = 1.0
    epsf: float = -0.0813
    Br: float = 8.62
    Cr: float = 2.65
    Dr: float = 4.617
    Er: float = 1.0
    epsr: float = -0.1263
    mass: float = 1.160
    Iz: float = 1.260
    g: float = 9.81
    lf: float = 1.51
    lr: float = 1.388
    brake_bias: float = 0.7
    Cm1: float = _FITTED["Cm1"] * 1e-3
    Cm2: float = _FITTED["Cm2"] * 1e-3
    Cm3: float = _FITTED["Cm3"] * 1e-3
    Cb1: float = _FITTED["Cb1"] * 1e-3
    Cb2: float = _FITTED["Cb2"] * 1e-3
    Cb3: float = _FITTED["Cb3"] * 1e-3
    Cfric1: float = _FITTED["Cfric1"] * 1e-3
    Cfric2: float = _FITTED["Cfric2"] * 1e-3
    Cfric3: float = _FITTED["Cfric3"] * 1e-3

    @classmethod
    def reference(cls, literal: bool = False) -> "DynamicBicycleParams":
        """The reference's vehicle: `literal=True` its numbers exactly as it holds them (longitudinal maps in N against
        tyre forces in kN); the default the kN-consistent block (the nine longitudinal coefficients times 1e-3)."""
        if literal:
            return cls(**_FITTED)
        return cls()

    @classmethod
    def from_coefficients(cls, coef) -> "DynamicBicycleParams":
        coef = np.asarray(coef, dtype=np.float64).ravel()
        if coef.size != len(FIELDS):
            raise ValueError("a vehicle block has %d values" % len(FIELDS))
        return cls(**{k: float(v) for k, v in zip(FIELDS, coef)})

    def with_grip(self, scale: float) -> "DynamicBicycleParams":
        """A copy on a road with `scale` times the grip: the Pacejka peak factors Df and Dr (proportional to the road's
        friction coefficient) scaled, nothing else.  The drive, brake and friction maps are left alone: without the tyre
        coupling (acmpc_set_dynamics_coupling, `coupling=` below) the longitudinal forces do not depend on the tyres' grip.
        With it each axle's drive and brake force is capped at rho times that axle's peak factor, which carries Df / Dr: the
        scale then limits braking and traction as well as cornering, and a saturated axle has no side force left.  The
        friction map is drag and stays as it is.  An ensemble of grips (DynamicSamplingSolver's `grip_ensemble`) scores every
        candidate on several such roads."""
        return self.with_axle_grip(scale, scale)

    def with_axle_grip(self, front: float, rear: float) -> "DynamicBicycleParams":
        """`with_grip` with a scale per axle: Df times `front`, Dr times `rear` (with_grip(s) is with_axle_grip(s, s)).
        What a hypothesis of the grip identification is (Engine.score_grips, GripEstimator)."""
        front, rear = float(front), float(rear)
        for scale in (front, rear):
            if not (np.isfinite(scale) and scale > 0.0):
                raise ValueError("a grip scale is finite and positive, not %r" % (scale,))
        return dataclasses.replace(self, Df=self.Df * front, Dr=self.Dr * rear)

    def coefficients(self) -> np.ndarray:
        """The ABI block: float64 [26] in FIELDS order (acmpc_set_dynamics)."""
        return np.array([getattr(self, k) for k in FIELDS], dtype=np.float64)

    @property
    def F_zf(self) -> float:
        return self.mass * self.g * self.lr / (self.lr + self.lf)

    @property
    def F_zr(self) -> float:
        return self.mass * self.g * self.lf / (self.lr + self.lf)

    @property
    def peak_front(self) -> float:
        """The front axle's peak factor Pf = Df (1 + epsf F_zf / F_z0) F_zf / F_z0: the most side force it gives."""
        return self.Df * (1 + self.epsf * self.F_zf / self.F_z0) * self.F_zf / self.F_z0

    @property
    def peak_rear(self) -> float:
        return self.Dr * (1 + self.epsr * self.F_zr / self.F_z0) * self.F_zr / self.F_z0

    def peak(self, axle: str, F_z: float) -> float:
        """The peak factor D (1 + eps F_z / F_z0) F_z / F_z0 of the axle 'f' or 'r' under the load F_z."""
        D, eps = (self.Df, self.epsf) if axle == "f" else (self.Dr, self.epsr)
        return D * (1 + eps * F_z / self.F_z0) * F_z / self.F_z0

    def downforce_at(self, vx: float, downforce) -> Tuple[float, float]:
        """(d_f, d_r), the downforce on the two axles at the speed `vx` under `downforce` = (k_f, k_r) or (k_f, k_r, v_sat =
        100) (acmpc_set_dynamics_downforce): k_a min(vx, v_sat)^2; None: (0, 0)."""
        if downforce is None:
            return 0.0, 0.0
        k_f, k_r, v_sat = _downforce(downforce)
        va = min(float(vx), v_sat)
        return k_f * va * va, k_r * va * va

    def loaded_axles(self, F_fx: float, F_rx: float, coupling, load_transfer, downforce=None, vx: float = 0.0) -> Tuple[float, float, float]:
        """(w, F_zf', F_zr') of the load transfer `load_transfer` = h_cg or (h_cg, w_frac = 0.9) for the longitudinal demands
        F_fx, F_rx (acmpc_set_dynamics_load_transfer, one explicit pass): the demands clipped at the STATIC caps of
        `coupling`, w = h_cg / (lf + lr) times their sum clipped at +-w_frac min(F_zf, F_zr) - the load moved to the rear,
        negative under braking - and the loads F_zf - w, F_zr + w.  With `downforce` (downforce_at's, at the speed `vx`) each
        axle's load has d_a on top of the static weight before anything moves: the caps are those AT THIS SPEED and the loads
        F_zf + d_f - w, F_zr + d_r + w.  load_transfer = None: nothing moves (w = 0)."""
        d_f, d_r = self.downforce_at(vx, downforce)
        if load_transfer is None:
            return 0.0, self.F_zf + d_f, self.F_zr + d_r
        h_cg, w_frac = (float(load_transfer), 0.9) if np.ndim(load_transfer) == 0 else (float(v) for v in load_transfer)
        rho_f, rho_r = _ratios(coupling)
        cap_f, cap_r = rho_f * self.peak("f", self.F_zf + d_f), rho_r * self.peak("r", self.F_zr + d_r)
        e_f = max(min(F_fx, cap_f), -cap_f)
        e_r = max(min(F_rx, cap_r), -cap_r)
        w_max = w_frac * min(self.F_zf, self.F_zr)
        w = max(min(h_cg / (self.lf + self.lr) * (e_f + e_r), w_max), -w_max)
        return w, self.F_zf + d_f - w, self.F_zr + d_r + w

    def predict_next_state(self, state, u, dt: float = 0.05, coupling=None, load_transfer=None,
                           downforce=None, grip=None, road=None) -> Tuple[np.ndarray, np.ndarray, list]:
        """One explicit Euler step in float64: state (X, Y, yaw, vx, vy, r), u = (delta, pedal) with the pedal in
        [-1, 1].  Returns (next_state, x_dot, [F_fy, F_ry, F_fx, F_rx]) like the reference; the caller clips vx >= 0
        (the reference's loop does, dynamic_bicycle_model.py:180; so do the kernels, inside the step).  `coupling` = rho
        or (rho_f, rho_r) is the tyre coupling of acmpc_set_dynamics_coupling in float64 (None: off; inf: none on that
        axle): per axle F_x is clipped at +-rho P and F_y scaled by sqrt(1 - (F_x / (rho P))^2); the returned forces are
        the coupled ones.  `load_transfer` = h_cg or (h_cg, w_frac) is the load transfer of
        acmpc_set_dynamics_load_transfer in float64 (None: off), the same one-pass formulation with the exact
        load-dependent peak: loaded_axles() gives each axle's load, which both the side force and the coupling's cap then
        take; the returned forces are the final ones.  `downforce` = (k_f, k_r) or (k_f, k_r, v_sat) is the downforce of
        acmpc_set_dynamics_downforce in float64 (None: off): the same one pass with k_a min(vx, v_sat)^2 on each axle's load
        under the load moved, and the exact load-dependent peak P(F_z + x); the force list holds the final forces.  `grip` =
        (mu_f, mu_r) is the surface's pair of this step (acmpc_set_surface; None: (1, 1)): the step of
        with_axle_grip(mu_f, mu_r) - both axles' peak factors scaled wherever the step reads them.  `road` = (a_x, a_y, n_z) is
        the road's row of this step (acmpc_set_road; None: (0, 0, 1)): both peak factors scaled by n_z as well - the normal load
        on a slope, taken linearly - and gravity's in-plane accelerations added to x_dot[3] and x_dot[4], along the body's axes."""
        if road is not None:
            a_x, a_y, n_z = (float(v) for v in road)
            mu_f, mu_r = (1.0, 1.0) if grip is None else (float(m) for m in grip)
            _, x_dot, forces = self.with_axle_grip(mu_f * n_z, mu_r * n_z).predict_next_state(
                state, u, dt, coupling=coupling, load_transfer=load_transfer, downforce=downforce)
            x_dot[3] += a_x
            x_dot[4] += a_y
            return np.asarray(state, dtype=np.float64) + x_dot * dt, x_dot, forces
        if grip is not None:
            return self.with_axle_grip(*grip).predict_next_state(state, u, dt, coupling=coupling, load_transfer=load_transfer,
                                                                 downforce=downforce)
        delta, pedal = float(u[0]), float(u[1])
        X, Y, yaw, vx, vy, r = (float(s) for s in state)
        den = vx + 1e-3
        alpha_f = delta - np.arctan((r * self.lf + vy) / den)
        alpha_r = np.arctan((r * self.lr - vy) / den)
        brake = self.Cb1 - self.Cb2 * vx - self.Cb3 * vx ** 2
        motor = self.Cm1 - self.Cm2 * vx - self.Cm3 * vx ** 2
        F_fric = -self.Cfric1 - self.Cfric2 * vx - self.Cfric3 * vx ** 2
        braking = min(0.0, pedal)
        F_rx = brake * (1 - self.brake_bias) * braking + motor * max(0.0, pedal)
        F_fx = brake * self.brake_bias * braking
        F_zf, F_zr = self.F_zf, self.F_zr
        if load_transfer is not None or downforce is not None:
            _, F_zf, F_zr = self.loaded_axles(F_fx, F_rx, coupling, load_transfer, downforce, vx)
        F_fy = self._lateral(alpha_f, self.Bf, self.Cf, self.Df, self.Ef, self.epsf, F_zf)
        F_ry = self._lateral(alpha_r, self.Br, self.Cr, self.Dr, self.Er, self.epsr, F_zr)
        if coupling is not None:
            rho_f, rho_r = _ratios(coupling)
            F_fx, F_fy = _couple(F_fx, F_fy, rho_f * self.peak("f", F_zf))
            F_rx, F_ry = _couple(F_rx, F_ry, rho_r * self.peak("r", F_zr))
        sd, cd = np.sin(delta), np.cos(delta)
        x_dot = np.array([
            vx * np.cos(yaw) - vy * np.sin(yaw),
            vx * np.sin(yaw) + vy * np.cos(yaw),
            r,
            (F_rx + F_fx + F_fric - F_fy * sd + self.mass * vy * r) / self.mass,
            (F_ry + F_fy * cd - self.mass * vx * r) / self.mass,
            (F_fy * self.lf * cd - F_ry * self.lr) / self.Iz,
        ])
        return np.asarray(state, dtype=np.float64) + x_dot * dt, x_dot, [F_fy, F_ry, F_fx, F_rx]

    def _lateral(self, alpha, B, C, D, E, eps, F_z):
        """Pacejka's magic formula with the load-dependent peak D (1 + eps F_z / F_z0) F_z / F_z0."""
        ba = B * alpha
        return D * (1 + eps * F_z / self.F_z0) * F_z / self.F_z0 * np.sin(C * np.arctan(ba - E * (ba - np.arctan(ba))))

    def rollout(self, state, U, dt: float = 0.05, substeps: int = 1, low_speed_blend=None, coupling=None,
                load_transfer=None, downforce=None, grip=None, actuator=None, road=None) -> np.ndarray:
        """The mirror over a control sequence U [n, 2] with vx clipped after every step: states [n + 1, 6].  `substeps`
        and `low_speed_blend` = (v_lo, v_hi) are the integration setting of acmpc_set_dynamics_integration in float64: a
        control step is `substeps` Euler steps of dt / substeps, and after each (vy, r) are blended towards the kinematic
        bicycle's r_k = vx tan(delta) / (lf + lr), vy_k = lr r_k by lam = clamp((vx - v_lo) / (v_hi - v_lo), 0, 1).
        `coupling`, `load_transfer`, `downforce`: predict_next_state's, in every sub-step.  `grip` = (mu_f, mu_r): one pair
        of grip scales for the whole roll (predict_next_state's; a surface table changes it per control step: trace()).
        `actuator` = (tau, a0) - tau = (tau_d, tau_p) in seconds, a0 = (a_d, a_p) the actuator positions at the start or None
        (U[0] then stands for them) - rolls on actuator_response's applied control instead of U (acmpc_set_dynamics_actuator).
        `road` = (a_x, a_y, n_z): one road row for the whole roll (predict_next_state's, in every sub-step; a road table changes
        it per control step: trace())."""
        if actuator is not None:
            tau, a0 = actuator
            applied, _ = actuator_response(U, a0, tau, dt)
            return self.rollout(state, applied, dt, substeps=substeps, low_speed_blend=low_speed_blend, coupling=coupling,
                                load_transfer=load_transfer, downforce=downforce, grip=grip, road=road)
        if grip is not None:
            return self.with_axle_grip(*grip).rollout(state, U, dt, substeps=substeps, low_speed_blend=low_speed_blend,
                                                      coupling=coupling, load_transfer=load_transfer, downforce=downforce, road=road)
        substeps = int(substeps)
        if substeps < 1:
            raise ValueError("substeps must be positive")
        h = dt / substeps
        out = [np.asarray(state, dtype=np.float64)]
        for u in np.asarray(U, dtype=np.float64):
            nxt = out[-1]
            for _ in range(substeps):
                nxt = self.predict_next_state(nxt, u, h, coupling=coupling, load_transfer=load_transfer, downforce=downforce,
                                              road=road)[0]
                nxt[3] = max(nxt[3], 0.0)
                if low_speed_blend is not None:
                    v_lo, v_hi = (float(v) for v in low_speed_blend)
                    r_k = nxt[3] * np.tan(u[0]) / (self.lf + self.lr)
                    lam = max(min((nxt[3] - v_lo) / (v_hi - v_lo), 1.0), 0.0)
                    nxt[4] = lam * nxt[4] + (1.0 - lam) * (r_k * self.lr)
                    nxt[5] = lam * nxt[5] + (1.0 - lam) * r_k
            out.append(nxt)
        return np.stack(out)


def _ratios(coupling) -> Tuple[float, float]:
    """(rho_f, rho_r) of a coupling setting: None is +inf on both axles, a scalar both axles'."""
    if coupling is None:
        return float("inf"), float("inf")
    rho_f, rho_r = (float(coupling),) * 2 if np.ndim(coupling) == 0 else (float(v) for v in coupling)
    return rho_f, rho_r


def _downforce(downforce) -> Tuple[float, float, float]:
    """(k_f, k_r, v_sat) of a downforce setting: a pair takes v_sat = 100 m/s."""
    values = tuple(float(v) for v in downforce)
    if len(values) not in (2, 3):
        raise ValueError("the downforce is (k_f, k_r) or (k_f, k_r, v_sat), not %r" % (downforce,))
    return values + (100.0,) if len(values) == 2 else values


def downforce_coefficients(cl_a: float, balance_front: float, air_density: float = 1.225, force_unit: float = 1000.0) -> Tuple[float, float]:
    """(k_f, k_r) of acmpc_set_dynamics_downforce for a car with the downforce area `cl_a` = C_L A (m^2), the fraction
    `balance_front` of it on the front axle, in air of `air_density` (kg/m^3): 1/2 rho C_L A split by the balance, in the
    vehicle block's force unit (`force_unit` newtons: 1000 for the kN of the reference block) per (m/s)^2."""
    cl_a, balance_front, air_density, force_unit = float(cl_a), float(balance_front), float(air_density), float(force_unit)
    if not (np.isfinite(cl_a) and cl_a >= 0.0):
        raise ValueError("cl_a is finite and >= 0 (lift is not modelled), not %r" % (cl_a,))
    if not 0.0 <= balance_front <= 1.0:
        raise ValueError("balance_front lies in [0, 1], not %r" % (balance_front,))
    if not (np.isfinite(air_density) and air_density > 0.0 and np.isfinite(force_unit) and force_unit > 0.0):
        raise ValueError("air_density and force_unit are finite and > 0")
    k = 0.5 * air_density * cl_a / force_unit
    return k * balance_front, k * (1.0 - balance_front)


def _couple(F_x: float, F_y: float, cap: float) -> Tuple[float, float]:
    """One axle on the friction ellipse: F_x clipped at +-cap, F_y scaled by what is left."""
    F_x = max(min(F_x, cap), -cap)
    u = F_x / cap
    return F_x, F_y * float(np.sqrt(1.0 - u * u))


def stage_terms(states, U, dt: float, u_prev, params: DynamicBicycleParams, rate_weight=(0.0, 0.0), rate_max=None,
                slip_weight: float = 0.0, slip_max=None) -> Tuple[float, float]:
    """The rate and slip terms of acmpc_set_dynamics_terms in float64 over `states` [n + 1, 6] = params.rollout(state, U, ...)
    and U [n, 2]: (E, extra_V) with E = 1/2 sum_i (w_d rd_i^2 + w_p rp_i^2 + w_s b_i^2) and extra_V the summed squared
    excesses over the limits (None: no limit), rd_i = (delta_i - delta_{i-1}) / dt, rp_i likewise - step 0 against
    `u_prev`, or a zero increment without one - and b_i = (r lr - vy) / (vx + 1e-3) on states[i + 1]."""
    U = np.asarray(U, dtype=np.float64)
    states = np.asarray(states, dtype=np.float64)
    first = U[0] if u_prev is None else np.asarray(u_prev, dtype=np.float64)
    rates = np.diff(np.concatenate([first[None], U]), axis=0) / dt
    b = (states[1:, 5] * params.lr - states[1:, 4]) / (states[1:, 3] + 1e-3)
    limits = [np.inf, np.inf] if rate_max is None else [np.inf if v is None else float(v) for v in rate_max]
    limits.append(np.inf if slip_max is None else float(slip_max))
    weights = (float(rate_weight[0]), float(rate_weight[1]), float(slip_weight))
    E, V = 0.0, 0.0
    for w, limit, a in zip(weights, limits, (rates[:, 0], rates[:, 1], b)):
        E += 0.5 * w * float(np.sum(a * a))
        V += float(np.sum(np.maximum(np.abs(a) - limit, 0.0) ** 2))
    return E, V


def objective_terms(states, U, table, progress_weight: float = 0.0, speed_ceiling=None, nn_window=None) -> Tuple[float, float]:
    """The progress and ceiling parts of acmpc_set_dynamics_objective in float64 over `states` [n + 1, 6] =
    params.rollout(state, U, ...) and the path `table` [7, n] (rows x, y, psi, kappa, ds, width, v): (s, extra_V).  s is the
    arc length made good at the last state - the polyline length up to its nearest waypoint j plus the along-track offset
    cos psi_j (X - x_j) + sin psi_j (Y - y_j); the cost's term is -progress_weight s, which the caller applies (`U` and
    `progress_weight` only say what the call is about: s does not depend on them).  extra_V is the summed squared excess
    of vx over scale * v_j + offset at every step's nearest waypoint (`speed_ceiling` a scale, a (scale, offset) pair or
    None: 0).  `nn_window` = (back, ahead) searches as the handle's window does, from waypoint 0; None: all waypoints."""
    states = np.asarray(states, dtype=np.float64)
    table = np.asarray(table, dtype=np.float64)
    x, y, psi, v = table[0], table[1], table[2], table[6]
    n = table.shape[1]
    arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    d2 = (states[1:, 0, None] - x[None, :]) ** 2 + (states[1:, 1, None] - y[None, :]) ** 2
    if nn_window is None:
        j = np.argmin(d2, axis=1)
    else:
        back, ahead = nn_window
        width = back + ahead + 1
        j = np.empty(len(d2), dtype=np.int64)
        prev = 0
        for i, row in enumerate(d2):
            first = min(max(prev - back, 0), max(n - width, 0))
            prev = j[i] = first + int(np.argmin(row[first:first + width]))
    last = j[-1]
    s = arc[last] + np.cos(psi[last]) * (states[-1, 0] - x[last]) + np.sin(psi[last]) * (states[-1, 1] - y[last])
    extra_V = 0.0
    if speed_ceiling is not None:
        scale, offset = (float(speed_ceiling), 0.0) if np.ndim(speed_ceiling) == 0 else (float(c) for c in speed_ceiling)
        extra_V = float(np.sum(np.maximum(states[1:, 3] - (scale * v[j] + offset), 0.0) ** 2))
    return float(s), extra_V


def clearance_terms(xy, obstacles, radii, weight: float = 0.0, margin: float = 0.0) -> Tuple[float, float]:
    """The obstacles' lines of acmpc_set_obstacles / acmpc_set_dynamics_clearance in float64 over `xy` [n, 2] - the
    positions after each control step, states[1:, :2] of params.rollout(state, U, ...) - `obstacles` [n, K, 2], where row i
    holds the discs at that same state, and `radii` [K] (each obstacle's plus the ego's): (cost, violation) with
    cost = 1/2 weight sum_ik max(R_k + margin - d_ik, 0)^2 and violation = sum_ik max(R_k - d_ik, 0)^2, d_ik the distance
    from the position to disc k's centre.  A NaN or infinite coordinate is a disc that does not exist at that step."""
    xy = np.asarray(xy, dtype=np.float64)
    obstacles = np.asarray(obstacles, dtype=np.float64)
    radii = np.asarray(radii, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(np.sum((xy[:, None, :] - obstacles) ** 2, axis=2))
        h = np.fmax(radii[None, :] - d, 0.0)
        g = np.fmax((radii[None, :] + float(margin)) - d, 0.0)
    return 0.5 * float(weight) * float(np.sum(g * g)), float(np.sum(h * h))


def predict_obstacles(position, velocity, n: int, dt: float) -> np.ndarray:
    """The constant-velocity table acmpc_set_obstacles takes: [n, K, 2], row i = position + velocity (i + 1) dt - where
    the K discs at `position` [K, 2] moving with `velocity` [K, 2] are when control step i has been taken."""
    position = np.asarray(position, dtype=np.float64).reshape(-1, 2)
    velocity = np.asarray(velocity, dtype=np.float64).reshape(-1, 2)
    t = (np.arange(int(n), dtype=np.float64) + 1.0) * float(dt)
    return position[None, :, :] + velocity[None, :, :] * t[:, None, None]


def surface_table(arc_length, patches) -> np.ndarray:
    """The table acmpc_set_surface takes for one path, [n, 2] float32 = (mu_f, mu_r) per waypoint, from `arc_length` [n] - the
    arc length of every waypoint (cumulative `ds` of the path table, in metres from the first) - and `patches`, a list of
    (s_from, s_to, mu) or (s_from, s_to, mu_f, mu_r): a waypoint with s_from <= s <= s_to takes the patch's scale(s), later
    patches override earlier ones, and a waypoint in no patch is 1.  Computed in float64, rounded once."""
    s = np.asarray(arc_length, dtype=np.float64).ravel()
    table = np.ones((s.size, 2), dtype=np.float64)
    for patch in patches:
        patch = tuple(float(v) for v in patch)
        if len(patch) not in (3, 4):
            raise ValueError("a patch is (s_from, s_to, mu) or (s_from, s_to, mu_f, mu_r), not %r" % (patch,))
        scales = patch[2:] * 2 if len(patch) == 3 else patch[2:]
        if not all(np.isfinite(m) and m > 0.0 for m in scales):
            raise ValueError("a grip scale is finite and positive, not %r" % (scales,))
        inside = (s >= patch[0]) & (s <= patch[1])
        table[inside, 0], table[inside, 1] = scales
    return table.astype(np.float32)


def road_table(grade, bank=None, g: float = 9.81, arc_length=None) -> np.ndarray:
    """The table acmpc_set_road takes for one path, [n, 3] float32 = (a_x, a_y, n_z) per waypoint, from `grade` [n] - theta, the
    road's slope along the path in radians, uphill positive - and `bank` [n] - beta, positive where the left side is lower (None:
    level): a_x = -g sin theta, a_y = g cos theta sin beta, n_z = cos theta cos beta, computed in float64 and rounded once each.
    With `arc_length` [n] (as surface_table's) `grade` is instead a list of patches (s_from, s_to, theta) or (s_from, s_to, theta,
    beta) - "6 % downhill from 40 m to 120 m" is (40, 120, -atan(0.06)) - later patches override earlier ones, a waypoint in no
    patch is level, and `bank` must be None.  |theta|, |beta| < pi / 2 (n_z > 0)."""
    if arc_length is not None:
        if bank is not None:
            raise ValueError("with arc_length the bank comes in the patches")
        s = np.asarray(arc_length, dtype=np.float64).ravel()
        theta, beta = np.zeros(s.size), np.zeros(s.size)
        for patch in grade:
            patch = tuple(float(v) for v in patch)
            if len(patch) not in (3, 4):
                raise ValueError("a patch is (s_from, s_to, theta) or (s_from, s_to, theta, beta), not %r" % (patch,))
            inside = (s >= patch[0]) & (s <= patch[1])
            theta[inside] = patch[2]
            beta[inside] = patch[3] if len(patch) == 4 else 0.0
    else:
        theta = np.asarray(grade, dtype=np.float64)
        beta = np.zeros_like(theta) if bank is None else np.asarray(bank, dtype=np.float64)
        if theta.ndim != 1 or beta.shape != theta.shape:
            raise ValueError("grade and bank are [n] each, not %r and %r" % (theta.shape, beta.shape))
    limit = np.pi / 2.0
    if not (np.all(np.isfinite(theta)) and np.all(np.isfinite(beta)) and np.all(np.abs(theta) < limit) and np.all(np.abs(beta) < limit)):
        raise ValueError("grade and bank are finite and within (-pi / 2, pi / 2)")
    g = float(g)
    rows = np.stack([-g * np.sin(theta), g * np.cos(theta) * np.sin(beta), np.cos(theta) * np.cos(beta)], axis=1)
    return rows.astype(np.float32)


def actuator_coefficients(tau, dt: float) -> Tuple[np.ndarray, np.ndarray]:
    """(k [2], m [2]) of acmpc_set_dynamics_actuator in float64 for tau = (tau_d, tau_p) seconds and the control step dt:
    k_c = exp(-dt / tau_c), what is left of an error after one control step, and m_c = (tau_c / dt)(1 - k_c), the mean of what is
    left over the step's interval; tau_c = 0 gives k_c = m_c = 0.  For tau_c > 0: 0 < k_c < m_c < 1."""
    tau = np.asarray(tau, dtype=np.float64).reshape(2)
    if not np.all(np.isfinite(tau) & (tau >= 0.0)):
        raise ValueError("tau_d, tau_p are finite and >= 0, not %r" % (tuple(tau),))
    k, m = np.zeros(2), np.zeros(2)
    on = tau > 0.0
    k[on] = np.exp(-float(dt) / tau[on])
    m[on] = (tau[on] / float(dt)) * (1.0 - k[on])
    return k, m


def actuator_response(U, a0, tau, dt: float) -> Tuple[np.ndarray, np.ndarray]:
    """The float64 mirror of the actuator lag over the commands U [n, 2] = (delta, pedal) from the positions a0 = (a_d, a_p)
    (None: U[0], so that the first step has no lag): per control step and channel e = u_i - a, applied_i = u_i - m e - what the
    vehicle is driven on during step i, the interval mean of the exact first-order response to the held command - and
    a = u_i - k e, the position at the step's end.  Returns (applied [n, 2], positions [n + 1, 2]), positions[0] = a0."""
    U = np.asarray(U, dtype=np.float64).reshape(-1, 2)
    k, m = actuator_coefficients(tau, dt)
    a = U[0].copy() if a0 is None else np.asarray(a0, dtype=np.float64).reshape(2).copy()
    applied, positions = np.empty_like(U), np.empty((U.shape[0] + 1, 2))
    positions[0] = a
    for i, u in enumerate(U):
        e = u - a
        applied[i] = u - m * e
        a = u - k * e
        positions[i + 1] = a
    return applied, positions


TRACE_HINGES = ("box", "corridor", "rate", "slip", "ceiling", "obstacles")   # what a step squares into V, in this order


def trace(params: DynamicBicycleParams, state, U, table, dt: float = 0.05, u_min=(-0.3, -1.0), u_max=(0.3, 1.0),
          margin: float = 0.0, wheelbase=None, nn_window=None, substeps: int = 1, low_speed_blend=None, coupling=None,
          load_transfer=None, downforce=None, u_prev=None, rate_max=None, slip_max=None, speed_ceiling=None, obstacles=None,
          radii=None, surface=None, actuator=None, road=None) -> dict:
    """The float64 mirror of Engine.trace_plans for one plan under one vehicle: `params.rollout(state, U, ...)` with the
    handle's step settings, and per control step - on the state after it, against its nearest waypoint j of `table` [7, n]
    (objective_terms' search: `nn_window` from waypoint 0, None: all) - what the cost lines see and the hinges they square
    into V, as stage_terms, objective_terms and clearance_terms define them: dict(states [n + 1, 6], j [n], e_y, e_psi, dv,
    dk [n], box [n, 2] = u - clip(u, u_min, u_max), corridor [n] = max(|e_y| - (width_j / 2 - margin), 0), rate [n, 2] and
    slip [n] = max(|.| - limit, 0) of stage_terms' rd, rp, b (step 0 against `u_prev`, or a zero increment; None: no limit, 0),
    ceiling [n] = max(vx - (scale v_j + offset), 0), obstacles [n, 8] = max(R_k - d_ik, 0) of clearance_terms (a NaN coordinate
    is a disc that is not there), V [n] the running sum of their squares, kink [n, 15] each hinge's distance from its kink).  `wheelbase` (default lf + lr) makes delta_ref =
    atan(wheelbase kappa_j).  `surface` [n, 2] = (mu_f, mu_r) per waypoint (acmpc_set_surface, surface_table): control step i
    is rolled with grip = surface[j_{i-1}], the nearest waypoint of the step before and waypoint 0 first - the scale lags the
    position by one control step, as on the device.  `actuator` = (tau, a0) (acmpc_set_dynamics_actuator, rollout's): the states
    are rolled on actuator_response's applied control; dk, the box and the rates stay on the command U.  `road` [n, 3] = (a_x,
    a_y, n_z) per waypoint (acmpc_set_road, road_table): control step i is rolled with road = road[j_{i-1}], the surface's lag."""
    U = np.asarray(U, dtype=np.float64)
    driven = U if actuator is None else actuator_response(U, actuator[1], actuator[0], dt)[0]
    table = np.asarray(table, dtype=np.float64)
    n = U.shape[0]
    x, y, psi, kappa, width, v = (table[row][:n] for row in (0, 1, 2, 3, 5, 6))
    L = params.lf + params.lr if wheelbase is None else float(wheelbase)
    step = dict(substeps=substeps, low_speed_blend=low_speed_blend, coupling=coupling, load_transfer=load_transfer,
                downforce=downforce)

    def nearest(pose, prev):
        d2 = (pose[0] - x) ** 2 + (pose[1] - y) ** 2
        if nn_window is None:
            return int(np.argmin(d2))
        back, ahead = nn_window
        span = back + ahead + 1
        first = min(max(prev - back, 0), max(n - span, 0))
        return first + int(np.argmin(d2[first:first + span]))

    j = np.empty(n, dtype=np.int64)
    if surface is None and road is None:
        states = params.rollout(state, driven, dt, **step)
        prev = 0
        for i in range(n):
            prev = j[i] = nearest(states[i + 1], prev)
    else:
        scales = np.ones((n, 2)) if surface is None else np.asarray(surface, dtype=np.float64)
        if scales.shape != (n, 2):
            raise ValueError("surface is [n, 2] = (mu_f, mu_r) per waypoint")
        rows = None if road is None else np.asarray(road, dtype=np.float64)
        if rows is not None and rows.shape != (n, 3):
            raise ValueError("road is [n, 3] = (a_x, a_y, n_z) per waypoint")
        rolled = [np.asarray(state, dtype=np.float64)]
        prev = 0
        for i in range(n):
            rolled.append(params.rollout(rolled[-1], driven[i:i + 1], dt, grip=scales[prev],
                                         road=None if rows is None else rows[prev], **step)[1])
            prev = j[i] = nearest(rolled[-1], prev)
        states = np.stack(rolled)
    after = states[1:]
    e_y = -np.sin(psi[j]) * (after[:, 0] - x[j]) + np.cos(psi[j]) * (after[:, 1] - y[j])
    e_psi = np.mod(after[:, 2] - psi[j] + np.pi, 2.0 * np.pi) - np.pi
    out = dict(states=states, j=j, e_y=e_y, e_psi=e_psi, dv=after[:, 3] - v[j], dk=U[:, 0] - np.arctan(L * kappa[j]))
    lo, hi = np.asarray(u_min, dtype=np.float64), np.asarray(u_max, dtype=np.float64)
    out["box"] = U - np.clip(U, lo, hi)
    # every other hinge is max(argument, 0): the arguments, in TRACE_HINGES' order behind the box's two
    first = U[0] if u_prev is None else np.asarray(u_prev, dtype=np.float64)
    rates = np.diff(np.concatenate([first[None], U]), axis=0) / dt
    limits = [np.inf, np.inf] if rate_max is None else [np.inf if m is None else float(m) for m in rate_max]
    b = (after[:, 5] * params.lr - after[:, 4]) / (after[:, 3] + 1e-3)
    over = np.full((n, 13), -np.inf)
    over[:, 0] = np.abs(e_y) - (width[j] / 2.0 - float(margin))
    over[:, 1:3] = np.abs(rates) - np.asarray(limits)[None, :]
    over[:, 3] = np.abs(b) - (np.inf if slip_max is None else float(slip_max))
    if speed_ceiling is not None:
        scale, offset = (float(speed_ceiling), 0.0) if np.ndim(speed_ceiling) == 0 else (float(c) for c in speed_ceiling)
        over[:, 4] = after[:, 3] - (scale * v[j] + offset)
    if obstacles is not None:
        discs = np.asarray(obstacles, dtype=np.float64)[:n]
        with np.errstate(invalid="ignore"):
            d = np.sqrt(np.sum((after[:, None, :2] - discs) ** 2, axis=2))
        gap = np.asarray(radii, dtype=np.float64)[None, :] - d
        over[:, 5:5 + discs.shape[1]] = np.where(np.isfinite(gap), gap, -np.inf)   # (a disc that is not there)
    hinge = np.maximum(over, 0.0)
    out.update(corridor=hinge[:, 0], rate=hinge[:, 1:3], slip=hinge[:, 3], ceiling=hinge[:, 4], obstacles=hinge[:, 5:])
    # how far every hinge's argument is from its kink (the box: from the nearer bound): where a float32 trace may differ in kind
    out["kink"] = np.concatenate([np.minimum(np.abs(U - lo), np.abs(U - hi)), np.abs(over)], axis=1)
    hinges = np.concatenate([out["box"], hinge], axis=1)
    out["V"] = np.cumsum(np.sum(hinges * hinges, axis=1))
    return out
