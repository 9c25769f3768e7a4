"""`DynamicSamplingSolver`: the sampling controller with mode D's vehicle - candidates (delta, pedal) rolled through the
dynamic (Pacejka) bicycle on the GPU (csrc/acmpc_dynamic.hip), scored with mode T's nearest-waypoint cost, the cheapest
kept (`acmpc_optimize`: sample -> rollout -> finalize per round).  The seam is ControlSolver's: `solve(state, path) ->
obj` with `obj.x` laid out `[x_0 .. x_n ; u_0 .. u_{n-1}]` (x = (X, Y, yaw), u = (delta, pedal)) and `obj.info.status`.

Optional config keys, as sampling_solver.py reads them: `n_candidates`, `sampling_rounds`, `sampling_sigma` (delta rad,
pedal), `sampling_seed`, `sampling_update` ("argmin", the default: a round recentres on its winner; or "softmin": on the
softmin-weighted mean of its candidates, MPPI's update, with the winner kept as candidate 1), `softmin_lambda` (default
1.0), `w_bound`, `nn_window`, `rollout_dt`; the weights `step_cost` (e_y, e_psi, -), `r_term` (speed
error, steering against delta_ref), `final_cost`; the input box `u_min` / `u_max` (default delta +-0.3 rad, pedal +-1).
The warm start is the previous plan shifted by one step (`warm_start(steps)`: by that many).

Plan states (acmpc_trace_plans): `plan_states: True` (default off) adds `obj.states` [n + 1, 6] = (X, Y, yaw, vx, vy, r) - the
accepted plan re-rolled on the device under vehicle 0 by the arithmetic that scored it, so the speed the plan reaches at every
step is the float32 one the GPU saw - from one more call per solve; `solver.trace()` is the full trace of the last accepted plan
(or of a given one) under every vehicle: the states, each vehicle's cost and violation, and per step what every limit saw
(Engine.trace_plans) - which limit made a plan infeasible, at which step, and where the low-grip member of an ensemble goes.

Robust scoring (acmpc_set_dynamics_ensemble): `vehicle_ensemble` - a list of DynamicBicycleParams or 26-double blocks -
or `grip_ensemble` - grip scales, each giving `params.with_grip(scale)` - scores every candidate under each vehicle;
`ensemble_weights` (positive, default equal) and `ensemble_reduce` ("mean", the default, or "max": the worst case) say
how the costs combine.  The two ensemble keys are mutually exclusive; with neither, the solver scores the one vehicle
`params` (acmpc_set_dynamics).

Integration (acmpc_set_dynamics_integration): `rollout_substeps` (default 1) Euler steps per control step and
`low_speed_blend` (default None, or (v_lo, v_hi) m/s: below v_hi the lateral velocity and the yaw rate go over to the
kinematic bicycle's).  The single step is unstable below about 7.5 m/s and chatters up to about 12: set
`rollout_substeps: 4, low_speed_blend: (3, 5)` whenever a plan can fall below that (a hairpin, a pit lane, a start).

Rate and slip terms (acmpc_set_dynamics_terms): `rate_cost` = (delta, pedal) weights of the squared control rates (per
second), `rate_limit` = their limits (None, or a pair whose members may be None), `slip_cost` / `slip_limit` the same for
the rear slip ratio (r lr - vy) / vx.  A candidate over a limit is infeasible, as one outside the input box is.  Step 0's
rate is taken against the control applied before the plan: `solve(..., previous_control=)`, by default the first control
of the last accepted plan - what a caller that applies the plans has just applied; none on the first solve.

Objective (acmpc_set_dynamics_objective): `progress_cost` (cost units per metre, default 0) rewards the arc length made
good at the end of the plan, the minimum-time objective, and `speed_ceiling` - a scale, or (scale, offset), default None -
makes a candidate infeasible wherever vx > scale * v_ref + offset.  To drive at the grip limit instead of tracking the
kinematic profile: `r_term` = (0, .), a `progress_cost`, the profile as the ceiling (scale = sqrt(tyre a_y / profile a_y))
and a `slip_limit`.  Costs may then be negative; a solve fails only on a non-finite one, as before.

Tyre coupling (acmpc_set_dynamics_coupling): `tyre_coupling` - a ratio rho, or (rho_f, rho_r), default None - clips each
axle's drive and brake force at rho times that axle's lateral peak and scales its side force by what the friction ellipse
leaves.  Without it the brake map asks the tyres for more than they have and grip scales do not reach braking; with it
`grip_ensemble` members and `grip_adapt` hypotheses brake and accelerate as their grip allows.  rho near 1.

Load transfer (acmpc_set_dynamics_load_transfer): `load_transfer` - the height of the centre of gravity, or (h_cg, w_frac),
default None - lets each axle's load, and with it its Pacejka peak and its coupling cap, follow the longitudinal tyre force:
under braking the front axle gains grip and the rear loses it.  Beside `tyre_coupling` it moves the braking limit (about 10 %
more deceleration on the reference vehicle at h_cg = 0.35) and takes rear side force from a plan that turns in on the brakes.

Obstacles (acmpc_set_obstacles, acmpc_set_dynamics_clearance): `solve(..., obstacles=(positions [n, K, 2], radii [K]))` - up
to 8 discs with a position per control step (row i at time (i + 1) dt; dynamic_model.predict_obstacles makes the
constant-velocity table), each radius with the ego's folded in - makes a candidate that enters a disc infeasible, as one
that leaves the corridor is; `clearance_cost` / `clearance_margin` (default 0) add 0.5 cost depth^2 inside the margin round
each disc.  An opponent car is two or three discs along its length.

Downforce (acmpc_set_dynamics_downforce): `downforce` - (k_f, k_r) or (k_f, k_r, v_sat), default None, v_sat 100 m/s - lets each
axle's load grow with vx^2 (dynamic_model.downforce_coefficients gives the pair from C_L A and the aero balance): the peaks and
the coupling caps are those the tyres have at the speed driven, 29 % more at 200 km/h on the reference vehicle with C_L A = 3.

Surface (acmpc_set_surface): `solve(..., surface=grip)` - [n, 2] = (mu_f, mu_r) per waypoint of this solve's path, or [n]: one
scale for both axles (dynamic_model.surface_table makes one from "wet from 40 m to 70 m") - scales each axle's peak factor by
the value at the waypoint a candidate is at: a damp braking zone or a cold sector changes the plan where it lies, not the whole
horizon as a low-grip ensemble member does.  A control step is driven on the scales of the waypoint the candidate was nearest to
one step before.  None: no table (a table set by an earlier solve is cleared).  `trace()` re-rolls under the same table.

Actuator lag (acmpc_set_dynamics_actuator, acmpc_set_actuator_state): `actuator_lag` - (tau_d, tau_p), the time constants in
seconds of the steering rack and the pedal actuator, default None - rolls every candidate on the first-order response to its
commands (the mean of that response over each control step), so that a plan turns in and comes off the brake as early as the
actuators need; the input box, dk, the rates and the controls returned stay commands.  `solve(..., actuator_state=(a_d, a_p))`
gives the measured positions at the start of the plan; when it is left out the solver keeps its own float64 estimate
(`solver.actuator_state`): the estimate of the previous solve - at first `previous_control`, or the last plan's first control -
advanced through the first `warm_steps` controls of the last accepted plan (dynamic_model.actuator_response); before there is a
plan, `previous_control`, or none (the first command then stands for the positions).  `trace()` re-rolls under the same lag and
positions.  A dead time is not modelled: roll the start state forward under the controls already sent.

Road (acmpc_set_road): `solve(..., road=rows)` - [n, 3] = (a_x, a_y, n_z) per waypoint of this solve's path
(dynamic_model.road_table makes one from the path's grade and bank, or from "6 % downhill from 40 m to 120 m") - adds gravity's
in-plane acceleration to every candidate's step where it is on the path and scales the tyres' peaks by the normal load's factor:
a downhill braking zone is planned with the deceleration that is there, a banked corner with the speed it carries.  The row lags
the position by one control step, as the surface's scales do.  None: a level road (a table set by an earlier solve is cleared).

Grip adaptation (acmpc_score_grips, GripEstimator): `grip_adapt` - a dict, off by default - lets the solver find the road's
grip from its own driving instead of being told an ensemble.  Every solve logs (state, the control applied since the
previous solve - `previous_control`, else the last accepted plan's first control), scores a grid of grip hypotheses
against the last `window` transitions, and when an ACCEPTED estimate (GripEstimator's rule) has moved by at least one
grid step, scores from then on under `set_dynamics_ensemble([params.with_axle_grip(f b, r b) for b in bracket],
reduce="mean")`.  Keys: `grid` (default 0.3 .. 1.5 step 0.05), `axles` ("tied" or "split"), `window` (40), `min_window`
(10), `segment` (1), `bracket` (default (0.8, 1.2)), `prior` (grip scales scored under until the first accepted estimate,
default (1.0,): the nominal vehicle), `log_dt` (default `rollout_dt`: the period at which solve is called).  Mutually
exclusive with `vehicle_ensemble` / `grip_ensemble`.  `solver.grip` is the current estimate."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np

from . import _capi
from .dynamic_model import DynamicBicycleParams, actuator_coefficients, actuator_response
from .grip_estimator import GripEstimator

SOLVED = "solved"
DEFAULT_CANDIDATES = 16384
DEFAULT_ROUNDS = 2
DEFAULT_SIGMA = (0.05, 0.3)
DEFAULT_U_MIN = (-0.3, -1.0)
DEFAULT_U_MAX = (0.3, 1.0)
SAMPLING_UPDATES = ("argmin", "softmin")
GRIP_ADAPT_KEYS = ("grid", "axles", "window", "min_window", "segment", "bracket", "prior", "log_dt")
DEFAULT_BRACKET = (0.8, 1.2)
DEFAULT_PRIOR = (1.0,)


def grip_adaptation(config: Dict) -> Optional[Dict]:
    """The checked `grip_adapt` setting of a config (None: off): ValueError with an ensemble key beside it, for an unknown
    key, or for a bracket / prior that is not 1 .. MAX_VEHICLES finite positive scales."""
    adapt = config.get("grip_adapt")
    if adapt is None:
        return None
    for key in ("vehicle_ensemble", "grip_ensemble", "ensemble_weights", "ensemble_reduce"):
        if config.get(key) is not None:
            raise ValueError("grip_adapt and %s are mutually exclusive" % key)
    adapt = dict(adapt)
    unknown = sorted(set(adapt) - set(GRIP_ADAPT_KEYS))
    if unknown:
        raise ValueError("unknown grip_adapt key(s) %s" % ", ".join(unknown))
    for key, default in (("bracket", DEFAULT_BRACKET), ("prior", DEFAULT_PRIOR)):
        scales = tuple(float(v) for v in adapt.get(key, default))
        if not 1 <= len(scales) <= _capi.MAX_VEHICLES or not all(np.isfinite(v) and v > 0.0 for v in scales):
            raise ValueError("grip_adapt %s is 1 .. %d finite, positive scales, not %r" % (key, _capi.MAX_VEHICLES, scales))
        adapt[key] = scales
    return adapt


def ensemble_vehicles(config: Dict, params: DynamicBicycleParams) -> Optional[list]:
    """The vehicles a config asks to score under (`vehicle_ensemble` or `grip_ensemble`), or None for `params` alone."""
    has_vehicles, has_grips = config.get("vehicle_ensemble") is not None, config.get("grip_ensemble") is not None
    if has_vehicles and has_grips:
        raise ValueError("vehicle_ensemble and grip_ensemble are mutually exclusive")
    if not has_vehicles and not has_grips:
        for key in ("ensemble_weights", "ensemble_reduce"):
            if config.get(key) is not None:
                raise ValueError("%s needs vehicle_ensemble or grip_ensemble" % key)
        return None
    if config.get("ensemble_reduce", "mean") not in _capi.ENSEMBLE_REDUCE:
        raise ValueError("ensemble_reduce is 'mean' or 'max', not %r" % (config.get("ensemble_reduce"),))
    if has_grips:
        vehicles = [params.with_grip(g) for g in config["grip_ensemble"]]
    else:
        vehicles = [v if isinstance(v, DynamicBicycleParams) else DynamicBicycleParams.from_coefficients(v)
                    for v in config["vehicle_ensemble"]]
    if not 1 <= len(vehicles) <= _capi.MAX_VEHICLES:
        raise ValueError("an ensemble has 1 .. %d vehicles, not %d" % (_capi.MAX_VEHICLES, len(vehicles)))
    weights = config.get("ensemble_weights")
    if weights is not None and len(weights) != len(vehicles):
        raise ValueError("%d ensemble_weights for %d vehicles" % (len(weights), len(vehicles)))
    return vehicles


class DynamicSamplingSolver:
    def __init__(self, config: Dict, params: Optional[DynamicBicycleParams] = None, device: int = -1):
        self._n = int(config["horizon"]) - 1
        self._N = int(config.get("n_candidates", DEFAULT_CANDIDATES))
        self._rounds = int(config.get("sampling_rounds", DEFAULT_ROUNDS))
        self._sigma = np.asarray(config.get("sampling_sigma", DEFAULT_SIGMA), dtype=np.float64)
        self._seed = int(config.get("sampling_seed", 0))
        self._dt = float(config.get("rollout_dt", 0.05))
        self._params = params if params is not None else DynamicBicycleParams.reference()
        adapt = grip_adaptation(config)                      # (a config error raises before any handle exists)
        vehicles = ensemble_vehicles(config, self._params)
        if adapt is not None:
            vehicles = [self._params.with_grip(g) for g in adapt["prior"]]
        integration = _capi.integration_setting(config.get("rollout_substeps", 1), config.get("low_speed_blend"))
        terms = _capi.dynamics_terms(config.get("rate_cost", (0.0, 0.0)), config.get("rate_limit"),
                                     config.get("slip_cost", 0.0), config.get("slip_limit"))
        objective = _capi.dynamics_objective(config.get("progress_cost", 0.0), config.get("speed_ceiling"))
        coupling = _capi.dynamics_coupling(config.get("tyre_coupling"))
        load_transfer = _capi.dynamics_load_transfer(config.get("load_transfer"))
        downforce = _capi.dynamics_downforce(config.get("downforce"))
        lag = config.get("actuator_lag")
        if lag is not None:
            lag = tuple(float(v) for v in np.asarray(lag, dtype=np.float64).reshape(-1))
            if len(lag) != 2:
                raise ValueError("actuator_lag is (tau_d, tau_p), not %r" % (config.get("actuator_lag"),))
            actuator_coefficients(lag, self._dt)             # (ValueError for a negative or non-finite time constant)
        clearance = (float(config.get("clearance_cost", 0.0)), float(config.get("clearance_margin", 0.0)))
        if not all(0.0 <= v <= float(np.finfo(np.float32).max) for v in clearance):   # (a NaN compares false)
            raise ValueError("clearance_cost and clearance_margin must be finite and >= 0, not %r" % (clearance,))
        self._centre_update = config.get("sampling_update", "argmin")   # or "softmin" (MPPI-style weighted mean)
        if self._centre_update not in SAMPLING_UPDATES:
            raise ValueError("sampling_update is 'argmin' or 'softmin', not %r" % (self._centre_update,))
        self._lambda = float(config.get("softmin_lambda", 1.0))
        if not self._lambda > 0.0:
            raise ValueError("softmin_lambda must be positive, not %r" % (self._lambda,))
        nn_window = config.get("nn_window")
        self._engine = _capi.Engine(
            mode=_capi.MODE_DYNAMIC, max_problems=1, max_candidates=self._N, max_steps=self._n,
            step_cost=config.get("step_cost", (1.0, 1.0, 0.0)), r_term=config.get("r_term", (0.5, 10.0)),
            final_cost=config.get("final_cost", (1.0, 1.0, 0.0)), u_min=config.get("u_min", DEFAULT_U_MIN),
            u_max=config.get("u_max", DEFAULT_U_MAX), margin=float(config.get("margin", 0.0)),
            wheelbase=self._params.lf + self._params.lr, dt=self._dt, w_bound=float(config.get("w_bound", 1.0e6)),
            device=device, nn_window=None if nn_window is None else tuple(nn_window),
            centre_update=self._centre_update, softmin_lambda=self._lambda)
        if vehicles is None:
            self._engine.set_dynamics(self._params)
        else:
            self._engine.set_dynamics_ensemble(vehicles, config.get("ensemble_weights"),
                                               config.get("ensemble_reduce", "mean"))
        if integration != (1, 0.0, 0.0):
            self._engine.set_dynamics_integration(integration[0], integration[1:] if integration[2] > 0.0 else None)
        self._rate_terms = bool(np.any(terms[0] != 0.0) or np.any(np.isfinite(terms[1])))
        if self._rate_terms or terms[2] != 0.0 or np.isfinite(terms[3]):
            self._engine.set_dynamics_terms(*terms)
        if objective[0] != 0.0 or objective[1] is not None:
            self._engine.set_dynamics_objective(*objective)
        if coupling is not None:
            self._engine.set_dynamics_coupling(coupling)
        if load_transfer is not None:
            self._engine.set_dynamics_load_transfer(load_transfer)
        if downforce is not None:
            self._engine.set_dynamics_downforce(downforce)
        if clearance != (0.0, 0.0):
            self._engine.set_dynamics_clearance(*clearance)
        self._lag = lag
        self._actuator: Optional[np.ndarray] = None   # the positions the last solve started from (float64), None: cleared
        if lag is not None:
            self._engine.set_dynamics_actuator(lag)
        self._has_obstacles = False
        self._has_surface = False
        self._has_road = False
        self._plan_states = bool(config.get("plan_states", False))
        self._last_state: Optional[np.ndarray] = None   # the start state of the last solve: what trace() re-rolls from
        self._plan: Optional[np.ndarray] = None
        self._calls = 0
        self._adapt = adapt
        self._estimator: Optional[GripEstimator] = None
        self._applied_grip: Optional[tuple] = None   # the estimate the current ensemble was built round
        self.grip = SimpleNamespace(front=None, rear=None, error=float("nan"), accepted=False, errors=None)
        if adapt is not None:
            # the handle's vehicle 0 - what acmpc_score_grips scales - is member 0 of the current ensemble, not `params`:
            # its own scale is divided out so that the grid stays relative to `params`
            self._base_grip = (adapt["prior"][0], adapt["prior"][0])
            self._estimator = GripEstimator(self._score_grips, grid=adapt.get("grid"), axles=adapt.get("axles", "tied"),
                                            window=int(adapt.get("window", 40)), min_window=int(adapt.get("min_window", 10)),
                                            segment=int(adapt.get("segment", 1)), dt=float(adapt.get("log_dt", self._dt)))

    @property
    def engine(self):
        return self._engine

    @property
    def actuator_state(self):
        """`actuator_lag`: the actuator positions (a_d, a_p) the last solve started its plans from, float64 - given, or the
        solver's own estimate; None before there is one (the plans' first commands then stood for them)."""
        return None if self._actuator is None else self._actuator.copy()

    def _actuator_estimate(self, previous_control, warm_steps):
        """The positions at the start of this solve's plans: the last estimate (at first `previous_control`, else the last plan's
        first control) advanced through the first `warm_steps` controls of the last accepted plan."""
        if self._plan is None:
            return None if previous_control is None else np.asarray(previous_control, dtype=np.float64).reshape(2)
        start = self._actuator
        if start is None:
            start = self._plan[0] if previous_control is None else previous_control
        steps = min(max(int(warm_steps), 0), self._n)
        sent = np.asarray(self._plan[:steps], dtype=np.float64)
        start = np.asarray(start, dtype=np.float64).reshape(2)
        return start.copy() if steps == 0 else actuator_response(sent, start, self._lag, self._dt)[1][-1]

    def warm_start(self, steps: int = 1) -> np.ndarray:
        """The centre of the next solve: the last plan shifted by `steps` control steps (its last control repeated), zeros
        at first."""
        if self._plan is None:
            return np.zeros((self._n, 2), dtype=np.float32)
        steps = min(max(int(steps), 0), self._n)
        return np.concatenate([self._plan[steps:], np.repeat(self._plan[-1:], steps, axis=0)]).astype(np.float32)

    def trace(self, plan=None):
        """Engine.trace_plans of `plan` [n, 2] (default: the last accepted plan) from the last solve's start state, on its
        path, previous control, obstacles, surface table, road table and actuator positions, under every vehicle of the handle: dict(states [K, n + 1, 6], cost [K],
        violation [K], terms [K, n, 22] and its named views)."""
        if self._last_state is None:
            raise ValueError("trace() follows a solve")
        plan = self._plan if plan is None else np.asarray(plan, dtype=np.float32)
        if plan is None or plan.shape != (self._n, 2):
            raise ValueError("no accepted plan to trace" if plan is None else "a plan is [n, 2]")
        out = self._engine.trace_plans(self._last_state[None], plan[None, None])
        return {name: (None if a is None else a[0, 0]) for name, a in out.items()}

    def _score_grips(self, states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0)):
        return self._engine.score_grips(states, controls, dt, np.asarray(scales) / np.asarray(self._base_grip), segment=segment,
                                        weights=weights)

    def _adapt_grip(self, state, previous_control):
        """grip_adapt: log this tick, estimate, and rebuild the ensemble round an accepted estimate that has moved."""
        est = self._estimator
        applied = previous_control if previous_control is not None else (None if self._plan is None else self._plan[0])
        if est.transitions == 0 and applied is None:
            est.reset()          # (nothing applied yet: this state starts the log)
        elif applied is None:
            return
        est.push(state, applied)
        self.grip = est.estimate()
        if not self.grip.accepted:
            return
        now = (self.grip.front, self.grip.rear)
        step = est.grid_step * (1.0 - 1e-9)
        if self._applied_grip is None or any(abs(a - b) >= step for a, b in zip(now, self._applied_grip)):
            self._engine.set_dynamics_ensemble([self._params.with_axle_grip(now[0] * b, now[1] * b)
                                                for b in self._adapt["bracket"]], reduce="mean")
            self._applied_grip = now
            self._base_grip = (now[0] * self._adapt["bracket"][0], now[1] * self._adapt["bracket"][0])

    def solve(self, state, reference_path, previous_control=None, obstacles=None, warm_steps: int = 1, surface=None,
              actuator_state=None, road=None):
        """state (X, Y, yaw, vx, vy, r); reference_path a [7, n] table (rows x, y, psi, kappa, ds, width, v) or an object
        with `as_table()` / `_reference_path` giving one.  `previous_control` = (delta, pedal) applied just before this
        solve, for the rate terms' step 0; None: the first control of the last accepted plan (none before there is one).
        `obstacles` = (positions [n, K, 2], radii [K]) for this solve (Engine.set_obstacles); None: no obstacles.
        `surface` = [n, 2] (mu_f, mu_r) per waypoint, or [n], for this solve (Engine.set_surface); None: no table.
        `road` = [n, 3] (a_x, a_y, n_z) per waypoint for this solve (Engine.set_road; dynamic_model.road_table makes one from the
        path's grade and bank); None: a level road.
        `actuator_state` = (a_d, a_p), the measured actuator positions now, with `actuator_lag` (Engine.set_actuator_state);
        None: the solver's own estimate.  `warm_steps`: control steps since the previous solve (warm_start's shift)."""
        table = reference_path
        if hasattr(reference_path, "as_table"):
            table = reference_path.as_table()
        elif hasattr(reference_path, "_reference_path"):
            table = reference_path._reference_path
        table = np.asarray(table, dtype=np.float64)[:, : self._n]
        self._engine.set_paths(table)
        if self._estimator is not None:
            self._adapt_grip(state, previous_control)
        if self._lag is not None:   # (before the rate terms fill `previous_control` in: the estimate starts from what was given)
            self._actuator = (self._actuator_estimate(previous_control, warm_steps) if actuator_state is None
                              else np.asarray(actuator_state, dtype=np.float64).reshape(2).copy())
            self._engine.set_actuator_state(self._actuator)
        if self._rate_terms:
            if previous_control is None and self._plan is not None:
                previous_control = self._plan[0]
            self._engine.set_previous_control(previous_control)
        if obstacles is not None:
            positions = np.asarray(obstacles[0], dtype=np.float32)[: self._n]
            self._engine.set_obstacles(positions, np.asarray(obstacles[1], dtype=np.float32))
            self._has_obstacles = True
        elif self._has_obstacles:
            self._engine.set_obstacles(None)
            self._has_obstacles = False
        if surface is not None:
            self._engine.set_surface(np.asarray(surface, dtype=np.float32)[: self._n])
            self._has_surface = True
        elif self._has_surface:
            self._engine.set_surface(None)
            self._has_surface = False
        if road is not None:
            self._engine.set_road(np.asarray(road, dtype=np.float32)[: self._n])
            self._has_road = True
        elif self._has_road:
            self._engine.set_road(None)
            self._has_road = False
        self._last_state = np.asarray(state, dtype=np.float32).reshape(6).copy()
        out = self._engine.optimize(self._last_state[None], self.warm_start(warm_steps)[None], None,
                                    self._N, self._rounds, self._sigma, seed=self._seed + self._calls)
        self._calls += 1
        u = np.asarray(out["u"][0], dtype=np.float64).reshape(self._n, 2)
        x = np.asarray(out["x"][0], dtype=np.float64).reshape(self._n + 1, 3)
        ok = bool(np.isfinite(out["cost"][0]))
        if ok:
            self._plan = u.astype(np.float32)
        status = SOLVED if ok else "failed"
        obj = SimpleNamespace(x=np.concatenate([x.ravel(), u.ravel()]), info=SimpleNamespace(status=status),
                              cost=float(out["cost"][0]), violation=float(out["violation"][0]),
                              n_feasible=int(out["n_feasible"][0]))
        if self._plan_states:   # the winner under vehicle 0, re-rolled by the arithmetic that scored it
            traced = self._engine.trace_plans(self._last_state[None], u.astype(np.float32)[None, None], want=("states",))
            obj.states = traced["states"][0, 0, 0].astype(np.float64)
        return obj

    def close(self):
        self._engine.close()
