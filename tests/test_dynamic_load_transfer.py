"""Mode D's longitudinal load transfer on the CPU ("Mode D, load transfer"): the identities of the float32
restatement (tests/dynamic_spec.py), the quadratic peak factor against the exact ratio of peaks, the physics of the float64
mirror (DynamicBicycleParams.predict_next_state(..., load_transfer=)) against figures worked out from the vehicle block, the
restatement against the mirror, what the setting gives the grip identification on a straight-line braking log, and the refusals
of the C ABI, the Engine and the solver's config (host side: no device work).

`python tests/test_dynamic_load_transfer.py` prints the measured maxima of the restatement against the mirror and what the
identification picks without the load transfer."""
import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "ac-mpc_amd"), os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acmpc_oracle as orc  # noqa: E402
import dynamic_spec as ds  # noqa: E402
import grip_spec as gs  # noqa: E402
from dynamic_spec import Settings  # noqa: E402
import test_dynamic_coupling as tdc  # noqa: E402

T = np.float32
EINVAL, ESTATE = -1, -5
INF, NAN = float("inf"), float("nan")
LOAD = (0.35, 0.9)
RATIOS = tdc.RATIOS
GRID = tdc.GRID

# The float32 restatement against the float64 mirror under LOAD over test_dynamic_coupling.py's set - its states, pedals and
# ratios - with that file's bars: 4 x its MIRROR_MEASURED, the coupled figures.  Measured here (NumPy 1.26, x86-64; this
# file's __main__), max |spec - mirror| per state component (X, Y, yaw, vx, vy, r) over that set:
#   1.064e-06, 1.062e-06, 1.192e-07, 1.992e-06, 4.807e-07, 4.313e-07      = 1.00, 1.00, 1.00, 1.00, 0.44, 0.30 x the coupled
# Under the load transfer each of those (ratio, pedal) sets clips an axle in every state or in none: the brake map hardly
# depends on vx, and the caps now rise with the demand.  So that the set still has a partly saturated case, two pedals are
# ADDED, -0.63 and -0.56, at which the front axle clips in 1188 and 1380 of the 2000 states under (1, 1) and (0.9, 1.1).
# Those are the points nearest saturation, where g = sqrt(1 - u^2) is steepest.  Over them X, Y, yaw, vx keep the 4 x bar
# (measured 1.00, 1.00, 1.00, 1.06 x); vy and r measure 5.070e-06 and 7.134e-06 = 4.61 and 4.97 x the coupled figures and do
# NOT hold 4 x.  Their bar on the added pedals is worked out, not measured: u = F_x / (rho P phi) carries about 16 float32
# roundings (the brake map, the bias, the pedal; rho, P, and phi with c_h, the sum, the clip, a1, a2), each 2^-24 relative, so
# |du| <= 16 * 2^-24; two values of u <= 1 that far apart give |dg| <= sqrt(2 |du|) = 1.4e-3 at worst (one of them exactly
# 1); the side force it scales is at most 1.604 Pf (phi_f's maximum); and that force enters vy as F dt / mass and r as
# F lf dt / Iz: near_saturation_bound() below, 6.1e-4 and 8.5e-4 - a worst case over every state, two orders above what a set
# of 2000 finds.
ADDED_PEDALS = (-0.63, -0.56)
MIRROR_PEDALS = tdc.MIRROR_PEDALS + ADDED_PEDALS
MIRROR_FACTOR = 4.0


def near_saturation_bound(p, dt=0.05):
    """(vy, r) bars of the added pedals: the header's derivation."""
    dg = np.sqrt(2.0 * 16.0 * 2.0 ** -24)
    force = 1.604 * p.peak_front
    return dg * force * dt / p.mass, dg * force * p.lf * dt / p.Iz


def _params():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams


def _bits(a):
    return np.asarray(a, dtype=T).view(np.uint32)


def _constants(vehicle, ratio, load):
    """The step's constants under (`ratio`, `load`): with the six scalars while the load transfer is on."""
    return ds.constants(vehicle, Settings(coupling=ratio, load_transfer=load), 0.05)


# ---- 1. identities of the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", RATIOS + [(INF, 0.5)])
def test_zero_height_is_the_coupled_step_bit_for_bit(ratio):
    vehicle = _params().reference().coefficients()
    st, delta, pedal = tdc._random_rows(4000, 11)
    want = tdc._step(_constants(vehicle, ratio, None), st, delta, pedal)
    got = tdc._step(_constants(vehicle, ratio, (0.0, 0.9)), st, delta, pedal)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isnan(want).any() and np.isfinite(want).all(axis=1).sum() > 3000     # the NaN / inf rows are in there
    moved = tdc._step(_constants(vehicle, ratio, LOAD), st, delta, pedal)
    assert not np.array_equal(_bits(moved), _bits(want))                           # and a height does something


@pytest.mark.parametrize("ratio", [None, (INF, INF)])
def test_zero_height_without_the_coupling_is_the_plain_step_bit_for_bit(ratio):
    vehicle = _params().reference().with_grip(0.7).coefficients()
    st, delta, pedal = tdc._random_rows(4000, 12)
    want = tdc._step(_constants(vehicle, None, None), st, delta, pedal)
    got = tdc._step(_constants(vehicle, ratio, (0.0, 0.5)), st, delta, pedal)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("ratio", RATIOS + [None])
def test_pedal_zero_is_the_step_without_the_setting_bit_for_bit(ratio):
    vehicle = _params().reference().with_grip(0.6).coefficients()
    st, delta, pedal = tdc._random_rows(4000, 13)
    zero = (pedal == 0) | np.isnan(pedal)        # +0, -0, and the NaN pedal that drives nothing
    assert zero.sum() > 1000 and np.signbit(pedal[zero]).any()
    want = tdc._step(_constants(vehicle, ratio, None), st, delta, pedal)
    got = tdc._step(_constants(vehicle, ratio, LOAD), st, delta, pedal)
    assert np.array_equal(_bits(got[zero]), _bits(want[zero]))
    assert not np.array_equal(_bits(got[~zero]), _bits(want[~zero]))


def test_without_the_coupling_the_estimate_is_the_force_itself():
    """rho = +inf: e = F, the transfer of what the uncoupled model really decelerates with."""
    p = _params().reference()
    k = _constants(p.coefficients(), None, LOAD).k
    F_fx, F_rx = np.array([-11.0, 0.0, -3.0], dtype=T), np.array([-5.0, 9.0, 2.0], dtype=T)
    _, _, w = ds.loaded_peaks(F_fx, F_rx, T(INF), T(INF), k)
    with np.errstate(all="ignore"):
        want = np.fmax(np.fmin(k["c_h"] * (F_fx + F_rx), k["w_max"]), -k["w_max"])
    assert np.array_equal(_bits(w), _bits(want)) and w[0] < 0 < w[1]


# ---- 2. the quadratic factor against the exact ratio of peaks -----------------------------------------------------------
def test_the_factor_is_the_exact_ratio_of_peaks():
    p = _params().reference()
    c = ds.constants64(p.coefficients(), LOAD)
    assert c["c_h"] == pytest.approx(0.1208, abs=1e-4) and c["w_max"] == pytest.approx(4.905, abs=1e-3)
    x = np.linspace(-c["w_max"], c["w_max"], 20001)
    lo_hi = {}
    for axle, F_z, sign in (("f", p.F_zf, -1.0), ("r", p.F_zr, 1.0)):
        a1, a2 = c["a1_" + axle], c["a2_" + axle]
        phi = 1 + x * (a1 + a2 * x)
        exact = np.array([p.peak(axle, F_z + v) for v in x]) / p.peak(axle, F_z)
        assert np.max(np.abs(phi - exact) / np.abs(exact)) <= 1e-12
        lo_hi[axle] = (phi.min(), phi.max())
        c32 = _constants(p.coefficients(), None, LOAD).k
        x32 = np.concatenate([x.astype(T), [T(c32["w_max"]), -T(c32["w_max"])]]).astype(T)
        phi32 = T(1.0) + x32 * (c32["a1_" + axle] + c32["a2_" + axle] * x32)
        assert phi32.dtype == T and np.all(phi32 > 0)
    assert lo_hi["f"] == pytest.approx((0.116, 1.604), abs=1e-3) and lo_hi["r"] == pytest.approx((0.220, 1.324), abs=1e-3)
    # the rear vertex (a maximum: eps < 0) lies outside +-w_max: phi_r is monotonic over the load that may move
    assert -c["a1_r"] / (2 * c["a2_r"]) == pytest.approx(5.95, abs=1e-2) and 5.95 > c["w_max"]


# ---- 3. physics of the mirror: figures from the vehicle block ---------------------------------------------------------------
def test_full_braking_moves_load_to_the_front():
    p = _params().reference()
    brake, _, fric = tdc._maps(p, 30.0)
    front, rear = 0.7 * brake, 0.3 * brake
    state = np.array([0.0, 0.0, 0.0, 30.0, 0.0, 0.0])
    w, F_zf, F_zr = p.loaded_axles(-front, -rear, (1.0, 1.0), LOAD)
    assert w == pytest.approx(-1.3835, abs=1e-3)
    Pf, Pr = p.peak("f", F_zf), p.peak("r", F_zr)
    assert Pf == pytest.approx(7.647, abs=1e-3) and Pr == pytest.approx(5.657, abs=1e-3)
    _, xd_static, f_static = p.predict_next_state(state, (0.0, -1.0), coupling=(1.0, 1.0))
    _, xd, f = p.predict_next_state(state, (0.0, -1.0), coupling=(1.0, 1.0), load_transfer=LOAD)
    assert f[2] == -Pf and f[3] == pytest.approx(-5.076, abs=1e-3) and f[3] == pytest.approx(-rear, rel=1e-12)
    assert abs(f[3]) < Pr and abs(f[3]) / Pr == pytest.approx(0.90, abs=0.01)            # the rear: 90 % of what is left
    assert xd[3] / xd_static[3] == pytest.approx((Pf + rear + fric) / (p.peak_front + rear + fric), rel=1e-12)
    assert xd[3] / xd_static[3] == pytest.approx((7.647 + 5.076 + fric) / (6.379 + 5.076 + fric), abs=2e-4)
    # a scalar is the height with w_frac = 0.9
    assert np.array_equal(p.predict_next_state(state, (0.0, -1.0), coupling=1.0, load_transfer=0.35)[1], xd)
    # half the grip: both axles saturate at half their loaded peaks (the estimate is clipped at the halved static caps)
    half = p.with_grip(0.5)
    wh, F_zfh, F_zrh = half.loaded_axles(-front, -rear, (1.0, 1.0), LOAD)
    assert wh == pytest.approx(-0.35 / (p.lf + p.lr) * 0.5 * (p.peak_front + p.peak_rear), rel=1e-12)
    fh = half.predict_next_state(state, (0.0, -1.0), coupling=(1.0, 1.0), load_transfer=LOAD)[2]
    assert fh[2] == pytest.approx(-0.5 * p.peak("f", F_zfh), rel=1e-12) and fh[3] == pytest.approx(-0.5 * p.peak("r", F_zrh), rel=1e-12)
    assert fh[2] == -half.peak("f", F_zfh) and fh[3] == -half.peak("r", F_zrh)


def test_full_brake_and_steering_leaves_the_front_no_side_force():
    p = _params().reference()
    state = np.array([0.0, 0.0, 0.0, 30.0, 0.0, 0.0])
    f = p.predict_next_state(state, (0.1, -1.0), coupling=(1.0, 1.0), load_transfer=LOAD)[2]
    off = p.predict_next_state(state, (0.1, -1.0), load_transfer=LOAD)[2]
    assert off[0] > 5.0 and f[0] == 0.0             # the front axle is saturated at its loaded peak: exactly no side force
    assert abs(f[3]) < abs(f[2])                    # (the rear axle is not)


def test_full_throttle_from_a_standstill_moves_load_to_the_rear():
    p = _params().reference()
    state = np.zeros(6)
    _, motor, _ = tdc._maps(p, 0.0)
    w, F_zf, F_zr = p.loaded_axles(0.0, motor, (1.0, 1.0), LOAD)
    assert w > 0 and p.peak("r", F_zr) > p.peak_rear and p.peak("f", F_zf) < p.peak_front
    f = p.predict_next_state(state, (0.0, 1.0), coupling=(1.0, 1.0), load_transfer=LOAD)[2]
    assert f[3] == pytest.approx(min(motor, p.peak("r", F_zr)), rel=1e-12) and f[2] == 0.0
    # rollout(load_transfer=) is predict_next_state(load_transfer=) step by step, sub-steps included; None is the parent
    U = np.array([[0.05, 1.0], [0.05, -1.0], [0.0, -0.4]])
    start = np.array([0.0, 0.0, 0.0, 20.0, 0.0, 0.0])
    traj = p.rollout(start, U, 0.05, substeps=2, coupling=(0.9, 1.1), load_transfer=LOAD)
    x = start.copy()
    for u in U:
        for _ in range(2):
            x = p.predict_next_state(x, u, 0.025, coupling=(0.9, 1.1), load_transfer=LOAD)[0]
            x[3] = max(x[3], 0.0)
    assert np.array_equal(traj[-1], x)
    assert np.array_equal(p.rollout(start, U, 0.05, coupling=1.0, load_transfer=None), p.rollout(start, U, 0.05, coupling=1.0))
    assert np.array_equal(p.rollout(start, U, 0.05, coupling=1.0, load_transfer=(0.0, 0.9)), p.rollout(start, U, 0.05, coupling=1.0))
    assert not np.array_equal(traj, p.rollout(start, U, 0.05, substeps=2, coupling=(0.9, 1.1)))


# ---- 4. the float32 specification against the float64 mirror --------------------------------------------------------------
def _mirror_errors():
    """test_dynamic_coupling._mirror_errors - its states, pedals and ratios - under LOAD: max |spec - mirror| per state
    component, per (ratio, pedal) the worst, and how many axles were clipped."""
    params = _params().reference()
    rng = np.random.default_rng(77)
    n = tdc.MIRROR_STATES
    st = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-3, 3, n), rng.uniform(5, 50, n),
                   rng.uniform(-2, 2, n), rng.uniform(-1, 1, n)], axis=1).astype(T)
    delta = rng.uniform(-0.3, 0.3, n).astype(T)
    worst = np.zeros(6)
    detail = {}
    saturated = {}
    for ratio in RATIOS:
        c = _constants(params.coefficients(), ratio, LOAD)
        for pedal in MIRROR_PEDALS:
            got = tdc._step(c, st, delta, np.full(n, pedal, dtype=T)).astype(np.float64)
            want = np.empty((n, 6))
            sat = 0
            for i in range(n):
                nxt, _, forces = params.predict_next_state(st[i].astype(np.float64), (float(delta[i]), pedal), 0.05, coupling=ratio,
                                                           load_transfer=LOAD)
                nxt[3] = max(nxt[3], 0.0)
                want[i] = nxt
                brake, motor, _ = tdc._maps(params, float(st[i, 3]))
                demand_f = brake * params.brake_bias * min(0.0, pedal)
                demand_r = brake * (1 - params.brake_bias) * min(0.0, pedal) + motor * max(0.0, pedal)
                sat += int(forces[2] != demand_f) + int(forces[3] != demand_r)
            err = np.abs(got - want).max(axis=0)
            worst = np.maximum(worst, err)
            detail[(ratio, pedal)] = err
            saturated[(ratio, pedal)] = sat
    return worst, detail, saturated


def test_the_restatement_against_the_float64_mirror():
    _, detail, saturated = _mirror_errors()
    issue_set = np.max([err for (ratio, pedal), err in detail.items() if pedal not in ADDED_PEDALS], axis=0)
    added = np.max([err for (ratio, pedal), err in detail.items() if pedal in ADDED_PEDALS], axis=0)
    for q, name in enumerate(("X", "Y", "yaw", "vx", "vy", "r")):
        print("max |spec - mirror| %s = %.3e (%.2f x the coupled %.3e); on the added pedals %.3e (%.2f x)"
              % (name, issue_set[q], issue_set[q] / tdc.MIRROR_MEASURED[q], tdc.MIRROR_MEASURED[q], added[q], added[q] / tdc.MIRROR_MEASURED[q]))
    # mixed: some (ratio, pedal) sets saturate an axle everywhere, some nowhere, some in part
    assert saturated[((1.0, 1.0), -1.0)] >= tdc.MIRROR_STATES and saturated[((1.0, 1.0), 0.0)] == 0
    assert any(0 < s < tdc.MIRROR_STATES for s in saturated.values())
    for q in range(6):
        assert issue_set[q] <= MIRROR_FACTOR * tdc.MIRROR_MEASURED[q], (q, issue_set[q])
    bound = near_saturation_bound(_params().reference())
    for q in range(4):
        assert added[q] <= MIRROR_FACTOR * tdc.MIRROR_MEASURED[q], (q, added[q])
    assert added[4] <= bound[0] and added[5] <= bound[1], (added[4:], bound)


# ---- 5. identification ------------------------------------------------------------------------------------------------------
def _identification():
    from acmpc_amd.grip_estimator import grip_scales
    base = _params().reference()
    tied = grip_scales(GRID, "tied")
    states, controls = gs.braking_log(base.with_grip(0.5), (1.0, 1.0), LOAD)
    with_load = gs.score(base.coefficients(), states, controls, 0.05, tied, settings=Settings(coupling=(1.0, 1.0), load_transfer=LOAD))
    without = gs.score(base.coefficients(), states, controls, 0.05, tied, settings=Settings(coupling=(1.0, 1.0)))
    return tied, states, with_load, without


def test_braking_in_a_straight_line_finds_the_grip_under_the_same_settings():
    tied, states, (E, best), (E_off, best_off) = _identification()
    assert np.all(states[:, 1:] == 0) and 15.0 < states[-1, 0] < 30.0
    assert tied[best, 0] == pytest.approx(0.5) and E[best] < 1e-6 < np.sort(E)[1]
    # recorded in DESIGN.md section 6, not asserted: what the coupling alone reads the loaded car's braking as
    print("scored without the load transfer: picks grip %.2f, error %.3e (with it: %.2f, %.3e)"
          % (tied[best_off, 0], E_off[best_off], tied[best, 0], E[best]))


def test_the_segment_loop_without_the_setting_is_the_couplings():
    base = _params().reference()
    from acmpc_amd.grip_estimator import grip_scales
    tied = grip_scales(GRID, "tied")
    states, controls = gs.braking_log(base.with_grip(0.5), (1.0, 1.0), LOAD)
    fine = Settings(substeps=2, low_speed_blend=(3.0, 5.0), coupling=(0.9, 1.1))
    b = gs.score(base.coefficients(), states, controls, 0.05, tied, segment=8, settings=fine)
    c = gs.score(base.coefficients(), states, controls, 0.05, tied, segment=8, settings=fine.replace(load_transfer=(0.0, 0.9)))
    assert np.array_equal(_bits(c[0]), _bits(b[0])) and c[1] == b[1]


# ---- 7. host refusals ---------------------------------------------------------------------------------------------------
def _engine(**extra):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    kw = dict(dp["kw"])
    kw.update(extra)
    return Engine(**kw), dp


def _call(eng, setting):
    r = None if setting is None else np.array(setting, dtype=np.float64)
    return eng._lib.acmpc_set_dynamics_load_transfer(eng._ctx, None if r is None else r.ctypes.data)


BAD = [(-1.0, 0.9), (-1e-300, 0.9), (NAN, 0.9), (INF, 0.9), (-INF, 0.9), (0.35, 0.0), (0.35, 1.0), (0.35, -0.1), (0.35, 1.5),
       (0.35, NAN), (0.35, INF)]


def test_entry_point_is_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    lib = acmpc_amd.load_library()
    assert "acmpc_set_dynamics_load_transfer" in _capi.SIGNATURES and hasattr(lib, "acmpc_set_dynamics_load_transfer")
    assert hasattr(acmpc_amd.Engine, "set_dynamics_load_transfer")


def test_set_dynamics_load_transfer_refusals():
    from acmpc_amd import EngineError, _capi
    vehicle = _params().reference()
    no_front = dataclasses.replace(vehicle, Df=0.0)           # a peak that is not > 0
    sinking = dataclasses.replace(vehicle, epsf=-0.5)         # a front factor phi that turns non-positive inside +-w_max
    eng, _ = _engine()
    # from off: a refused setting leaves it off - vehicles it would refuse are still taken
    for setting in BAD:
        assert _call(eng, setting) == EINVAL, setting
        assert b"h_cg" in eng._lib.acmpc_last_error(eng._ctx) or b"w_frac" in eng._lib.acmpc_last_error(eng._ctx)
        with pytest.raises(ValueError):
            eng.set_dynamics_load_transfer(*setting)
    eng.set_dynamics(sinking)
    # ... which the setting then refuses, staying off
    assert _call(eng, LOAD) == EINVAL and b"phi" in eng._lib.acmpc_last_error(eng._ctx)
    eng.set_dynamics(no_front)
    assert _call(eng, LOAD) == EINVAL and b"Pf, Pr" in eng._lib.acmpc_last_error(eng._ctx)
    eng.set_dynamics_ensemble([vehicle, sinking])
    assert _call(eng, LOAD) == EINVAL
    eng.set_dynamics(no_front)                                  # (still off: taken)
    eng.set_dynamics(vehicle)
    for setting in (LOAD, (0.0, 0.5), (0.35, 0.999), (2.0, 1e-3), (-0.0, 0.9)):
        assert _call(eng, setting) == 0, setting
    assert _call(eng, LOAD) == 0
    # from on: a refused setting leaves it on - the vehicles are refused, alone and as members, by acmpc_set_dynamics and
    # acmpc_set_dynamics_ensemble, and the handle keeps the vehicle it had
    for setting in BAD:
        assert _call(eng, setting) == EINVAL, setting
    for bad_vehicle in (sinking, no_front, dataclasses.replace(vehicle, Dr=-4.0)):
        with pytest.raises(EngineError) as e:
            eng.set_dynamics(bad_vehicle)
        assert e.value.code == EINVAL
        with pytest.raises(EngineError) as e:
            eng.set_dynamics_ensemble([vehicle, vehicle.with_grip(0.5), bad_vehicle])
        assert e.value.code == EINVAL
    # a setting under which the vehicle's factor stays positive is taken for it: the refusal is the factor's, not the vehicle's
    assert _call(eng, (0.35, 0.05)) == 0
    eng.set_dynamics(sinking)
    assert _call(eng, LOAD) == EINVAL                            # and the wider one is refused, the narrow one kept
    with pytest.raises(EngineError):
        eng.set_dynamics(no_front)
    # NULL / None turns it off, and the same vehicles are taken again
    assert _call(eng, None) == 0
    eng.set_dynamics(no_front)
    eng.set_dynamics(vehicle)
    # the Engine's forms; the setting is taken before, between and after the others and survives them
    eng.set_dynamics_load_transfer(0.35)
    eng.set_dynamics_load_transfer((0.35, 0.8))
    eng.set_dynamics_load_transfer(0.35, 0.8)
    for wrong in ("x", (1.0,), (1.0, 0.5, 3.0), (1.0, "y")):
        with pytest.raises(ValueError):
            eng.set_dynamics_load_transfer(wrong)
    eng.set_dynamics_ensemble([vehicle, vehicle.with_grip(0.6)])
    eng.set_dynamics_integration(4, (3.0, 5.0))
    eng.set_dynamics_terms(rate_weight=(0.3, 0.02), slip_max=0.08)
    eng.set_dynamics_objective(2.0, (1.1, 0.0))
    eng.set_dynamics_coupling((0.9, 1.1))
    eng.set_dynamics_coupling(None)
    with pytest.raises(EngineError):
        eng.set_dynamics(sinking)                  # still on
    eng.set_dynamics_load_transfer(None)
    eng.set_dynamics(sinking)
    assert _capi.dynamics_load_transfer(None) is None and list(_capi.dynamics_load_transfer(0.35)) == [0.35, 0.9]
    assert list(_capi.dynamics_load_transfer((0.2, 0.5))) == [0.2, 0.5]
    eng.close()
    # before any vehicle: taken, and the first vehicle is then checked
    eng, _ = _engine()
    eng.set_dynamics_load_transfer(0.35)
    with pytest.raises(EngineError):
        eng.set_dynamics(sinking)
    eng.set_dynamics(vehicle)
    eng.close()
    for mode in (0, 1):
        other, _ = _engine(mode=mode)
        with pytest.raises(EngineError) as e:
            other.set_dynamics_load_transfer(0.35)
        assert e.value.code == ESTATE
        assert _call(other, None) == ESTATE
        other.close()
    assert _capi.load_library().acmpc_set_dynamics_load_transfer(None, None) == EINVAL


@pytest.mark.parametrize("bad", [dict(load_transfer=-0.1), dict(load_transfer=NAN), dict(load_transfer=INF),
                                 dict(load_transfer=(0.35, 0.0)), dict(load_transfer=(0.35, 1.0)),
                                 dict(load_transfer=(0.35, 0.9, 1.0)), dict(load_transfer="high")])
def test_solver_config_is_checked_before_any_handle_exists(bad, monkeypatch):
    from acmpc_amd import _capi
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver

    def no_engine(*args, **kwargs):
        raise AssertionError("a handle was created for a config that must be refused")

    monkeypatch.setattr(_capi, "Engine", no_engine)
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(horizon=20, n_candidates=64, **bad))


def test_solver_takes_the_key_without_device_work():
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    for value in (0.35, (0.35, 0.8), None):
        solver = DynamicSamplingSolver(dict(horizon=10, n_candidates=8, tyre_coupling=1.0, load_transfer=value, grip_ensemble=(0.5, 1.0)))
        solver.close()


if __name__ == "__main__":
    worst, detail, saturated = _mirror_errors()
    print("max |spec - mirror| (X, Y, yaw, vx, vy, r):", ", ".join("%.3e" % v for v in worst))
    print("against the coupled figures:", ", ".join("%.2f" % (v / m) for v, m in zip(worst, tdc.MIRROR_MEASURED)))
    for key, err in detail.items():
        print(key, "clipped axles %d" % saturated[key], " ".join("%.2e" % v for v in err))
    tied, states, (E, best), (E_off, best_off) = _identification()
    print("identification with the load transfer: grip %.2f error %.3e next %.3e" % (tied[best, 0], E[best], np.sort(E)[1]))
    print("identification without it:             grip %.2f error %.3e next %.3e" % (tied[best_off, 0], E_off[best_off], np.sort(E_off)[1]))
