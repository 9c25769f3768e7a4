"""Mode D's tyre coupling on the CPU ("Mode D, tyre coupling"): the identities of the float32
restatement (tests/dynamic_spec.py), the restatement against the float64 mirror
(DynamicBicycleParams.predict_next_state(..., coupling=)), the mirror's physics against figures worked out from the vehicle
block, what the coupling gives the grip identification on a straight-line braking log, and the refusals of the C ABI, the
Engine and the solver's config (host side: no device work).

`python tests/test_dynamic_coupling.py` prints the measured maxima the mirror's bars come from."""
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
from dynamic_spec import Settings  # noqa: E402
import grip_spec as gs  # noqa: E402

T = np.float32
EINVAL, ESTATE = -1, -5
INF, NAN = float("inf"), float("nan")
RATIOS = [(1.0, 1.0), (0.9, 1.1)]
GRID = 0.3 + 0.05 * np.arange(25)          # 0.3 .. 1.5, step 0.05

# The float32 restatement against the float64 mirror, one step of 50 ms from MIRROR_STATES random states - vx in [5, 50],
# |vy| <= 2, |r| <= 1, |delta| <= 0.3, each rounded to float32 first - at the pedals MIRROR_PEDALS and both RATIOS: mixed
# saturated and unsaturated axles.  Measured maxima of |spec - mirror| per state component (X, Y, yaw, vx, vy, r) over that
# set (NumPy 1.26, x86-64; this file's __main__); the bars are 4 x the measured, the project's custom for a specification
# against its mirror.  The loosest points are where an unclipped axle is near saturation: g = sqrt(1 - u^2) turns an error
# of 1e-7 in u into up to 3.5e-4 in g, times a side force of kilonewtons.
MIRROR_STATES = 2000
MIRROR_PEDALS = (-1.0, -0.6, -0.3, 0.0, 0.5, 1.0)
MIRROR_MEASURED = (1.064e-6, 1.062e-6, 1.192e-7, 1.998e-6, 1.100e-6, 1.436e-6)


def _params():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams


def _bits(a):
    return np.asarray(a, dtype=T).view(np.uint32)


def _random_rows(count, seed):
    """(states [count, 6], delta [count], pedal [count]) float32: random states, pedals that include -1, +1, +-0 and NaN,
    steering that includes +-inf."""
    rng = np.random.default_rng(seed)
    st = np.stack([rng.uniform(-50, 50, count), rng.uniform(-50, 50, count), rng.uniform(-4, 4, count),
                   rng.uniform(0.0, 50.0, count), rng.uniform(-2, 2, count), rng.uniform(-1, 1, count)], axis=1).astype(T)
    delta = rng.uniform(-0.3, 0.3, count).astype(T)
    pedal = rng.uniform(-1.2, 1.2, count).astype(T)
    pedal[0::7] = T(-1.0)
    pedal[1::7] = T(1.0)
    pedal[2::7] = T(0.0)
    pedal[3::7] = T(-0.0)
    pedal[4::97] = T(NAN)
    delta[5::101] = T(INF)
    delta[6::103] = T(-INF)
    st[7::50, 3] = T(0.0)     # standstill rows
    return st, delta, pedal


def _constants(vehicle, ratio=None):
    return ds.constants(vehicle, Settings(coupling=ratio), 0.05)


def _step(c, st, delta, pedal):
    return np.stack(ds.dynamic_step(tuple(st[:, q] for q in range(6)), delta, pedal, c), axis=1)


# ---- 1. identities of the restatement ---------------------------------------------------------------------------------------
def test_infinite_ratios_are_the_uncoupled_step_bit_for_bit():
    vehicle = _params().reference().coefficients()
    st, delta, pedal = _random_rows(4000, 1)
    want = _step(_constants(vehicle), st, delta, pedal)
    got = _step(_constants(vehicle, (INF, INF)), st, delta, pedal)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isnan(want).any() and np.isfinite(want).all(axis=1).sum() > 3000     # the NaN / inf rows are in there


@pytest.mark.parametrize("ratio", RATIOS + [(0.05, 0.05), (INF, 0.5)])
def test_pedal_zero_is_the_uncoupled_step_bit_for_bit(ratio):
    vehicle = _params().reference().with_grip(0.6).coefficients()
    st, delta, pedal = _random_rows(4000, 2)
    zero = (pedal == 0) | np.isnan(pedal)        # +0, -0, and the NaN pedal that drives nothing
    assert zero.sum() > 1000 and np.signbit(pedal[zero]).any()
    want = _step(_constants(vehicle), st, delta, pedal)
    got = _step(_constants(vehicle, ratio), st, delta, pedal)
    assert np.array_equal(_bits(got[zero]), _bits(want[zero]))
    assert not np.array_equal(_bits(got[~zero]), _bits(want[~zero]))               # and the coupling does something elsewhere


def test_a_saturated_axle_has_no_side_force_and_the_root_is_never_nan():
    """After the clip |u| <= 1: u = +-1 exactly on a saturated axle, g = 0; a finite state never gets a NaN from the block."""
    vehicle = _params().reference().coefficients()
    k = ds.derived_constants(vehicle)
    st, delta, pedal = _random_rows(4000, 3)
    finite = np.isfinite(delta) & np.isfinite(pedal)
    got = _step(_constants(vehicle, (1.0, 1.0)), st[finite], delta[finite], pedal[finite])
    assert np.isfinite(got).all()
    F_x, F_y = ds.couple_axle(np.array([-20.0, 20.0, 3.0, -0.0], dtype=T), np.array([5.0, -5.0, 5.0, 5.0], dtype=T), T(1.0), k["Pf"])
    assert F_x[0] == -k["Pf"] and F_x[1] == k["Pf"] and F_y[0] == 0 and F_y[1] == 0 and 0 < F_y[2] < 5.0
    assert _bits(F_x[3]) == _bits(T(-0.0)) and _bits(F_y[3]) == _bits(T(5.0))


# ---- 2. the float32 specification against the float64 mirror --------------------------------------------------------------
def _mirror_errors():
    """max |spec - mirror| per state component over the set of the header, and per (ratio, pedal) the worst overall."""
    params = _params().reference()
    rng = np.random.default_rng(77)
    n = MIRROR_STATES
    st = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-3, 3, n), rng.uniform(5, 50, n),
                   rng.uniform(-2, 2, n), rng.uniform(-1, 1, n)], axis=1).astype(T)
    delta = rng.uniform(-0.3, 0.3, n).astype(T)
    worst = np.zeros(6)
    detail = {}
    saturated = {}
    for ratio in RATIOS:
        c = _constants(params.coefficients(), ratio)
        for pedal in MIRROR_PEDALS:
            got = _step(c, st, delta, np.full(n, pedal, dtype=T)).astype(np.float64)
            want = np.empty((n, 6))
            sat = 0
            for i in range(n):
                nxt, _, forces = params.predict_next_state(st[i].astype(np.float64), (float(delta[i]), pedal), 0.05, coupling=ratio)
                nxt[3] = max(nxt[3], 0.0)
                want[i] = nxt
                sat += int(abs(forces[2]) == ratio[0] * params.peak_front) + int(abs(forces[3]) == ratio[1] * params.peak_rear)
            err = np.abs(got - want).max(axis=0)
            worst = np.maximum(worst, err)
            detail[(ratio, pedal)] = err
            saturated[(ratio, pedal)] = sat
    return worst, detail, saturated


def test_the_restatement_against_the_float64_mirror():
    worst, detail, saturated = _mirror_errors()
    for q, name in enumerate(("X", "Y", "yaw", "vx", "vy", "r")):
        print("max |spec - mirror| %s = %.3e (measured %.3e)" % (name, worst[q], MIRROR_MEASURED[q]))
    # mixed: some (ratio, pedal) sets saturate an axle everywhere, some nowhere, some in part
    assert saturated[((1.0, 1.0), -1.0)] >= MIRROR_STATES and saturated[((1.0, 1.0), 0.0)] == 0
    assert any(0 < s < MIRROR_STATES for s in saturated.values())
    for q in range(6):
        assert worst[q] <= 4.0 * MIRROR_MEASURED[q], (q, worst[q])


# ---- 3. physics of the mirror: figures from the vehicle block ---------------------------------------------------------------
def _maps(p, vx):
    brake = p.Cb1 - p.Cb2 * vx - p.Cb3 * vx ** 2
    motor = p.Cm1 - p.Cm2 * vx - p.Cm3 * vx ** 2
    fric = p.Cfric1 + p.Cfric2 * vx + p.Cfric3 * vx ** 2
    return brake, motor, fric


def test_full_braking_is_what_the_front_tyres_give():
    p = _params().reference()
    Pf, Pr = p.peak_front, p.peak_rear
    assert Pf == pytest.approx(6.379, abs=1e-3) and Pr == pytest.approx(6.847, abs=1e-3)
    brake, _, fric = _maps(p, 30.0)
    front, rear = 0.7 * brake, 0.3 * brake
    assert front == pytest.approx(11.84, abs=5e-3) and rear == pytest.approx(5.076, abs=1e-3) and front > 1.85 * Pf
    state = np.array([0.0, 0.0, 0.0, 30.0, 0.0, 0.0])
    _, xd_off, f_off = p.predict_next_state(state, (0.0, -1.0))
    _, xd_on, f_on = p.predict_next_state(state, (0.0, -1.0), coupling=(1.0, 1.0))
    assert -xd_off[3] == pytest.approx((front + rear + fric) / p.mass, rel=1e-12)
    assert (front + rear) / p.mass == pytest.approx(14.59, abs=5e-3)                   # the brake map alone, uncoupled
    assert f_on[2] == -Pf and f_on[3] == pytest.approx(-rear, rel=1e-12)               # the front axle saturates, the rear does not
    assert -xd_on[3] == pytest.approx((Pf + rear + fric) / p.mass, rel=1e-12) and -xd_on[3] < 14.59 < -xd_off[3]
    # half the grip: uncoupled the same deceleration; coupled both axles at their halved peaks
    half = p.with_grip(0.5)
    _, xh_off, _ = half.predict_next_state(state, (0.0, -1.0))
    _, xh_on, fh_on = half.predict_next_state(state, (0.0, -1.0), coupling=(1.0, 1.0))
    assert xh_off[3] == xd_off[3]
    assert fh_on[2] == pytest.approx(-0.5 * Pf, rel=1e-12) and fh_on[3] == pytest.approx(-0.5 * Pr, rel=1e-12)
    assert -xh_on[3] == pytest.approx((0.5 * Pf + 0.5 * Pr + fric) / p.mass, rel=1e-12)
    assert (-xh_on[3] - fric / p.mass) < 0.6 * (-xd_on[3] - fric / p.mass)             # the tyre part: 6.61 kN against 11.46


def test_full_brake_and_steering_leaves_the_front_no_side_force():
    p = _params().reference()
    state = np.array([0.0, 0.0, 0.0, 30.0, 0.0, 0.0])
    _, xd_off, f_off = p.predict_next_state(state, (0.1, -1.0))
    _, xd_on, f_on = p.predict_next_state(state, (0.1, -1.0), coupling=(1.0, 1.0))
    assert f_off[0] > 5.0 and f_on[0] == 0.0                       # uncoupled: full braking AND nearly the full side force
    assert xd_on[5] == -f_on[1] * p.lr / p.Iz                      # the yaw acceleration is the rear axle's alone
    assert f_on[1] == pytest.approx(f_off[1] * np.sqrt(1.0 - (f_on[3] / p.peak_rear) ** 2), rel=1e-12)


def test_full_throttle_on_half_grip_is_half_the_rear_peak():
    p = _params().reference()
    half = p.with_grip(0.5)
    _, motor, _ = _maps(p, 5.0)
    assert motor > 0.5 * p.peak_rear
    assert p.peak_rear > p.Cm1 > 0.9 * p.peak_rear       # from a standstill the drive binds a rear cap of 0.9 Pr, not of Pr
    state = np.array([0.0, 0.0, 0.0, 5.0, 0.0, 0.0])
    forces = half.predict_next_state(state, (0.0, 1.0), coupling=(1.0, 1.0))[2]
    assert forces[3] == pytest.approx(0.5 * p.peak_rear, rel=1e-12) and forces[2] == 0.0
    assert half.predict_next_state(state, (0.0, 1.0))[2][3] == pytest.approx(motor, rel=1e-12)
    # rollout(coupling=) is predict_next_state(coupling=) step by step, sub-steps included
    U = np.array([[0.05, 1.0], [0.05, -1.0], [0.0, -0.4]])
    traj = half.rollout(state, U, 0.05, substeps=2, coupling=(0.9, 1.1))
    x = state.copy()
    for u in U:
        for _ in range(2):
            x = half.predict_next_state(x, u, 0.025, coupling=(0.9, 1.1))[0]
            x[3] = max(x[3], 0.0)
    assert np.array_equal(traj[-1], x)
    assert np.array_equal(half.rollout(state, U, 0.05, coupling=None), half.rollout(state, U, 0.05))
    assert np.array_equal(half.rollout(state, U, 0.05, coupling=(INF, INF)), half.rollout(state, U, 0.05))


# ---- 4. identification --------------------------------------------------------------------------------------------------
def test_braking_in_a_straight_line_now_tells_the_grips_apart():
    from acmpc_amd import GripEstimator
    from acmpc_amd.grip_estimator import grip_scales
    base = _params().reference()
    tied = grip_scales(GRID, "tied")
    states, controls = gs.braking_log(base.with_grip(0.5), (1.0, 1.0))
    assert np.all(states[:, 1:] == 0) and 20.0 < states[-1, 0] < 30.0
    E, best = gs.score(base.coefficients(), states, controls, 0.05, tied, settings=Settings(coupling=(1.0, 1.0)))
    assert tied[best, 0] == pytest.approx(0.5) and E[best] < 1e-6 < np.sort(E)[1]

    def scorer(ratio):
        return lambda x, u, dt, sc, segment=1, weights=(1, 1, 1): gs.score(base.coefficients(), x, u, dt, sc, segment, weights,
                                                        settings=Settings(coupling=ratio))

    for ratio, accepted in (((1.0, 1.0), True), (None, False)):
        est = GripEstimator(scorer(ratio), grid=GRID, axles="tied")          # contrast 0.25, floor 1e-6: the defaults
        for j in range(41):
            est.push(states[j], controls[j - 1] if j else None)
        got = est.estimate()
        assert got.accepted == accepted
        if accepted:
            assert got.front == pytest.approx(0.5) and got.rear == pytest.approx(0.5)
        else:                                                                # uncoupled, delta = 0: every hypothesis ties
            assert got.front is None and np.all(got.errors == got.errors[0])


# ---- 5. host refusals ---------------------------------------------------------------------------------------------------
def _engine(**extra):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    kw = dict(dp["kw"])
    kw.update(extra)
    return Engine(**kw), dp


def _call(eng, ratio):
    r = None if ratio is None else np.array(ratio, dtype=np.float64)
    return eng._lib.acmpc_set_dynamics_coupling(eng._ctx, None if r is None else r.ctypes.data)


def test_entry_point_is_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    lib = acmpc_amd.load_library()
    assert "acmpc_set_dynamics_coupling" in _capi.SIGNATURES and hasattr(lib, "acmpc_set_dynamics_coupling")
    assert hasattr(acmpc_amd.Engine, "set_dynamics_coupling")


def test_set_dynamics_coupling_refusals():
    from acmpc_amd import EngineError, _capi
    vehicle = _params().reference()
    no_front = dataclasses.replace(vehicle, Df=0.0)
    eng, _ = _engine()
    bad = [(0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, -0.5), (NAN, 1.0), (1.0, NAN), (-INF, 1.0), (1e-60, 1.0), (-0.0, 1.0)]
    # from off: a refused ratio leaves the coupling off - a vehicle without front grip is still taken
    for ratio in bad:
        assert _call(eng, ratio) == EINVAL, ratio
        assert b"coupling ratio" in eng._lib.acmpc_last_error(eng._ctx)
        with pytest.raises(ValueError):
            eng.set_dynamics_coupling(ratio)
    eng.set_dynamics(no_front)
    # ... which the coupling then refuses, staying off
    assert _call(eng, (1.0, 1.0)) == EINVAL and b"Pf, Pr" in eng._lib.acmpc_last_error(eng._ctx)
    eng.set_dynamics_ensemble([vehicle, no_front])
    assert _call(eng, (1.0, 1.0)) == EINVAL
    eng.set_dynamics(vehicle)
    for ratio in ((1.0, 1.0), (0.9, 1.1), (INF, INF), (INF, 0.7), (1e60, 1.0), (1e-30, 2.0)):
        assert _call(eng, ratio) == 0, ratio
    # from on: a refused ratio leaves it on - the vehicle without front grip is refused, alone and as a member, and the
    # handle keeps the vehicle it had
    for ratio in bad:
        assert _call(eng, ratio) == EINVAL, ratio
    with pytest.raises(EngineError) as e:
        eng.set_dynamics(no_front)
    assert e.value.code == EINVAL
    with pytest.raises(EngineError) as e:
        eng.set_dynamics_ensemble([vehicle, vehicle.with_grip(0.5), dataclasses.replace(vehicle, Dr=0.0)])
    assert e.value.code == EINVAL
    with pytest.raises(EngineError):
        eng.set_dynamics(dataclasses.replace(vehicle, Dr=-4.0))
    # NULL / None turns it off, and the same vehicles are taken again
    assert _call(eng, None) == 0
    eng.set_dynamics(no_front)
    eng.set_dynamics(vehicle)
    # the Engine's forms: a scalar is both axles; the setting is taken before, between and after the others and survives them
    eng.set_dynamics_coupling(1.0)
    eng.set_dynamics_coupling((0.9, INF))
    for wrong in ("x", (1.0,), (1.0, 2.0, 3.0), (1.0, "y")):
        with pytest.raises(ValueError):
            eng.set_dynamics_coupling(wrong)
    eng.set_dynamics_ensemble([vehicle, vehicle.with_grip(0.6)])
    eng.set_dynamics_integration(4, (3.0, 5.0))
    eng.set_dynamics_terms(rate_weight=(0.3, 0.02), slip_max=0.08)
    eng.set_dynamics_objective(2.0, (1.1, 0.0))
    with pytest.raises(EngineError):
        eng.set_dynamics(no_front)                 # still on
    eng.set_dynamics_coupling(None)
    eng.set_dynamics(no_front)
    assert _capi.dynamics_coupling(None) is None and list(_capi.dynamics_coupling(1.5)) == [1.5, 1.5]
    assert list(_capi.dynamics_coupling((0.9, INF))) == [0.9, INF]
    eng.close()
    # before any vehicle: taken, and the first vehicle is then checked
    eng, _ = _engine()
    eng.set_dynamics_coupling(1.0)
    with pytest.raises(EngineError):
        eng.set_dynamics(no_front)
    eng.set_dynamics(vehicle)
    eng.close()
    for mode in (0, 1):
        other, _ = _engine(mode=mode)
        with pytest.raises(EngineError) as e:
            other.set_dynamics_coupling(1.0)
        assert e.value.code == ESTATE
        assert _call(other, None) == ESTATE
        other.close()
    assert _capi.load_library().acmpc_set_dynamics_coupling(None, None) == EINVAL


@pytest.mark.parametrize("bad", [dict(tyre_coupling=0.0), dict(tyre_coupling=-1.0), dict(tyre_coupling=NAN),
                                 dict(tyre_coupling=(1.0, 0.0)), dict(tyre_coupling=(1.0, 1.0, 1.0)), dict(tyre_coupling="grippy")])
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
    for value in (1.0, (0.9, 1.1), None):
        solver = DynamicSamplingSolver(dict(horizon=10, n_candidates=8, tyre_coupling=value, grip_ensemble=(0.5, 1.0)))
        solver.close()


if __name__ == "__main__":
    worst, detail, saturated = _mirror_errors()
    print("max |spec - mirror| (X, Y, yaw, vx, vy, r):", ", ".join("%.3e" % v for v in worst))
    for key, err in detail.items():
        print(key, "saturated axles %d" % saturated[key], " ".join("%.2e" % v for v in err))
