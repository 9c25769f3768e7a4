"""Mode D's integration setting on the CPU ("Sub-steps and the low-speed blend"): the float32
restatement (tests/dynamic_spec.py) under Settings(1, None) against its default and against the float64 mirror
at others, what the setting buys at low speed - 24 constant-control runs from 0 .. 10 m/s against a fine integration - and
the refusals of the C ABI, the Engine and the solver's config (host-side: no device work)."""
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

GOLDEN = np.load(os.path.join(HERE, "golden", "dynamic_bicycle.npz"))
EINVAL = -1
POSITION_BOUND_M = 1.0e-3     # test_dynamic_model.py's: the float32 specification against the mirror over 50 steps
STEP_BOUND = 1.0e-5           # and over one step, relative to max(|x|, 1)
BLEND = (3.0, 5.0)

# the low-speed study: 49 steps of 0.05 s under a constant control from (0, 0, 0, v0, 0, 0)
STUDY_STEPS, STUDY_DT = 49, 0.05
STUDY_CASES = [(v0, delta, pedal) for v0 in (0.0, 2.0, 4.0, 6.0, 8.0, 10.0) for delta in (0.03, 0.05) for pedal in (0.1, 0.5)]
FINE_SUBSTEPS = 64            # the comparison: the same model (and blend) with 64 sub-steps per control step
YAW_BOUND_RAD = 0.005
STUDY_POSITION_BOUND_M = 0.2
INCREMENT_FLOOR = 1.0e-3      # rad/s: smaller yaw-rate increments are not counted as a direction
MAX_SIGN_CHANGES = 2
MIN_SIGN_CHANGES_DEFAULT = 30
CONVERGENCE_RATIO = 0.7       # M = 8's worst position error against M = 4's


def _params():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def sign_changes(r):
    """Sign changes of the yaw-rate increment r[i + 1] - r[i] along a run, over the increments above INCREMENT_FLOOR."""
    d = np.diff(np.asarray(r, dtype=np.float64))
    d = d[np.abs(d) > INCREMENT_FLOOR]
    return int(np.count_nonzero(np.sign(d[1:]) != np.sign(d[:-1])))


def test_entry_point_is_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    assert "acmpc_set_dynamics_integration" in _capi.SIGNATURES
    assert _capi.MAX_SUBSTEPS == ds.MAX_SUBSTEPS == 16
    assert hasattr(acmpc_amd.Engine, "set_dynamics_integration")
    assert hasattr(acmpc_amd.load_library(), "acmpc_set_dynamics_integration")


@pytest.mark.parametrize("track,H,N,seed,vx0,window", [("monza", 20, 33, 0, None, None), ("monza", 50, 17, 1, 0.0, (2, 5)),
                                                       ("monza", 8, 9, 2, 4.0, None)])
def test_default_setting_is_dynamic_spec_bit_for_bit(track, H, N, seed, vx0, window):
    dp = ds.make_dynamic_problem(orc, track, H, N, seed, vx0=vx0)
    dp["U"][1, 0, 0] = np.nan   # (a NaN and an inf control go through the same way)
    dp["U"][4, H // 2, 1] = np.inf
    coef = orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(np.float32)
    vehicle = _params().reference().coefficients()
    want = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True)
    got = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True,
                        settings=Settings(substeps=1, low_speed_blend=None))
    for a, b in zip(want, got):
        assert np.array_equal(_bits(a), _bits(b))
    # and another setting is another result (the restatement is not a pass-through)
    other = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, settings=Settings(substeps=4, low_speed_blend=BLEND))
    assert not np.array_equal(_bits(want[0]), _bits(other[0]))


def test_step_size_and_blend_constants_round_once():
    assert ds.constants(None, Settings(), 0.05).h == np.float32(0.05)
    for m in range(1, 17):
        assert ds.constants(None, Settings(substeps=m), 0.05).h == np.float32(0.05 / m)
    assert ds.constants(None, Settings(), 0.05).blend is None
    lo, inv = ds.constants(None, Settings(low_speed_blend=(3.0, 5.0)), 0.05).blend
    assert (lo, inv) == (np.float32(3.0), np.float32(0.5))
    p = _params().reference()
    assert ds.constants(p.coefficients()).k["inv_L"] == np.float32(1.0 / (p.lf + p.lr))


def test_blend_passes_the_dynamic_state_through_above_v_hi_and_is_kinematic_below_v_lo():
    p = _params().reference()
    vehicle = p.coefficients()
    plain, blended = ds.constants(vehicle, Settings(), 0.05), ds.constants(vehicle, Settings(low_speed_blend=BLEND), 0.05)
    delta, pedal = np.float32([0.05, -0.1]), np.float32([0.3, 0.2])
    fast = tuple(np.float32([v, v]) for v in (0.0, 0.0, 0.1, 9.0, 0.2, 0.05))
    want = ds.dynamic_step(fast, delta, pedal, plain)
    got = ds.control_step(fast, delta, pedal, blended)
    for a, b in zip(want, got):
        assert np.array_equal(_bits(a), _bits(b))
    slow = tuple(np.float32([v, v]) for v in (0.0, 0.0, 0.1, 1.5, 0.2, 0.05))
    got = ds.control_step(slow, delta, pedal, blended)
    vx = got[3].astype(np.float64)
    r_k = vx * np.tan(delta.astype(np.float64)) / (p.lf + p.lr)
    np.testing.assert_allclose(got[5], r_k, rtol=2e-6)
    np.testing.assert_allclose(got[4], r_k * p.lr, rtol=2e-6)


def test_mirror_default_is_todays_rollout():
    p = _params().reference()
    for x0, U, S in zip(GOLDEN["roll_x0"], GOLDEN["roll_u"], GOLDEN["roll_states"]):
        got = p.rollout(x0, U, float(GOLDEN["roll_dt"]), substeps=1, low_speed_blend=None)
        assert np.array_equal(got, p.rollout(x0, U, float(GOLDEN["roll_dt"])))
        np.testing.assert_allclose(got, S, rtol=1e-12, atol=1e-9)
    with pytest.raises(ValueError):
        p.rollout(GOLDEN["roll_x0"][0], GOLDEN["roll_u"][0], 0.05, substeps=0)


@pytest.mark.parametrize("substeps,blend", [(4, BLEND), (2, None), (1, BLEND), (16, BLEND)])
def test_float32_spec_tracks_the_float64_mirror(substeps, blend):
    """test_dynamic_model.py's two bounds, with the same setting on both sides: one control step from the mirror's state
    within 1e-5 of the mirror's next, and the positions of the whole rollout within 1e-3 m."""
    p = _params().reference()
    vehicle = p.coefficients()
    dt = float(GOLDEN["roll_dt"])
    x0, U = np.asarray(GOLDEN["roll_x0"]), np.asarray(GOLDEN["roll_u"])
    S = np.stack([p.rollout(a, u, dt, substeps=substeps, low_speed_blend=blend) for a, u in zip(x0, U)])   # [B, n + 1, 6]
    one = gs.rollout_states(S[:, :-1].reshape(-1, 6), U.reshape(-1, 1, 2), vehicle, dt, settings=Settings(substeps, blend))[:, 1]
    nxt = S[:, 1:].reshape(-1, 6)
    worst_step = float(np.max(np.abs(one.astype(np.float64) - nxt) / np.maximum(np.abs(nxt), 1.0)))
    traj = gs.rollout_states(x0, U, vehicle, dt, settings=Settings(substeps=substeps, low_speed_blend=blend)).astype(np.float64)
    worst_pos = float(np.max(np.hypot(traj[..., 0] - S[..., 0], traj[..., 1] - S[..., 1])))
    print("substeps %d blend %s: worst step %.3g, worst position %.3g m" % (substeps, blend, worst_step, worst_pos))
    assert worst_step <= STEP_BOUND
    assert worst_pos < POSITION_BOUND_M


@pytest.fixture(scope="module")
def study():
    """The 24 runs: the mirror at 64 sub-steps with the blend (the comparison), the mirror at the default setting."""
    p = _params().reference()
    x0 = np.array([[0.0, 0.0, 0.0, v0, 0.0, 0.0] for v0, _, _ in STUDY_CASES])
    U = np.array([np.tile([delta, pedal], (STUDY_STEPS, 1)) for _, delta, pedal in STUDY_CASES])
    fine = np.stack([p.rollout(a, u, STUDY_DT, substeps=FINE_SUBSTEPS, low_speed_blend=BLEND) for a, u in zip(x0, U)])
    default = np.stack([p.rollout(a, u, STUDY_DT) for a, u in zip(x0, U)])
    return dict(x0=x0, U=U, fine=fine, default=default, vehicle=p.coefficients())


def _study_errors(study, substeps):
    got = gs.rollout_states(study["x0"], study["U"], study["vehicle"], STUDY_DT, settings=Settings(substeps, BLEND)).astype(np.float64)
    fine = study["fine"]
    yaw = np.abs(got[:, -1, 2] - fine[:, -1, 2])
    pos = np.hypot(got[:, -1, 0] - fine[:, -1, 0], got[:, -1, 1] - fine[:, -1, 1])
    flips = np.array([sign_changes(run[:, 5]) for run in got])
    return yaw, pos, flips


def test_low_speed_study(study):
    """The float32 specification at 4 sub-steps with the blend (3, 5) against the fine integration: final yaw within
    0.005 rad, final position within 0.2 m, at most 2 sign changes of the yaw-rate increment in every one of the 24 runs;
    8 sub-steps at most 0.7 of 4's worst position error.  The contrast: the mirror at the default setting changes the sign
    of that increment at least 30 times in 48 in every run that starts at 4 m/s or more."""
    yaw4, pos4, flips4 = _study_errors(study, 4)
    yaw8, pos8, flips8 = _study_errors(study, 8)
    default_flips = np.array([sign_changes(run[:, 5]) for run in study["default"]])
    moving = np.array([v0 >= 4.0 for v0, _, _ in STUDY_CASES])
    print("M = 4: yaw %.4g rad, position %.4g m, sign changes %d" % (yaw4.max(), pos4.max(), flips4.max()))
    print("M = 8: yaw %.4g rad, position %.4g m, sign changes %d, ratio %.3f" % (yaw8.max(), pos8.max(), flips8.max(),
                                                                                 pos8.max() / pos4.max()))
    print("default: sign changes %s" % (default_flips,))
    assert yaw4.max() <= YAW_BOUND_RAD
    assert pos4.max() <= STUDY_POSITION_BOUND_M
    assert flips4.max() <= MAX_SIGN_CHANGES
    assert pos8.max() <= CONVERGENCE_RATIO * pos4.max()
    assert default_flips[moving].min() >= MIN_SIGN_CHANGES_DEFAULT


def _engine(**extra):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    kw = dict(dp["kw"])
    kw.update(extra)
    return Engine(**kw), dp


def test_set_dynamics_integration_refusals():
    from acmpc_amd import EngineError
    eng, _ = _engine()
    lib, ctx = eng._lib, eng._ctx
    for m in (0, 17, -1):
        assert lib.acmpc_set_dynamics_integration(ctx, m, 0.0, 0.0) == EINVAL
    for lo, hi in ((5.0, 3.0), (3.0, 3.0), (-1.0, 5.0), (np.nan, 5.0), (3.0, np.nan), (3.0, np.inf), (0.0, -0.0 - 1.0)):
        assert lib.acmpc_set_dynamics_integration(ctx, 4, lo, hi) == EINVAL
        assert b"blend" in lib.acmpc_last_error(ctx)
    for m, lo, hi in ((1, 0.0, 0.0), (16, 0.0, 0.0), (4, 3.0, 5.0), (1, 0.0, 0.5), (1, 0.0, 0.0)):
        assert lib.acmpc_set_dynamics_integration(ctx, m, lo, hi) == 0
    # the setting does not depend on a vehicle: it is taken before, after and between acmpc_set_dynamics[_ensemble]
    good = _params().reference()
    eng.set_dynamics_integration(4, BLEND)
    eng.set_dynamics(good)
    eng.set_dynamics_integration(2)
    eng.set_dynamics_ensemble([good, good.with_grip(0.6)])
    eng.set_dynamics_integration()
    for bad in (dict(substeps=0), dict(substeps=17), dict(substeps=2.5), dict(low_speed_blend=(5, 3)),
                dict(low_speed_blend=(-1, 3)), dict(low_speed_blend=(np.nan, 3)), dict(low_speed_blend=(1, 2, 3)),
                dict(low_speed_blend=3.0)):
        with pytest.raises(ValueError):
            eng.set_dynamics_integration(**bad)
    eng.close()
    for mode in (0, 1):
        other, _ = _engine(mode=mode)
        with pytest.raises(EngineError) as e:
            other.set_dynamics_integration(4, BLEND)
        assert e.value.code == EINVAL
        other.close()


@pytest.mark.parametrize("bad", [dict(rollout_substeps=0), dict(rollout_substeps=17), dict(low_speed_blend=(5.0, 3.0)),
                                 dict(low_speed_blend=(4.0, 4.0)), dict(low_speed_blend=(-1.0, 3.0)),
                                 dict(low_speed_blend=(float("nan"), 3.0)), dict(low_speed_blend=(3.0, float("inf")))])
def test_solver_config_is_checked_before_any_handle_exists(bad, monkeypatch):
    from acmpc_amd import _capi
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver

    def no_engine(*args, **kwargs):
        raise AssertionError("a handle was created for a config that must be refused")

    monkeypatch.setattr(_capi, "Engine", no_engine)
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(horizon=20, n_candidates=64, **bad))
