"""Mode D's grip identification on the MI355X: acmpc_score_grips' errors and best index bit-identical to the restatement
(tests/grip_spec.py) at the smallest shapes that can go wrong, under the default integration and under (4, (3, 5));
non-finite logs, ties, no side effect on a later solve; and the closed loop of test_gpu_dynamic_ensemble.py on the road
with half the grip, with NOTHING in the config naming that grip: the solver finds it from its own driving."""
import numpy as np
import pytest

import grip_spec as gs
import test_gpu_dynamic as tgd
import test_gpu_dynamic_ensemble as tge

pytestmark = pytest.mark.gpu

HANDLE_DT = 0.05
# (W, L, K): the smallest call | a few short segments | ragged last segment, K across a wavefront | K across a 256-lane
# workgroup | one segment | the typical window on the 25 x 25 grid | the step limit | the segment limit
SHAPES = [(1, 1, 1), (5, 1, 3), (7, 3, 65), (33, 8, 257), (12, 12, 64), (40, 1, 625), (512, 512, 2), (512, 1, 2)]
INTEGRATIONS = [(1, None), (4, (3.0, 5.0))]
UNEQUAL_WEIGHTS = {(33, 8, 257): (1.0, 4.0, 0.25)}
OTHER_DT = {(7, 3, 65): 0.02}            # the log's period is not the handle's


def _vehicle0():
    from acmpc_amd import DynamicBicycleParams
    return DynamicBicycleParams.reference()


def _engine(integration=(1, None)):
    from acmpc_amd import Engine, _capi
    eng = Engine(mode=_capi.MODE_DYNAMIC, max_problems=1, max_candidates=64, max_steps=8, step_cost=(1.0, 1.0, 0.0),
                 r_term=(0.5, 10.0), final_cost=(1.0, 1.0, 0.0), u_min=(-0.3, -1.0), u_max=(0.3, 1.0), margin=0.0,
                 wheelbase=2.898, dt=HANDLE_DT)
    eng.set_dynamics(_vehicle0())
    if integration != (1, None):
        eng.set_dynamics_integration(*integration)
    return eng


def _log(W, slow, seed=0):
    """A synthetic log (it need not be any vehicle's): at speed for the default integration - whose single Euler step is
    only stable there - and, `slow`, one whose vx falls from 6.5 m/s through the blend's 3 .. 5 m/s."""
    rng = np.random.default_rng(100 + seed + W)
    t = np.arange(W + 1) * 0.05
    if slow:
        vx = np.linspace(6.5, 2.0, W + 1) if W > 1 else np.array([4.5, 4.2])
        pedal = np.full(W, -0.08)
    else:
        vx = 28.0 + 1.5 * np.sin(0.3 * t)
        pedal = np.full(W, 0.3)
    states = np.stack([vx, 0.05 * np.sin(2.0 * t) + 0.01 * rng.standard_normal(W + 1),
                       0.1 * np.sin(2.0 * t + 0.4) + 0.01 * rng.standard_normal(W + 1)], axis=1)
    controls = np.stack([0.02 * np.sin(np.pi * t[:W]) + 0.01, pedal + 0.05 * rng.standard_normal(W)], axis=1)
    return states.astype(np.float32), controls.astype(np.float32)


def _scales(K, seed=0):
    rng = np.random.default_rng(200 + seed + K)
    scales = rng.uniform(0.3, 1.5, (K, 2))
    scales[0] = (1.0, 1.0)
    return scales


def _same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize("integration", INTEGRATIONS, ids=["default", "fine"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "W%d_L%d_K%d" % s)
def test_errors_and_best_are_the_specification(shape, integration):
    W, L, K = shape
    states, controls = _log(W, slow=integration != (1, None))
    scales = _scales(K)
    weights = UNEQUAL_WEIGHTS.get(shape, (1.0, 1.0, 1.0))
    dt = OTHER_DT.get(shape, HANDLE_DT)
    eng = _engine(integration)
    errors, best = eng.score_grips(states, controls, dt, scales, segment=L, weights=weights)
    want, want_best = gs.score(_vehicle0().coefficients(), states, controls, dt, scales, segment=L, weights=weights,
                               substeps=integration[0], low_speed_blend=integration[1])
    if integration != (1, None):
        assert states[:, 0].max() > 5.0 and states[:, 0].min() < 3.0 or W == 1      # the log crosses the blend
    _same_bits(errors, want)
    assert best == want_best
    assert np.isfinite(want).all()
    eng.close()


def test_a_nan_in_the_log_makes_every_error_nan():
    states, controls = _log(5, slow=False)
    states[2, 0] = np.nan
    eng = _engine()
    errors, best = eng.score_grips(states, controls, HANDLE_DT, _scales(3))
    assert np.isnan(errors).all() and best == 0
    want, want_best = gs.score(_vehicle0().coefficients(), states, controls, HANDLE_DT, _scales(3))
    assert np.isnan(want).all() and want_best == 0
    eng.close()


def test_an_inf_in_a_control_of_the_last_segment_is_the_specification():
    states, controls = _log(7, slow=False)
    controls[6, 0] = np.inf
    scales = _scales(65)
    eng = _engine()
    errors, best = eng.score_grips(states, controls, HANDLE_DT, scales, segment=3)
    want, want_best = gs.score(_vehicle0().coefficients(), states, controls, HANDLE_DT, scales, segment=3)
    _same_bits(errors, want)
    assert best == want_best
    eng.close()


def test_duplicate_hypotheses_give_the_lower_index():
    states, controls = gs.steering_log(_vehicle0().with_axle_grip(0.5, 0.7), 0.02)
    scales = _scales(300, seed=5)
    scales[[7, 130, 299]] = (0.5, 0.7)          # the true vehicle three times, in two workgroups
    eng = _engine()
    errors, best = eng.score_grips(states, controls, HANDLE_DT, scales)
    assert best == 7 and errors[7] == errors[130] == errors[299] == errors.min()
    eng.close()


@pytest.mark.parametrize("ensemble", [False, True], ids=["one_vehicle", "four_vehicles_and_terms"])
def test_a_solve_gives_the_same_bits_before_and_after(ensemble):
    P, N, n = 2, 512, 30
    dps = tgd._problems(P, N, n, seed=60)
    eng = tgd._engine(dps, P, N, n, (2, 5))
    if ensemble:
        vs = tge._vehicles()
        eng.set_dynamics_ensemble([vs[i] for i in (0, 1, 2, 4)], reduce="mean")
        eng.set_dynamics_terms(rate_weight=(5.0, 0.1), rate_max=(2.0, None), slip_weight=10.0, slip_max=0.2)
        eng.set_previous_control(np.array([[0.01, 0.1], [0.0, -0.2]], dtype=np.float32))
    x0 = np.stack([d["x0"] for d in dps])
    U = np.stack([d["U"] for d in dps])
    before = eng.solve(x0, U)
    states, controls = gs.steering_log(_vehicle0().with_grip(0.5), 0.02)
    errors, best = eng.score_grips(states, controls, HANDLE_DT, _scales(625), segment=8)
    assert np.isfinite(errors).all()
    after = eng.solve(x0, U)
    tgd._same_bits(after["costs"], before["costs"])
    tgd._same_bits(after["records"], before["records"])
    assert list(after["best_idx"]) == list(before["best_idx"])
    eng.close()


# ---- closed loop: the road's grip found from the drive ---------------------------------------------------------------
ADAPT = dict(axles="tied", grid=tuple(0.3 + 0.05 * np.arange(25)))       # 0.3 .. 1.5, step 0.05
GRID_STEP = 0.05


def _adaptive_loop(plant):
    """test_gpu_dynamic's loop with LOOP_CONFIG + grip_adapt: (log, the estimates of every tick)."""
    from acmpc_amd import DynamicBicycleParams, DynamicSamplingSolver
    solver = DynamicSamplingSolver(dict(tgd.LOOP_CONFIG, grip_adapt=ADAPT), DynamicBicycleParams.reference())
    estimates = []

    def solve(state, table):
        obj = solver.solve(state, table)
        estimates.append((solver.grip.front, solver.grip.accepted))
        return obj

    try:
        log = tgd.run_loop(solve, plant)
    finally:
        solver.close()
    return log, estimates


def test_the_adaptive_solver_holds_the_road_with_half_the_grip():
    """The plant has half the nominal grip and nothing tells the solver: it starts on the nominal vehicle, identifies the
    grip from its own logged driving and holds the bars the told-the-truth ensemble (0.4, 0.6) holds there."""
    from acmpc_amd import DynamicBicycleParams
    assert "grip_ensemble" not in tgd.LOOP_CONFIG and tge.LOOP_GRIP == 0.5
    log, estimates = _adaptive_loop(DynamicBicycleParams.reference().with_grip(tge.LOOP_GRIP))
    ey, slip, dv, idx = log.T
    accepted = [front for front, ok in estimates if ok]
    print("adaptive loop on grip 0.5: max |e_y| %.3f m, max sideslip %.4f, travelled %d waypoints, %d accepted estimates, "
          "first accepted at tick %d, final %r" % (np.abs(ey).max(), slip.max(), (idx[-1] - idx[0]) % 11586, len(accepted),
                                                     [ok for _, ok in estimates].index(True) if accepted else -1,
                                                     estimates[-1][0]))
    assert accepted, "no estimate was accepted"
    assert abs(estimates[-1][0] - tge.LOOP_GRIP) <= GRID_STEP + 1e-9
    assert np.abs(ey).max() < tgd.LOOP_CORRIDOR, "left the corridor: |e_y| %.2f m" % np.abs(ey).max()
    assert slip.max() < tgd.LOOP_SLIP, "sideslip %.4f" % slip.max()
    assert (idx[-1] - idx[0]) % 11586 > 1000                  # > 500 m, through the tightest corner


def test_the_adaptive_solver_leaves_the_nominal_road_alone():
    from acmpc_amd import DynamicBicycleParams
    log, estimates = _adaptive_loop(DynamicBicycleParams.reference())
    ey, slip, dv, idx = log.T
    print("adaptive loop on grip 1.0: max |e_y| %.3f m, max sideslip %.4f, final %r" % (np.abs(ey).max(), slip.max(),
                                                                                       estimates[-1][0]))
    assert estimates[-1][0] is not None and abs(estimates[-1][0] - 1.0) <= GRID_STEP + 1e-9
    assert np.abs(ey).max() < tgd.LOOP_CORRIDOR, "left the corridor: |e_y| %.2f m" % np.abs(ey).max()
    assert slip.max() < tgd.LOOP_SLIP, "sideslip %.4f" % slip.max()
