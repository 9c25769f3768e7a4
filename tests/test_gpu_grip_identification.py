"""Mode D's grip identification on the MI355X: acmpc_score_grips' errors and best index bit-identical to the restatement
(tests/grip_spec.py) at the smallest shapes that can go wrong, under the default integration and under (4, (3, 5));
non-finite logs, ties, no side effect on a later solve; and the closed loop of test_gpu_dynamic_ensemble.py on the road
with half the grip, with NOTHING in the config naming that grip: the solver finds it from its own driving."""
import numpy as np
import pytest

import grip_spec as gs
from dynamic_spec import Settings
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
                               settings=Settings(substeps=integration[0], low_speed_blend=integration[1]))
    if integration != (1, None):
        assert states[:, 0].max() > 5.0 and states[:, 0].min() < 3.0 or W == 1      # the log crosses the blend
    _same_bits(errors, want)
    assert best == want_best
    assert np.isfinite(want).all()
    eng.close()


# ---- the launch at its thresholds ---------------------------------------------------------------------------------------
# identify_grip_kernel's workgroup (x, y) rolls the run of segments [y run, min((y + 1) run, S)); run = 1 up to 2 048
# workgroups, that is whenever K <= 1 024 and S <= 2048 / blocks.  Every shape below is asserted through
# `describe_score_grips` - the launcher's own numbers (tests/test_grip_identification.py has them as literals) - and then
# compared bit for bit with the restatement, the best index included.
# (W, L, K): dict(blocks, rows, run, grid_y, last_run = segments in the last run, last_segment = steps in the last segment)
RUN_SHAPES = {
    (512, 1, 1024): dict(segments=512, blocks=4, rows=512, run=1, grid_y=512, last_run=1, last_segment=1),    # the last with run = 1
    (205, 1, 2305): dict(segments=205, blocks=10, rows=204, run=2, grid_y=103, last_run=1, last_segment=1),   # a last run of one
    (409, 2, 2305): dict(segments=205, blocks=10, rows=204, run=2, grid_y=103, last_run=1, last_segment=1),   # ... of one step
    (409, 1, 2305): dict(segments=409, blocks=10, rows=204, run=3, grid_y=137, last_run=1, last_segment=1),   # run = 3, ragged
    (511, 1, 1025): dict(segments=511, blocks=5, rows=409, run=2, grid_y=256, last_run=1, last_segment=1),
}
RUN_CASES = [(shape, (1, None)) for shape in RUN_SHAPES] + [((205, 1, 2305), (4, (3.0, 5.0)))]


@pytest.mark.parametrize("shape,integration", RUN_CASES,
                         ids=["W%d_L%d_K%d-%s" % (*s, "default" if i == (1, None) else "fine") for s, i in RUN_CASES])
def test_runs_of_segments_are_the_specification(shape, integration):
    """The restatement of these shapes takes 1.4 .. 2.9 s on one slow core under the default integration and 6.4 s under the
    fine one (4 sub-steps: four times the arithmetic), which is why only the smallest shape with run > 1 runs there; on the
    MI355X host the whole cases took 0.4 .. 1.0 s and 2.1 s."""
    W, L, K = shape
    states, controls = _log(W, slow=integration != (1, None))
    scales = _scales(K)
    eng = _engine(integration)
    try:
        assert eng.describe_score_grips(W, L, K) == RUN_SHAPES[shape]
        errors, best = eng.score_grips(states, controls, HANDLE_DT, scales, segment=L)
    finally:
        eng.close()
    want, want_best = gs.score(_vehicle0().coefficients(), states, controls, HANDLE_DT, scales, segment=L,
                               settings=Settings(substeps=integration[0], low_speed_blend=integration[1]))
    assert np.isfinite(want).all()
    _same_bits(errors, want)
    assert best == want_best


@pytest.mark.parametrize("variant", ["coupled", "loaded", "aero"])
def test_runs_of_segments_in_the_other_three_kernels(variant):
    """identify_grip_coupled_kernel, _loaded_kernel and _aero_kernel each hold the run's lines again: (205, 1, 2305) - run = 2,
    a last run of one segment - under the coupling alone, the load transfer and the downforce, each against its own
    restatement on its own module's log (1.4 .. 1.5 s each on one core)."""
    import test_gpu_dynamic_coupling as tgc
    import test_gpu_dynamic_downforce as tgf
    import test_gpu_dynamic_load_transfer as tgl
    W, L, K = shape = (205, 1, 2305)
    ratio = (0.9, 1.1)
    scales = _scales(K)
    if variant == "coupled":
        states, controls = tgc._braking_log(W)
        want, want_best = gs.score(tgc._vehicle().coefficients(), states, controls, 0.05, scales, segment=L,
                                   settings=Settings(coupling=ratio))
    elif variant == "loaded":
        states, controls = tgl._braking_log(W)
        want, want_best = gs.score(tgl._vehicle().coefficients(), states, controls, 0.05, scales, segment=L,
                                   settings=Settings(coupling=ratio, load_transfer=tgl.LOAD))
    else:
        states, controls = tgf._fast_log(W)
        want, want_best = gs.score(tgf._vehicle().coefficients(), states, controls, 0.05, scales, segment=L,
                                   settings=Settings(coupling=ratio, load_transfer=tgf.LOAD, downforce=tgf.AERO))
    eng = _engine()
    try:
        assert eng.describe_score_grips(W, L, K) == RUN_SHAPES[shape]
        before = [eng.score_grips(states, controls, 0.05, scales, segment=L)[0]]     # the kernels this variant is built on
        eng.set_dynamics_coupling(ratio)
        if variant != "coupled":
            before.append(eng.score_grips(states, controls, 0.05, scales, segment=L)[0])
            eng.set_dynamics_load_transfer(tgl.LOAD if variant == "loaded" else tgf.LOAD)
        if variant == "aero":
            before.append(eng.score_grips(states, controls, 0.05, scales, segment=L)[0])
            eng.set_dynamics_downforce(tgf.AERO)
        errors, best = eng.score_grips(states, controls, 0.05, scales, segment=L)
    finally:
        eng.close()
    assert np.isfinite(want).all()
    _same_bits(errors, want)
    assert best == want_best
    for earlier in before:          # the setting is in these errors
        assert not np.array_equal(errors.view(np.uint32), earlier.view(np.uint32))


def test_the_best_of_65_partial_keys():
    """K = 16 385 is 65 workgroups, so identify_best_kernel's lanes go round their loop twice: the true vehicle alone in the
    65th workgroup, then three times - the lowest index wins across the passes."""
    W, L, K = 5, 2, 16385
    states, controls = gs.steering_log(_vehicle0().with_axle_grip(0.5, 0.7), 0.02, steps=W)
    scales = _scales(K, seed=5)
    scales[16384] = (0.5, 0.7)
    eng = _engine()
    try:
        assert eng.describe_score_grips(W, L, K) == dict(segments=3, blocks=65, rows=3, run=1, grid_y=3, last_run=1, last_segment=1)
        errors, best = eng.score_grips(states, controls, HANDLE_DT, scales, segment=L)
        want, want_best = gs.score(_vehicle0().coefficients(), states, controls, HANDLE_DT, scales, segment=L)
        _same_bits(errors, want)
        assert best == want_best == 16384 and errors[16384] < np.delete(errors, 16384).min()
        scales[[300, 9000]] = (0.5, 0.7)
        errors, best = eng.score_grips(states, controls, HANDLE_DT, scales, segment=L)
        assert best == 300 and errors[300] == errors[16384] == errors[9000] == errors.min()
        assert np.count_nonzero(errors == errors.min()) == 3
    finally:
        eng.close()


def test_the_limits_65536_hypotheses_and_two_to_the_22_values():
    """K = 65 536 and S K = 2^22: 256 workgroups along the hypotheses (256 partial keys), runs of 8 segments.  The whole
    restatement would take 17 s, so: the errors are those of the same hypotheses scored 1 024 at a time (run = 1, tied to
    the restatement above); they are the restatement's on every workgroup's first and last lane and every 97th
    hypothesis; and the best index is the key rule over the device's own errors, the minimum planted in the last workgroup."""
    import acmpc_oracle as orc
    W, L, K = 64, 1, 65536
    states, controls = gs.steering_log(_vehicle0().with_axle_grip(0.5, 0.7), 0.02, steps=W)
    scales = _scales(K, seed=6)
    scales[K - 100] = (0.5, 0.7)
    eng = _engine()
    try:
        assert eng.describe_score_grips(W, L, K) == dict(segments=64, blocks=256, rows=8, run=8, grid_y=8, last_run=8, last_segment=1)
        assert eng.describe_score_grips(W, L, 1024) == dict(segments=64, blocks=4, rows=64, run=1, grid_y=64, last_run=1, last_segment=1)
        errors, best = eng.score_grips(states, controls, HANDLE_DT, scales, segment=L)
        pieces = [eng.score_grips(states, controls, HANDLE_DT, scales[k:k + 1024], segment=L)[0] for k in range(0, K, 1024)]
    finally:
        eng.close()
    _same_bits(errors, np.concatenate(pieces))
    subset = np.unique(np.concatenate([np.arange(0, K, 256), np.arange(255, K, 256), np.arange(0, K, 97), [K - 100]]))
    want, _ = gs.score(_vehicle0().coefficients(), states, controls, HANDLE_DT, scales[subset], segment=L)
    assert np.isfinite(want).all()
    _same_bits(errors[subset], want)
    assert best == int(orc.pick_best(errors)[0]) == K - 100


def test_a_larger_call_after_a_smaller_one_and_back():
    """The per-segment scratch e [S][K] grows with the call: S K = 3, then 2^20 (64 workgroups, runs of 2), then 3 again on
    one handle, each the bits of a fresh handle."""
    calls = [(3, 1, 1), (64, 1, 16384), (3, 1, 1)]
    inputs = [(_log(W, slow=False, seed=i), _scales(K, seed=i)) for i, (W, L, K) in enumerate(calls)]

    def run(eng, i):
        (states, controls), scales = inputs[i]
        return eng.score_grips(states, controls, HANDLE_DT, scales, segment=calls[i][1])

    eng = _engine()
    try:
        assert eng.describe_score_grips(*calls[1]) == dict(segments=64, blocks=64, rows=32, run=2, grid_y=32, last_run=2, last_segment=1)
        got = [run(eng, i) for i in range(3)]
    finally:
        eng.close()
    for i in range(3):
        fresh = _engine()
        try:
            errors, best = run(fresh, i)
        finally:
            fresh.close()
        _same_bits(got[i][0], errors)
        assert got[i][1] == best
    for i in (0, 2):
        (states, controls), scales = inputs[i]
        want, want_best = gs.score(_vehicle0().coefficients(), states, controls, HANDLE_DT, scales)
        _same_bits(got[i][0], want)
        assert got[i][1] == want_best


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
