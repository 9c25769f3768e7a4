"""Mode D's plan trace without a device ("Mode D, plan trace"): the float32 restatement
(tests/dynamic_spec.py's trace_plans) against the rollout it records, its hinge replay, the float64 mirror
(dynamic_model.trace) against it, every refusal of acmpc_trace_plans, and the Python wiring up to `rollout_mode: "D"`."""
import copy

import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_fuzz_cases as fz
import dynamic_spec as ds
from dynamic_spec import Settings

T = np.float32
INF = float("inf")
EINVAL, ECAPACITY, ESTATE = -1, -4, -5
K_F, K_R = 7.35e-4, 1.1025e-3


def _vehicle():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams.reference()


def _problem(H=13, N=4, seed=71, track="monza", width=None, **kind):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, track, H, N, seed, **kind)
    if width is not None:
        dp["table"][orc.ROW_WIDTH] = width
    eng = Engine(**dict(dp["kw"], max_problems=1, max_candidates=N, max_steps=H - 1))
    eng.set_paths(dp["table"])
    coef = eng.coefficients(0)
    eng.close()
    return dp, coef


def _rollout(dp, coef, block, window=None, **kwargs):
    kw = dp["kw"]
    return ds.rollout_dynamic(dp["x0"], coef, dp["U"], block, kw["step_cost"], kw["r_term"], kw["final_cost"], kw["u_min"],
                              kw["u_max"], kw["w_bound"], kw["dt"], kw["wheelbase"], nn_window=window, **kwargs)


def _same(a, b):
    return np.array_equal(ds.bits(a), ds.bits(b))


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [None, (2, 5)])
def test_the_default_trace_is_dynamic_specs_rollout(window):
    dp, coef = _problem()
    block = _vehicle().coefficients()
    cost, V, X = _rollout(dp, coef, block, window, return_states=True)
    got = ds.trace_plans(dp, coef, dp["U"], [block], Settings(), window)
    assert _same(got["states"][:, 0, :, :3], X)
    assert _same(got["totals"][:, 0, 0], cost) and _same(got["totals"][:, 0, 1], V)
    assert _same(got["states"][:, 0, 0], np.tile(dp["x0"], (4, 1)))
    assert np.any(V > 0), "candidates 2 and 3 leave the input box"
    assert _same(ds.replay(got["terms"]), got["terms"][..., ds.V_SLOT]) and _same(got["terms"][..., -1, ds.V_SLOT], V[:, None])
    assert not np.any(got["terms"][..., ds.RATE:ds.V_SLOT]) and not np.any(got["terms"][..., ds.E_SLOT])


CASES = [("fine", 0), ("terms", 1), ("objective", 2), ("coupled", 0), ("coupled", 5), ("loaded", 1), ("loaded", 3)]


@pytest.mark.parametrize("family,index", CASES)
def test_with_settings_on_it_is_the_composed_restatement(family, index):
    """Cases of tests/dynamic_fuzz_cases.py: (cost, V, x) of every vehicle and problem bit for bit, and the replay."""
    from acmpc_amd import Engine
    c = fz.case(family, "matrix", index)
    dps = fz.problems(c, orc, limit=6)
    eng = Engine(**dict(dps[0]["kw"], max_problems=c["P"], max_candidates=8, max_steps=c["H"] - 1))
    eng.set_paths(np.stack([d["table"] for d in dps]))
    coefs = [eng.coefficients(p) for p in range(c["P"])]
    eng.close()
    u_prev = fz.previous(c)
    for p, dp in enumerate(dps):
        prev = None if u_prev is None else u_prev[p]
        blocks = [fz.blocks()[v] for v in c["vehicles"]]
        got = ds.trace_plans(dp, coefs[p], dp["U"], blocks, Settings.of_case(c), c["window"], prev)
        for k, block in enumerate(blocks):
            cost, V, X = _rollout(dp, coefs[p], block, c["window"], return_states=True, settings=Settings.of_case(c), u_prev=prev)
            where = np.isfinite(cost)
            assert _same(got["totals"][:, k, 0][where], cost[where]) and _same(got["totals"][:, k, 1][where], V[where])
            assert _same(got["states"][:, k, :, :3][where], X[where])
        finite = np.isfinite(got["terms"][..., ds.V_SLOT]).all(axis=-1)
        assert _same(ds.replay(got["terms"])[finite], got["terms"][..., ds.V_SLOT][finite])
        assert _same(got["terms"][..., -1, ds.V_SLOT], got["totals"][..., 1])


def test_with_obstacles_and_downforce_it_is_the_composed_restatement():
    dp, coef = _problem(seed=72)
    n = 12
    discs = ds.make_obstacles(dp, n, 8, 5, nan="some")
    s = Settings(substeps=2, low_speed_blend=(3.0, 5.0), coupling=(0.9, 1.1), load_transfer=(0.35, 0.9), downforce=(K_F, K_R, 100.0),
                 clearance_weight=40.0, clearance_margin=1.0, rate_weight=(0.3, 0.02), rate_max=(1.5, 6.0), slip_weight=40.0,
                 slip_max=0.08, progress_weight=3.0, speed_ceiling=(1.05, 0.0))
    block = _vehicle().coefficients()
    got = ds.trace_plans(dp, coef, dp["U"], [block], s, (2, 5), (0.01, 0.2), discs)
    cost, V, X = _rollout(dp, coef, block, (2, 5), return_states=True, settings=s, u_prev=(0.01, 0.2), obstacles=discs)
    assert _same(got["totals"][:, 0, 0], cost) and _same(got["totals"][:, 0, 1], V) and _same(got["states"][:, 0, :, :3], X)
    assert _same(ds.replay(got["terms"]), got["terms"][..., ds.V_SLOT])
    terms = got["terms"]
    assert np.any(terms[..., ds.DISCS:ds.V_SLOT] != 0) and np.any(terms[..., ds.RATE] != 0) and np.any(terms[..., ds.E_SLOT] != 0)


# ---- the float64 mirror ----------------------------------------------------------------------------------------------------------
# Worst |float64 mirror - float32 restatement| over the committed cases below, sixteen runs of four plans and twelve steps (this
# file's __main__ prints them): the six states 3.9e-6 (3.82e-6 measured, under the coupling with four sub-steps), the hinges
# and the cost lines' operands 4.3e-6 (4.24e-6, under the load transfer and the downforce).  Held at 4x the measured value, the
# project's convention.  The nearest hinge of the float64 side sits 6.9e-5 from its kink.
STATE_TOL, HINGE_TOL = 4 * 3.9e-6, 4 * 4.3e-6
MIRROR_WIDTH = 1.0                         # metres: narrow enough for the plans to leave the corridor
MIRROR_TERMS = dict(rate_weight=(0.3, 0.02), rate_max=(1.5, 6.0), slip_weight=40.0, slip_max=0.005)
MIRROR_CASES = {
    "default": Settings(),
    "terms": Settings(speed_ceiling=(0.98, 0.0), **MIRROR_TERMS),
    "fine-coupled": Settings(substeps=4, low_speed_blend=(3.0, 5.0), coupling=(0.9, 1.1), **MIRROR_TERMS),
    "loaded-aero": Settings(substeps=2, coupling=(0.9, 1.1), load_transfer=(0.35, 0.9), downforce=(K_F, K_R, 100.0),
                            progress_weight=3.0, speed_ceiling=(0.98, 0.0)),
}


def _mirror(name, window, with_discs):
    from acmpc_amd.dynamic_model import trace
    s = MIRROR_CASES[name]
    dp, coef = _problem(seed=73, width=MIRROR_WIDTH)
    n = 12
    kw = dp["kw"]
    discs = ds.make_obstacles(dp, n, 3, 9) if with_discs else None
    u_prev = (0.01, 0.2)
    f32 = ds.trace_plans(dp, coef, dp["U"], [_vehicle().coefficients()], s, window, u_prev, discs)
    worst = dict(state=0.0, hinge=0.0, kink=INF)
    binds = np.zeros(15, dtype=bool)
    for m in range(dp["U"].shape[0]):
        f64 = trace(_vehicle(), dp["x0"].astype(np.float64), dp["U"][m].astype(np.float64), dp["table"], kw["dt"],
                    u_min=kw["u_min"], u_max=kw["u_max"], margin=kw["margin"], wheelbase=kw["wheelbase"], nn_window=window,
                    substeps=s.substeps, low_speed_blend=s.low_speed_blend, coupling=s.coupling,
                    load_transfer=s.load_transfer, downforce=s.downforce, u_prev=u_prev, rate_max=s.rate_max, slip_max=s.slip_max,
                    speed_ceiling=s.speed_ceiling, obstacles=None if discs is None else discs[0],
                    radii=None if discs is None else discs[1])
        row = f32["terms"][m, 0].astype(np.float64)
        assert np.array_equal(f64["j"], row[:, ds.J].astype(np.int64)), (name, m)
        hinges = np.concatenate([f64["box"], f64["corridor"][:, None], f64["rate"], f64["slip"][:, None],
                                 f64["ceiling"][:, None], f64["obstacles"]], axis=1)
        worst["state"] = max(worst["state"], float(np.abs(f64["states"] - f32["states"][m, 0]).max()))
        worst["hinge"] = max(worst["hinge"], float(np.abs(hinges - row[:, ds.HINGES]).max()))
        worst["kink"] = min(worst["kink"], float(f64["kink"].min()))
        binds |= (hinges != 0).any(axis=0)
        for key, slot in (("e_y", ds.EY), ("e_psi", ds.EPSI), ("dv", ds.DV), ("dk", ds.DK)):
            worst["hinge"] = max(worst["hinge"], float(np.abs(f64[key] - row[:, slot]).max()))
    return worst, binds


@pytest.mark.parametrize("with_discs", [False, True], ids=["no-discs", "discs"])
@pytest.mark.parametrize("window", [None, (2, 5)], ids=["all", "window"])
@pytest.mark.parametrize("name", list(MIRROR_CASES))
def test_the_float64_mirror_against_the_restatement(name, window, with_discs):
    worst, _ = _mirror(name, window, with_discs)
    # the float64 side alone keeps the case: no hinge of it sits within the tolerance of its kink
    assert worst["kink"] > HINGE_TOL, (name, worst)
    assert worst["state"] <= STATE_TOL and worst["hinge"] <= HINGE_TOL, (name, worst)


def test_the_mirror_cases_bind():
    """Over the cases every kind of hinge is non-zero somewhere: the comparison above is not one of zeros."""
    seen = np.zeros(15, dtype=bool)
    for name in MIRROR_CASES:
        seen |= _mirror(name, None, True)[1]
    assert seen[:7].all() and seen[7:10].any(), seen


@pytest.mark.parametrize("window", [None, (2, 5)], ids=["all", "window"])
def test_the_mirror_is_the_existing_float64_terms_step_by_step(window):
    """dynamic_model.trace's hinges, squared and summed, are what stage_terms, objective_terms and clearance_terms return for
    the same rollout (plus the box and the corridor, which have no function of their own)."""
    from acmpc_amd.dynamic_model import clearance_terms, objective_terms, stage_terms, trace
    s = MIRROR_CASES["fine-coupled"]
    dp, _ = _problem(seed=73, width=MIRROR_WIDTH)
    kw, n = dp["kw"], 12
    discs = ds.make_obstacles(dp, n, 3, 9)
    u_prev, ceiling = (0.01, 0.2), (0.98, 0.0)
    bound = np.zeros(3)
    for U in dp["U"].astype(np.float64):
        t = trace(_vehicle(), dp["x0"].astype(np.float64), U, dp["table"], kw["dt"], u_min=kw["u_min"], u_max=kw["u_max"],
                  margin=kw["margin"], wheelbase=kw["wheelbase"], nn_window=window, substeps=s.substeps, low_speed_blend=s.low_speed_blend,
                  coupling=s.coupling, u_prev=u_prev, rate_max=MIRROR_TERMS["rate_max"], slip_max=MIRROR_TERMS["slip_max"],
                  speed_ceiling=ceiling, obstacles=discs[0], radii=discs[1])
        np.testing.assert_array_equal(t["states"], _vehicle().rollout(dp["x0"].astype(np.float64), U, kw["dt"], substeps=s.substeps,
                                                                      low_speed_blend=s.low_speed_blend, coupling=s.coupling))
        V_terms = stage_terms(t["states"], U, kw["dt"], u_prev, _vehicle(), rate_max=MIRROR_TERMS["rate_max"],
                              slip_max=MIRROR_TERMS["slip_max"])[1]
        V_ceiling = objective_terms(t["states"], U, dp["table"], speed_ceiling=ceiling, nn_window=window)[1]
        V_discs = clearance_terms(t["states"][1:, :2], discs[0], discs[1])[1]
        np.testing.assert_allclose(np.sum(t["rate"] ** 2) + np.sum(t["slip"] ** 2), V_terms, rtol=1e-12)
        np.testing.assert_allclose(np.sum(t["ceiling"] ** 2), V_ceiling, rtol=1e-12)
        np.testing.assert_allclose(np.sum(t["obstacles"] ** 2), V_discs, rtol=1e-12)
        total = np.sum(t["box"] ** 2) + np.sum(t["corridor"] ** 2) + V_terms + V_ceiling + V_discs
        np.testing.assert_allclose(t["V"][-1], total, rtol=1e-12)
        bound += (V_terms, V_ceiling, V_discs)
    assert np.all(bound > 0), bound


# ---- refusals (no device work) ---------------------------------------------------------------------------------------------------
def _engine(mode=2, P=2, n=5, M_cap=4):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", n + 1, 4, 21)
    return Engine(**dict(dp["kw"], mode=mode, max_problems=P, max_candidates=M_cap, max_steps=n)), dp


def _code(eng, x0, U, P, M, n, outputs=(True, True, True)):
    K = max(eng.K, 1)
    rolls = P * M * K if min(P, M, n) > 0 and P * M * K * n < 1 << 16 else 0   # (a refused call writes nothing: any buffer will do)
    arrays = tuple(np.zeros(max(rolls * per, 1), dtype=T) for per in ((n + 1) * 6, 2, n * 22))
    return eng._lib.acmpc_trace_plans(eng._ctx, None if x0 is None else x0.ctypes.data, None if U is None else U.ctypes.data, P, M, n,
                                      *(a.ctypes.data if on else None for a, on in zip(arrays, outputs)))


def test_every_refusal_of_the_entry_point():
    from acmpc_amd import EngineError, _capi
    lib = _capi.load_library()
    assert "acmpc_trace_plans" in _capi.SIGNATURES and hasattr(lib, "acmpc_trace_plans")
    P, n, M = 2, 5, 3
    x0, U = np.zeros((P, 6), dtype=T), np.zeros((P, M, n, 2), dtype=T)
    assert lib.acmpc_trace_plans(None, x0.ctypes.data, U.ctypes.data, P, M, n, None, None, None) == EINVAL
    # a mode S / T handle, or no vehicle
    for mode in (0, 1):
        other, dp = _engine(mode=mode)
        other.set_paths(np.stack([dp["table"]] * P))
        assert _code(other, x0[:, :3].copy(), U, P, M, n) == ESTATE
        other.close()
    eng, dp = _engine()
    eng.set_paths(np.stack([dp["table"]] * P))
    assert _code(eng, x0, U, P, M, n) == ESTATE and b"acmpc_set_dynamics" in lib.acmpc_last_error(eng._ctx)
    eng.set_dynamics(_vehicle())
    # null inputs, three null outputs, shapes below 1
    assert _code(eng, None, U, P, M, n) == EINVAL and _code(eng, x0, None, P, M, n) == EINVAL
    assert _code(eng, x0, U, P, M, n, outputs=(False, False, False)) == EINVAL
    assert _code(eng, x0, U, 0, M, n) == EINVAL and _code(eng, x0, U, P, 0, n) == EINVAL and _code(eng, x0, U, P, M, 0) == EINVAL
    assert _code(eng, x0, U, -1, M, n) == EINVAL and _code(eng, x0, U, P, -3, n) == EINVAL
    # beyond the handle's capacity; outputs beyond 1 GiB (M is not bounded by max_candidates: the scratch is the call's own)
    assert _code(eng, x0, U, P + 1, M, n) == ECAPACITY and _code(eng, x0, U, P, M, n + 1) == ECAPACITY
    huge = (1 << 30) // (4 * P * (n * 22 + (n + 1) * 6 + 2)) + 1
    assert _code(eng, x0, U, P, huge, n, outputs=(False, True, False)) == ECAPACITY
    assert b"1 GiB" in lib.acmpc_last_error(eng._ctx)
    # the paths': none set, or another shape
    bare, _ = _engine()
    bare.set_dynamics(_vehicle())
    assert _code(bare, x0, U, P, M, n) == ESTATE and b"acmpc_set_paths" in lib.acmpc_last_error(bare._ctx)
    bare.close()
    assert _code(eng, x0, U, 1, M, n) == EINVAL and _code(eng, x0, U, P, M, n - 1) == EINVAL
    # stored previous controls or obstacles of another shape
    eng.set_previous_control(np.zeros((1, 2), dtype=T))
    assert _code(eng, x0, U, P, M, n) == ESTATE and b"acmpc_set_previous_control" in lib.acmpc_last_error(eng._ctx)
    eng.set_previous_control(None)
    eng.set_obstacles(np.zeros((P, n - 1, 2, 2), dtype=T), np.ones((P, 2), dtype=T))
    assert _code(eng, x0, U, P, M, n) == ESTATE and b"acmpc_set_obstacles" in lib.acmpc_last_error(eng._ctx)
    eng.set_obstacles(None)
    # after all of it the handle takes the call as far as the device (or runs it)
    assert _code(eng, x0, U, P, M, n) not in (EINVAL, ECAPACITY, ESTATE)
    with pytest.raises(ValueError):
        eng.trace_plans(x0, U[..., :1])
    with pytest.raises(EngineError) as e:
        eng.trace_plans(x0[:1], U[:1])
    assert e.value.code == EINVAL
    eng.close()


# ---- Python wiring ---------------------------------------------------------------------------------------------------------------
def test_unpack_decision_dynamic_on_a_hand_made_plan():
    from acmpc_amd import _capi
    n, dt = 4, 0.05
    states = np.arange(6 * (n + 1), dtype=np.float64).reshape(n + 1, 6)
    u = np.array([[0.1, 0.5], [0.2, -0.5], [0.0, 0.25], [-0.1, 1.0]])
    pc, pred, cum, times, acc, rates, pedal = _capi.unpack_decision_dynamic(states, u, dt)
    assert pc.dtype == np.float64 and pc.shape == (2, n)
    np.testing.assert_array_equal(pc[0], states[1:, 3])         # the speed reached UNDER control i
    np.testing.assert_array_equal(pc[1], u[:, 0])
    np.testing.assert_array_equal(pred, states[:n, :2])
    np.testing.assert_array_equal(cum, dt * np.arange(n))
    np.testing.assert_array_equal(times, np.full(n - 1, dt))
    np.testing.assert_allclose(acc, np.full(n - 1, 6.0 / dt), rtol=1e-15)
    np.testing.assert_allclose(rates, np.diff(u[:, 0]) / dt, rtol=1e-15)
    np.testing.assert_array_equal(pedal, u[:, 1])
    with pytest.raises(ValueError):
        _capi.unpack_decision_dynamic(states[:n], u, dt)


def _control_config(**over):
    from acmpc_amd import workloads
    cfg = copy.deepcopy(workloads.RACING_CONTROL["monza"])
    cfg.update(n_candidates=64, **over)
    return cfg


def test_rollout_mode_d_constructs_and_the_others_are_named():
    from acmpc_amd import workloads
    from acmpc_amd.mpc import build_mpc
    from acmpc_amd.sampling_solver import ControlSolver
    from acmpc_amd.bicycle_model import SpatialBicycleModel
    cfg = _control_config(rollout_mode="D", tyre_coupling=(0.9, 1.1), rollout_substeps=2)
    limits = cfg["speed_profile_constraints"]
    model = SpatialBicycleModel(workloads.PlaceholderVehicle(), {"max": limits["v_max"], "min": limits["v_min"]})
    solver = ControlSolver(cfg, model)
    assert solver.dynamic and not solver.temporal and not solver.supports_tick()
    assert solver.dynamic_solver._plan_states and solver.dynamic_solver.engine.params.margin == model.margin
    with pytest.raises(ValueError, match="'S', 'T' or 'D'"):
        ControlSolver(_control_config(rollout_mode="X"), model)
    block = _vehicle().with_grip(0.8).coefficients()
    mpc = build_mpc(_control_config(rollout_mode="D", dynamic_vehicle=block), workloads.PlaceholderVehicle())
    H = cfg["horizon"]
    path = np.stack([np.zeros(H), np.linspace(0.0, 2.0 * H, H), np.full(H, 8.0)], axis=1)
    with pytest.raises(ValueError, match="motion"):
        mpc.get_control(path)
    with pytest.raises(ValueError):
        mpc.get_control_at(0)
    for mode in ("S", "T"):
        assert not ControlSolver(_control_config(rollout_mode=mode), model).dynamic


def test_plan_states_is_off_by_default(monkeypatch):
    """solve() with the key off makes no trace call and leaves no `.states`; with it on, one call on the winner."""
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    n = 9
    table = np.zeros((7, n))
    table[1] = np.arange(n)
    for on in (False, True):
        solver = DynamicSamplingSolver(dict(horizon=n + 1, n_candidates=8, plan_states=on))
        calls = []
        fake = dict(u=np.full((1, n, 2), 0.25, dtype=T), x=np.zeros((1, n + 1, 3), dtype=T), cost=np.ones(1, dtype=T),
                    violation=np.zeros(1, dtype=T), n_feasible=np.ones(1))
        monkeypatch.setattr(solver.engine, "optimize", lambda *a, **k: fake)
        monkeypatch.setattr(solver.engine, "trace_plans",
                            lambda x0, U, want=None: calls.append((x0, U, want)) or dict(states=np.ones((1, 1, 1, n + 1, 6), dtype=T)))
        obj = solver.solve(np.zeros(6), table)
        assert hasattr(obj, "states") == on and len(calls) == int(on)
        if on:
            assert obj.states.shape == (n + 1, 6) and calls[0][1].shape == (1, 1, n, 2) and calls[0][2] == ("states",)
        np.testing.assert_array_equal(solver.warm_start(), np.full((n, 2), 0.25, dtype=T))
        solver._plan = np.arange(2 * n, dtype=T).reshape(n, 2)
        np.testing.assert_array_equal(solver.warm_start(3)[:n - 3], solver._plan[3:])
        np.testing.assert_array_equal(solver.warm_start(3)[n - 3:], np.tile(solver._plan[-1], (3, 1)))
        np.testing.assert_array_equal(solver.warm_start(), solver.warm_start(1))
        np.testing.assert_array_equal(solver.warm_start(99), np.tile(solver._plan[-1], (n, 1)))
        np.testing.assert_array_equal(solver.warm_start(0), solver._plan)
        solver.close()


if __name__ == "__main__":
    for name in MIRROR_CASES:
        for window in (None, (2, 5)):
            for with_discs in (False, True):
                print(name, window, with_discs, _mirror(name, window, with_discs)[0])
