"""Mode D's obstacles on the CPU ("Mode D, obstacles"): the float32 restatement
(tests/dynamic_spec.py) against the float64 mirror (acmpc_amd.dynamic_model.clearance_terms on
tests/dynamic_reference64.py's states), the order and the switches of its lines, the disc at the candidate's own position,
predict_obstacles against its definition, and the refusals of acmpc_set_obstacles / acmpc_set_dynamics_clearance on a
handle without a device."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_fuzz_cases as fz
import dynamic_reference64 as r64
import dynamic_spec as ds
from dynamic_spec import Settings
from acmpc_oracle import fma32

T = np.float32
NAN, INF = float("nan"), float("inf")
EINVAL, ESTATE = -1, -5
NO_TERMS = ((0.0, 0.0), None, 0.0, None)
NO_OBJECTIVE = (0.0, None)

# max |J32 - J64| and |V32 - V64| over the mirror set below, as measured; four times each is allowed
MIRROR_MEASURED = dict(J=1.434e-4, V=3.078e-6)
MIRROR_FACTOR = 4.0
WEIGHT, MARGIN = 40.0, 1.0


def _bits(a):
    return np.asarray(a, dtype=T).view(np.uint32)


def _vehicle():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams.reference().coefficients()


def _problem(H=13, N=512, seed=7, track="monza", **kind):
    dp = ds.make_dynamic_problem(orc, track, H, N, seed, **kind)
    coef = orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(T)
    return dp, coef


def _args(dp, coef, U=None, w_bound=None):
    kw = dp["kw"]
    return (dp["x0"], coef, dp["U"] if U is None else U, _vehicle(), kw["step_cost"], kw["r_term"], kw["final_cost"], kw["u_min"],
            kw["u_max"], kw["w_bound"] if w_bound is None else w_bound, kw["dt"], kw["wheelbase"])


def _settings(clearance=(0.0, 0.0), objective=NO_OBJECTIVE, terms=NO_TERMS):
    return Settings(rate_weight=terms[0], rate_max=terms[1], slip_weight=terms[2], slip_max=terms[3], progress_weight=objective[0],
                    speed_ceiling=objective[1], clearance_weight=clearance[0], clearance_margin=clearance[1])


def _roll(dp, coef, obstacles, clearance=(0.0, 0.0), objective=NO_OBJECTIVE, terms=NO_TERMS, trace=None, **kw):
    states = kw.pop("return_states", False)
    return ds.rollout_dynamic(*_args(dp, coef, **kw), settings=_settings(clearance, objective, terms), obstacles=obstacles,
                              trace=trace, return_states=states)


def _mirror_set():
    """512 candidates at n = 12 with 3 discs: disc 0 stands where the centre plan (candidate 0 in float64) is after step
    6, disc 1 runs beside the start's own velocity 2.5 m to the left, disc 2 comes towards it from 30 m ahead."""
    dp, coef = _problem()
    n = 12
    ref = r64.reference_costs(dp, coef, _vehicle(), U=dp["U"][:1])["states"][0]
    x0 = np.asarray(dp["x0"], dtype=np.float64)
    heading = np.array([np.cos(x0[2]), np.sin(x0[2])])
    left = np.array([-heading[1], heading[0]])
    from acmpc_amd.dynamic_model import predict_obstacles
    start = np.stack([ref[7, :2], x0[:2] + 2.5 * left, x0[:2] + 30.0 * heading])
    velocity = np.stack([np.zeros(2), x0[3] * heading, -0.5 * x0[3] * heading])
    pos = predict_obstacles(start, velocity, n, dp["kw"]["dt"])
    pos[:, 0] = ref[7, :2]
    return dp, coef, (pos.astype(T), np.array([1.5, 1.0, 2.0], dtype=T))


def _mirror_errors():
    from acmpc_amd.dynamic_model import clearance_terms
    dp, coef, (pos, radii) = _mirror_set()
    J32, V32 = _roll(dp, coef, (pos, radii), (WEIGHT, MARGIN), w_bound=0.0)
    ref = r64.reference_costs(dp, coef, _vehicle())
    extra = np.array([clearance_terms(s[1:, :2], pos, radii, WEIGHT, MARGIN) for s in ref["states"]])
    J64, V64 = ref["J"] + extra[:, 0], ref["V"] + extra[:, 1]
    crossed = clearance_terms(ref["states"][0][1:, :2], pos[:, :1], radii[:1])[1]
    return np.abs(J32 - J64), np.abs(V32 - V64), extra, crossed


def test_the_restatement_against_the_float64_mirror():
    dJ, dV, extra, crossed = _mirror_errors()
    print("max |J32 - J64| = %.3e, max |V32 - V64| = %.3e over %d candidates; %d pay clearance, %d penetrate"
          % (dJ.max(), dV.max(), len(dJ), np.count_nonzero(extra[:, 0]), np.count_nonzero(extra[:, 1])))
    assert crossed > 0.0                                        # the centre plan crosses disc 0
    assert np.count_nonzero(extra[:, 1]) > 0 and np.count_nonzero(extra[:, 0]) > 0
    assert dJ.max() <= MIRROR_FACTOR * MIRROR_MEASURED["J"], dJ.max()
    assert dV.max() <= MIRROR_FACTOR * MIRROR_MEASURED["V"], dV.max()


# ---- order and switches ---------------------------------------------------------------------------------------------------------
OBJECTIVE = (3.0, (1.0, 0.3))
TERMS = ((0.3, 0.02), (1.5, None), 40.0, 0.08)


@pytest.mark.parametrize("objective, terms", [(NO_OBJECTIVE, NO_TERMS), (OBJECTIVE, NO_TERMS), (OBJECTIVE, TERMS)])
def test_no_discs_or_discs_that_do_not_exist_are_the_parent_restatement(objective, terms):
    dp, coef = _problem(H=10, N=64, seed=11)
    want = ds.rollout_dynamic(*_args(dp, coef), settings=_settings(objective=objective, terms=terms))
    pos, radii = ds.make_obstacles(dp, 9, 3, 1, nan="all")
    for obstacles in (None, (np.zeros((9, 0, 2), dtype=T), np.zeros(0, dtype=T)), (pos, radii)):
        got = _roll(dp, coef, obstacles, (WEIGHT, MARGIN), objective, terms)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    # +-inf coordinates too: R - inf < 0
    pos[:] = np.inf
    pos[::2] = -np.inf
    got = _roll(dp, coef, (pos, radii), (WEIGHT, MARGIN), objective, terms)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_weight_zero_leaves_E_alone_and_out_of_the_stage_sum():
    dp, coef = _problem(H=10, N=64, seed=12)
    obstacles = ds.make_obstacles(dp, 9, 3, 2)
    off, hard, soft = {}, {}, {}
    plain = _roll(dp, coef, None, trace=off)
    got = _roll(dp, coef, obstacles, (0.0, MARGIN), trace=hard)
    assert not hard["E_added"] and not hard["E"].any()           # E untouched, stage + E not executed
    assert not np.array_equal(_bits(got[1]), _bits(plain[1]))      # ... while the hard part runs
    with_soft = _roll(dp, coef, obstacles, (WEIGHT, MARGIN), trace=soft)
    assert soft["E_added"] and soft["E"].any()
    assert np.array_equal(_bits(with_soft[1]), _bits(got[1]))      # the soft part does not touch V
    assert not np.array_equal(_bits(with_soft[0]), _bits(got[0]))
    # with the rate part on, E is the rate's alone under weight 0
    rate_only, both = {}, {}
    _roll(dp, coef, None, terms=TERMS, trace=rate_only)
    _roll(dp, coef, obstacles, (0.0, MARGIN), terms=TERMS, trace=both)
    assert both["E_added"] and np.array_equal(_bits(both["E"]), _bits(rate_only["E"]))
    # -0.0 and a weight that rounds to 0 as float32 are 0
    for weight in (-0.0, 1e-60):
        assert not ds.constants(None, Settings(clearance_weight=weight, clearance_margin=MARGIN)).soft


def test_a_disc_beyond_its_margin_changes_nothing():
    dp, coef = _problem(H=10, N=64, seed=13)
    want = _roll(dp, coef, None, return_states=True)
    n = 9
    far = np.empty((n, 2, 2), dtype=T)
    far[:, 0] = want[2][:, 1:, :2].max(axis=0) + T(50.0)
    far[:, 1] = want[2][:, 1:, :2].min(axis=0) - T(50.0)
    radii = np.array([3.0, 0.0], dtype=T)
    trace = {}
    got = _roll(dp, coef, (far, radii), (WEIGHT, MARGIN), trace=trace)
    assert trace["E_added"] and not trace["E"].any()             # the soft part ran and added +0
    assert np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(got[0], want[0])                         # stage + 0 is stage


def test_the_order_of_a_steps_additions_to_V():
    """One step where the input box, the corridor, the ceiling and a disc all contribute: V is their squares added in that
    order, each by one fma."""
    dp, coef = _problem(H=3, N=4, seed=14)
    kw = dp["kw"]
    n = 2
    U = np.zeros((1, n, 2), dtype=T)
    U[0, :, 0] = T(kw["u_max"][0]) + T(0.25)                     # outside the box on delta, inside on the pedal
    narrow = coef.copy()
    narrow[:, 7] = T(1e-3)                                         # a corridor the state is outside of
    x0 = np.array(dp["x0"], dtype=T)
    x0[1] += T(0.5)
    dp = dict(dp, x0=x0)
    objective = (0.0, (0.5, 0.0))                                  # a ceiling at half the reference speed
    base = ds.rollout_dynamic(*_args(dp, narrow, U=U[:, :1]), settings=_settings(objective=objective), return_states=True)
    X1 = base[2][0, 1, :2]
    pos = np.full((1, 1, 2), np.nan, dtype=T)
    pos[0, 0] = X1 + T(0.75)
    radii = np.array([2.0], dtype=T)
    got = _roll(dp, narrow, (pos, radii), objective=objective, U=U[:, :1])
    # the step's own pieces, from the restatement without the ceiling and without the disc
    box_corridor = ds.rollout_dynamic(*_args(dp, narrow, U=U[:, :1]))[1]
    assert box_corridor[0] > 0 and base[1][0] > box_corridor[0]    # box + corridor, then the ceiling
    ox, oy = narrow[0, 0], narrow[0, 1]
    Xr, Yr = T(X1[0] - ox), T(X1[1] - oy)
    dx, dy = Xr - T(pos[0, 0, 0] - ox), Yr - T(pos[0, 0, 1] - oy)
    d = np.sqrt(T(fma32(dy, dy, dx * dx)))
    h = np.fmax(radii[0] - d, T(0.0))
    assert h > 0
    assert _bits(got[1])[0] == _bits(fma32(h, h, base[1][0]))


def test_a_disc_exactly_at_the_candidates_position():
    dp, coef = _problem(H=4, N=8, seed=15)
    n = 3
    base = _roll(dp, coef, None, return_states=True)
    R = T(1.25)
    for c in range(3):
        pos = np.full((n, 1, 2), np.nan, dtype=T)
        pos[1, 0] = base[2][c, 2, :2]                              # where candidate c is after step 1
        ox, oy = coef[0, 0], coef[0, 1]
        # (the state is kept relative to the first waypoint: the disc is at the candidate's position when its relative
        # coordinates are the state's, which holds whenever adding the origin back is exact - the path starts at the origin)
        assert T(T(pos[1, 0, 0] - ox) + ox) == pos[1, 0, 0]
        trace = {}
        got = _roll(dp, coef, (pos, np.array([R], dtype=T)), (WEIGHT, 0.0), trace=trace)
        assert _bits(got[1])[c] == _bits(fma32(R, R, base[1][c]))              # d = +0, h = R
        assert _bits(trace["E"])[c] == _bits(fma32((T(0.5) * T(WEIGHT)) * R, R, T(0.0)))


def test_the_generator_bites_without_swamping():
    """make_obstacles' discs are entered by some candidates of every problem, and a single disc not by all of them."""
    for seed, K in ((0, 1), (1, 8), (2, 3)):
        dp, coef = _problem(H=10, N=65, seed=40 + seed)
        plain = _roll(dp, coef, None)
        got = _roll(dp, coef, ds.make_obstacles(dp, 9, K, seed, nan="some"), (WEIGHT, MARGIN))
        changed = _bits(got[1]) != _bits(plain[1])
        assert np.count_nonzero(changed) > 0, (seed, K)
        assert K > 1 or np.count_nonzero(changed) < changed.size, (seed, K)
        assert np.count_nonzero(_bits(got[0]) != _bits(plain[0])) >= np.count_nonzero(changed)


def test_setting_composes_with_the_other_restatements_and_restores_the_module():
    c = fz.case("loaded", "matrix", 0)
    dps = fz.problems(c, orc, limit=16)
    coefs = [orc.coefficients_temporal(d["table"], d["kw"]["margin"]).astype(T) for d in dps]
    want = fz.specification(c, orc, dps, coefs, limit=16, only=[0])[0]
    obstacles = ds.make_obstacles(dps[0], c["H"] - 1, 2, 3)
    got = fz.specification(c, orc, dps, coefs, limit=16, only=[0], obstacles=[obstacles], clearance=(WEIGHT, MARGIN))[0]
    same = fz.specification(c, orc, dps, coefs, limit=16, only=[0], obstacles=None, clearance=(WEIGHT, MARGIN))[0]
    assert np.array_equal(_bits(same[0]), _bits(want[0])) and np.array_equal(_bits(same[1]), _bits(want[1]))
    assert not np.array_equal(_bits(got[0]), _bits(want[0]))
    assert np.array_equal(_bits(got[2]), _bits(want[2]))           # the trajectories do not feel the discs


# ---- the mirror ---------------------------------------------------------------------------------------------------------------
def test_predict_obstacles_against_its_definition():
    from acmpc_amd.dynamic_model import predict_obstacles
    position = np.array([[1.0, 2.0], [-3.0, 0.5]])
    velocity = np.array([[40.0, 0.0], [0.25, -1.0]])
    n, dt = 7, 0.05
    got = predict_obstacles(position, velocity, n, dt)
    assert got.shape == (n, 2, 2) and got.dtype == np.float64
    for i in range(n):
        for k in range(2):
            assert np.array_equal(got[i, k], position[k] + velocity[k] * ((i + 1) * dt))
    one = predict_obstacles([5.0, 6.0], [1.0, 1.0], 3, 0.1)          # a single disc as a flat pair
    assert one.shape == (3, 1, 2) and np.allclose(one[2, 0], [5.3, 6.3])


def test_clearance_terms_against_its_definition():
    from acmpc_amd.dynamic_model import clearance_terms
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
    discs = np.array([[[0.0, 3.0], [NAN, 0.0]], [[1.0, 1.0], [9.0, 9.0]], [[2.0, 0.0], [INF, 0.0]]])
    radii = np.array([2.0, 1.0])
    cost, violation = clearance_terms(xy, discs, radii, weight=4.0, margin=1.5)
    # distances to disc 0: 3, 1, 0 -> depth 0, 1, 2; into the margin 0.5, 2.5, 3.5; disc 1 never exists or is far
    assert violation == pytest.approx(0.0 + 1.0 + 4.0)
    assert cost == pytest.approx(0.5 * 4.0 * (0.25 + 6.25 + 12.25))
    assert clearance_terms(xy, discs, np.zeros(2)) == (0.0, 0.0)


# ---- the handle -----------------------------------------------------------------------------------------------------------------
def _engine(mode=2, P=2, n=5):
    from acmpc_amd import Engine
    dp, _ = _problem(H=n + 1, N=4, seed=21)
    eng = Engine(**dict(dp["kw"], mode=mode, max_problems=P, max_candidates=4, max_steps=n))
    return eng, dp


def _set(eng, pos, radii, P, n, K):
    pos = None if pos is None else np.ascontiguousarray(pos, dtype=T)
    radii = None if radii is None else np.ascontiguousarray(radii, dtype=T)
    return eng._lib.acmpc_set_obstacles(eng._ctx, None if pos is None else pos.ctypes.data,
                                        None if radii is None else radii.ctypes.data, P, n, K)


def _solve_code(eng, dp, P, n):
    """The code the next solve of shape (P, n) ends with on this machine: the shape check comes before any device work."""
    from acmpc_amd import EngineError
    eng.set_paths(np.stack([dp["table"][:, :n]] * P))
    try:
        eng.solve(np.stack([dp["x0"]] * P), np.zeros((P, 4, n, 2), dtype=T))
    except EngineError as e:
        return e.code
    return 0


def test_entry_points_are_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    lib = acmpc_amd.load_library()
    for name in ("acmpc_set_obstacles", "acmpc_set_dynamics_clearance"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert hasattr(acmpc_amd.Engine, "set_obstacles") and hasattr(acmpc_amd.Engine, "set_dynamics_clearance")


def test_refusals_leave_the_handle_as_it_was():
    from acmpc_amd import EngineError
    P, n, K = 2, 5, 3
    eng, dp = _engine(P=P, n=n)
    eng.set_dynamics(_vehicle())
    good = np.zeros((P, n, K, 2), dtype=T)
    radii = np.ones((P, K), dtype=T)
    # nothing set: a solve of any shape passes the obstacles' check (and ends at the missing device, or runs)
    assert _solve_code(eng, dp, 1, 4) != ESTATE
    assert _set(eng, good, radii, P, n, K) == 0
    assert _solve_code(eng, dp, P, n) != ESTATE
    assert _solve_code(eng, dp, P, n - 1) == ESTATE and b"acmpc_set_obstacles" in eng._lib.acmpc_last_error(eng._ctx)
    assert _solve_code(eng, dp, P - 1, n) == ESTATE
    # refused data: the handle keeps the (P, n) it had
    for bad in (-1.0, NAN, INF, -INF):
        r = radii.copy()
        r[0, K - 1] = bad
        assert _set(eng, good[:1, :3], r[:1], 1, 3, K) == EINVAL, bad
        assert b"radius" in eng._lib.acmpc_last_error(eng._ctx)
    assert _set(eng, np.zeros((1, 3, 9, 2), dtype=T), np.ones((1, 9), dtype=T), 1, 3, 9) == EINVAL      # K > 8
    assert _set(eng, good, radii, P, n, -1) == EINVAL
    assert _set(eng, good, radii, P + 1, n, K) == EINVAL and _set(eng, good, radii, 0, n, K) == EINVAL
    assert _set(eng, good, radii, P, n + 1, K) == EINVAL and _set(eng, good, radii, P, 0, K) == EINVAL
    assert _set(eng, good, None, P, n, K) == EINVAL
    with pytest.raises(ValueError):
        eng.set_obstacles(good, radii[:, :2])
    with pytest.raises(EngineError) as e:
        eng.set_obstacles(np.zeros((1, 3, 9, 2), dtype=T), np.ones((1, 9), dtype=T))
    assert e.value.code == EINVAL
    assert _solve_code(eng, dp, P, n) != ESTATE and _solve_code(eng, dp, 1, 3) == ESTATE
    # a radius of 0 and NaN positions are data, not errors; 8 discs are taken
    eng.set_obstacles(np.full((P, n, 8, 2), NAN, dtype=T), np.zeros((P, 8), dtype=T))
    # the Engine's single-problem form, and clearing: NULL, None or K = 0
    eng.set_obstacles(good[0, :, :1], radii[0, :1])
    assert _solve_code(eng, dp, 1, n) != ESTATE and _solve_code(eng, dp, P, n) == ESTATE
    for clear in (lambda: eng.set_obstacles(None), lambda: _set(eng, None, None, 0, 0, 0), lambda: _set(eng, good, radii, P, n, 0),
                  lambda: eng.set_obstacles(np.zeros((P, n, 0, 2), dtype=T), np.zeros((P, 0), dtype=T))):
        eng.set_obstacles(good, radii)
        assert _solve_code(eng, dp, 1, 3) == ESTATE
        assert clear() in (0, None)
        assert _solve_code(eng, dp, 1, 3) != ESTATE
    # the clearance setting: refusals keep the previous one (seen through what the handle still takes), -0.0 is 0
    call = eng._lib.acmpc_set_dynamics_clearance
    assert call(eng._ctx, 40.0, 1.0) == 0
    for weight, margin in ((-1.0, 1.0), (NAN, 1.0), (INF, 1.0), (1e60, 1.0), (1.0, -0.5), (1.0, NAN), (1.0, INF), (1.0, 1e60)):
        assert call(eng._ctx, weight, margin) == EINVAL, (weight, margin)
        with pytest.raises(EngineError):
            eng.set_dynamics_clearance(weight, margin)
    for weight, margin in ((0.0, 0.0), (-0.0, -0.0), (0.0, 2.0), (3.0, 0.0)):
        assert call(eng._ctx, weight, margin) == 0
    # both survive the other setters
    eng.set_obstacles(good, radii)
    eng.set_dynamics_clearance(40.0, 1.0)
    eng.set_dynamics_integration(4, (3.0, 5.0))
    eng.set_dynamics_terms(rate_weight=(0.3, 0.02), slip_max=0.08)
    eng.set_dynamics_objective(2.0, (1.1, 0.0))
    eng.set_dynamics_coupling((0.9, 1.1))
    eng.set_dynamics_load_transfer(0.35)
    eng.set_dynamics(_vehicle())
    assert _solve_code(eng, dp, 1, 3) == ESTATE
    eng.close()
    for mode in (0, 1):
        other, _ = _engine(mode=mode)
        assert _set(other, good, radii, P, n, K) == ESTATE and _set(other, None, None, 0, 0, 0) == ESTATE
        assert other._lib.acmpc_set_dynamics_clearance(other._ctx, 1.0, 1.0) == ESTATE
        with pytest.raises(EngineError) as e:
            other.set_dynamics_clearance(1.0, 1.0)
        assert e.value.code == ESTATE
        other.close()
    lib = eng._lib
    assert lib.acmpc_set_obstacles(None, None, None, 0, 0, 0) == EINVAL and lib.acmpc_set_dynamics_clearance(None, 0.0, 0.0) == EINVAL


def test_solver_takes_the_keys_and_the_argument_without_device_work():
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    solver = DynamicSamplingSolver(dict(horizon=10, n_candidates=8, clearance_cost=40.0, clearance_margin=1.0, progress_cost=3.0))
    solver.close()
    import inspect
    assert "obstacles" in inspect.signature(DynamicSamplingSolver.solve).parameters


@pytest.mark.parametrize("bad", [dict(clearance_cost=-1.0), dict(clearance_cost=NAN), dict(clearance_margin=INF),
                                 dict(clearance_margin=-0.5), dict(clearance_cost=1e60)])
def test_solver_config_is_checked_before_any_handle_exists(bad, monkeypatch):
    from acmpc_amd import _capi
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver

    def no_engine(*args, **kwargs):
        raise AssertionError("a handle was created for a config that must be refused")

    monkeypatch.setattr(_capi, "Engine", no_engine)
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(horizon=20, n_candidates=64, **bad))


if __name__ == "__main__":
    dJ, dV, extra, crossed = _mirror_errors()
    print("max |J32 - J64| = %.6e  max |V32 - V64| = %.6e  (J up to %.3e, V up to %.3e)" % (dJ.max(), dV.max(), 0, 0))
