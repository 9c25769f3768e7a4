"""Mode D's objective on the CPU ("Mode D, progress and ceiling"): the refusals of the C ABI, the Engine
and the solver's config (host side: no device work), the host's progress table against its restatement bit for bit, the
float32 restatement (tests/dynamic_spec.py) with both parts off against the same settings without them and against its
own definition with one part on, the order of negative costs, and the restatement against the float64 mirror
(acmpc_amd.dynamic_model.objective_terms).

`python tests/test_dynamic_objective.py` prints the measured maxima the mirror's bars come from."""
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
import dynamic_reference64 as r64  # noqa: E402
import dynamic_sampled_spec as dss  # noqa: E402
import dynamic_spec as ds  # noqa: E402
from dynamic_spec import Settings  # noqa: E402
import test_dynamic_cost_float64 as c64  # noqa: E402
from acmpc_oracle import fma32  # noqa: E402

T = np.float32
EINVAL, ESTATE = -1, -5
INF, NAN = float("inf"), float("nan")
BLEND = (3.0, 5.0)
TERMS = dict(rate_weight=(0.3, 0.02), rate_max=(1.5, 6.0), slip_weight=40.0, slip_max=0.08)

# The float32 restatement against the float64 mirror over the cases of tests/test_dynamic_cost_float64.py (each under its
# first vehicle, its first 256 candidates' worth: N = min(N, 256)), progress_weight 2 and the ceiling (1.02, 0.2).  Measured maxima (NumPy 1.26, x86-64; this file's __main__),
# the cases that do not start at a standstill | the three that do - the split test_dynamic_cost_float64.py makes, for its
# reason: from vx near 0 the model amplifies the last place of its inputs and the two ROLLOUTS part:
#   |s32 - s64| over every candidate                                         1.830e-4 m (silverstone yaw n 128) | 6.779e-3 m
#   |c32 - c64| / max(|c64|, 1) over the candidates feasible on both sides   1.266e-4 (monza far n 49)          | 4.853e-4
# The bars are 4 x the measured, the margin the grip tests keep.  The candidates whose float64 vx - cap comes within the
# |s32 - s64| bar of 0 at some step may be feasible on one side only; MIRROR_EXCEPTED is their measured share.
MIRROR_OBJECTIVE = dict(progress_weight=2.0, speed_ceiling=(1.02, 0.2))
MIRROR_S = (1.830e-4, 6.779e-3)
MIRROR_REL = (1.266e-4, 4.853e-4)
MIRROR_EXCEPTED_CAP = 0.02


def _params():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams


def _bits(a):
    return np.asarray(a, dtype=T).view(np.uint32)


def _problem(track, H, N, seed, vx0=None):
    dp = ds.make_dynamic_problem(orc, track, H, N, seed, vx0=vx0)
    coef = orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(T)
    return dp, coef, _params().reference().coefficients()


def _engine(**extra):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    kw = dict(dp["kw"])
    kw.update(extra)
    return Engine(**kw), dp


def _call(eng, weight, ceiling):
    c = None if ceiling is None else np.array(ceiling, dtype=np.float64)
    return eng._lib.acmpc_set_dynamics_objective(eng._ctx, float(weight), None if c is None else c.ctypes.data)


def test_entry_points_are_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    lib = acmpc_amd.load_library()
    for name in ("acmpc_set_dynamics_objective", "acmpc_get_progress_table"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert hasattr(acmpc_amd.Engine, "set_dynamics_objective") and hasattr(acmpc_amd.Engine, "progress_table")


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_set_dynamics_objective_refusals():
    """Each bad argument gives ACMPC_EINVAL, another mode ACMPC_ESTATE; NULL is no ceiling; the Engine's own check agrees
    with the ABI's; and the call is taken before, between and after the other settings of the handle."""
    from acmpc_amd import EngineError
    eng, dp = _engine()
    assert _call(eng, 2.0, (1.1, 0.5)) == 0
    bad = [(-1.0, None), (NAN, None), (INF, None), (1e39, None), (-1e-30, (1.0, 0.0)), (0.0, (-0.5, 0.0)), (0.0, (NAN, 0.0)),
           (0.0, (INF, 0.0)), (1.0, (1.0, NAN)), (1.0, (1.0, INF)), (1.0, (1.0, -INF)), (1.0, (1e39, 0.0)), (1.0, (1.0, -1e39))]
    for weight, ceiling in bad:
        assert _call(eng, weight, ceiling) == EINVAL, (weight, ceiling)
        assert b"progress_weight" in eng._lib.acmpc_last_error(eng._ctx) or b"ceiling" in eng._lib.acmpc_last_error(eng._ctx)
        with pytest.raises(ValueError):
            eng.set_dynamics_objective(weight, ceiling)
    for weight, ceiling in ((0.0, None), (-0.0, None), (0.0, (0.0, 0.0)), (3.0, None), (1e-30, (1.0, -5.0)), (0.0, (-0.0, 0.0))):
        assert _call(eng, weight, ceiling) == 0, (weight, ceiling)
    eng.set_dynamics_objective()
    eng.set_dynamics_objective(1.5, 1.1)                  # a scalar: the scale, offset 0
    eng.set_dynamics_objective(speed_ceiling=(1.1, -0.5))
    for wrong in (dict(progress_weight="x"), dict(speed_ceiling=(1.0,)), dict(speed_ceiling=(1.0, 2.0, 3.0)),
                  dict(speed_ceiling="fast")):
        with pytest.raises(ValueError):
            eng.set_dynamics_objective(**wrong)
    vehicle = _params().reference()
    eng.set_dynamics_objective(2.0, (1.1, 0.0))
    eng.set_dynamics(vehicle)
    eng.set_dynamics_ensemble([vehicle, vehicle.with_grip(0.6)])
    eng.set_dynamics_integration(4, BLEND)
    eng.set_dynamics_terms(**TERMS)
    eng.set_dynamics_objective()
    eng.close()
    for mode in (0, 1):
        other, odp = _engine(mode=mode)
        with pytest.raises(EngineError) as e:
            other.set_dynamics_objective(1.0)
        assert e.value.code == ESTATE
        other.set_paths(odp["table"])
        with pytest.raises(EngineError) as e:
            other.progress_table(0)
        assert e.value.code == ESTATE
        other.close()


@pytest.mark.parametrize("bad", [dict(progress_cost=-1.0), dict(progress_cost=NAN), dict(progress_cost="fast"),
                                 dict(speed_ceiling=-1.0), dict(speed_ceiling=(1.0, INF)), dict(speed_ceiling=(1.0, 2.0, 3.0)),
                                 dict(speed_ceiling=INF), dict(progress_cost=1.0, speed_ceiling="x")])
def test_solver_config_is_checked_before_any_handle_exists(bad, monkeypatch):
    from acmpc_amd import _capi
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver

    def no_engine(*args, **kwargs):
        raise AssertionError("a handle was created for a config that must be refused")

    monkeypatch.setattr(_capi, "Engine", no_engine)
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(horizon=20, n_candidates=64, **bad))


# ---- the progress table ----------------------------------------------------------------------------------------------------
def _line_table(n, heading, spacing=2.0, origin=(100.0, -40.0)):
    m = np.arange(n, dtype=np.float64)
    return np.stack([origin[0] + spacing * m * np.cos(heading), origin[1] + spacing * m * np.sin(heading),
                     np.full(n, heading), np.zeros(n), np.full(n, spacing), np.full(n, 8.0), np.full(n, 10.0)])


def test_progress_table_is_the_restatement_bit_for_bit():
    from acmpc_amd import EngineError
    eng, dp = _engine(max_steps=512, max_problems=2)
    try:
        with pytest.raises(EngineError) as e:
            eng.progress_table(0)                          # no paths yet
        assert e.value.code == ESTATE
        # a monza window, through set_paths and through set_coefficients of the same rows
        eng.set_paths(dp["table"])
        coef = eng.coefficients(0)
        q = eng.progress_table(0)
        assert np.array_equal(_bits(q), _bits(ds.progress_table(coef)))
        assert q[0] == 0.0 and np.all(np.isfinite(q))
        eng.set_paths(_line_table(19, 0.3))                # (other rows in between: q follows the rows)
        assert not np.array_equal(_bits(eng.progress_table(0)), _bits(q))
        eng.set_coefficients(coef[None])
        assert np.array_equal(_bits(eng.progress_table(0)), _bits(q))
        # two problems: each its own rows
        other = ds.make_dynamic_problem(orc, "silverstone", 20, 8, 3)["table"]
        eng.set_paths(np.stack([dp["table"], other]))
        for p in range(2):
            assert np.array_equal(_bits(eng.progress_table(p)), _bits(ds.progress_table(eng.coefficients(p))))
        assert not np.array_equal(_bits(eng.progress_table(0)), _bits(eng.progress_table(1)))
        with pytest.raises(EngineError):
            eng.progress_table(2)
        # a straight line: the arc length of waypoint m IS its along-track distance from the first - q_m == 0 within one
        # rounding of the float32 positions (spacing 2 m from (100, -40): half an ulp of 2^10 at most, times sqrt 2)
        for heading in (0.0, 0.3, -2.0):
            eng.set_paths(_line_table(300, heading))
            q = eng.progress_table(0)
            assert np.array_equal(_bits(q), _bits(ds.progress_table(eng.coefficients(0))))
            assert np.abs(q).max() <= 2.0 ** -13 * 1.5, (heading, np.abs(q).max())
        # a repeated waypoint: dx = dy = 0 adds nothing
        table = _line_table(12, 0.7)
        table[:2, 5] = table[:2, 4]
        coef = orc.coefficients_temporal(table, 0.0).astype(T)
        assert np.array_equal(_bits(coef[5, :4]), _bits(coef[4, :4]))
        eng.set_coefficients(coef[None])
        q = eng.progress_table(0)
        assert np.array_equal(_bits(q), _bits(ds.progress_table(coef))) and q[5] == q[4]
        # the smallest and the largest horizon of a handle: n = 2 (acmpc_set_paths refuses n = 1, where the restatement's
        # table is the single 0) and n = 512
        assert np.array_equal(_bits(ds.progress_table(coef[:1])), _bits(np.zeros(1)))
        with pytest.raises(EngineError):
            eng.set_paths(_line_table(1, 0.0))
        eng.set_paths(dp["table"][:, :2])
        assert np.array_equal(_bits(eng.progress_table(0)), _bits(ds.progress_table(eng.coefficients(0))))
        big = ds.make_dynamic_problem(orc, "monza", 513, 4, 1)["table"][:, :512]
        eng.set_paths(big)
        q = eng.progress_table(0)
        assert q.shape == (512,) and np.array_equal(_bits(q), _bits(ds.progress_table(eng.coefficients(0))))
    finally:
        eng.close()


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track,H,N,seed,vx0,window", [("monza", 20, 33, 0, None, None), ("monza", 50, 17, 1, 0.0, (2, 5)),
                                                       ("monza", 8, 9, 2, 4.0, None)])
def test_both_parts_off_is_the_parent_restatement_bit_for_bit(track, H, N, seed, vx0, window):
    """Costs, V and states: against dynamic_spec alone, through the terms' block, and through the terms' and the
    integration's blocks."""
    dp, coef, vehicle = _problem(track, H, N, seed, vx0)
    dp["U"][1, 0, 0] = np.nan
    dp["U"][4, H // 2, 1] = np.inf
    u_prev = (0.02, 0.1)
    want = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True)
    want_terms = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True, settings=Settings(**TERMS),
                               u_prev=u_prev)
    want_fine = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True, settings=Settings(4, BLEND, **TERMS),
                              u_prev=u_prev)
    for off in (dict(), dict(progress_weight=0.0, speed_ceiling=None), dict(progress_weight=-0.0)):
        got = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True, settings=Settings(**off))
        got_terms = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True, settings=Settings(**TERMS, **off),
                                  u_prev=u_prev)
        got_fine = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True,
                                 settings=Settings(4, BLEND, **TERMS, **off), u_prev=u_prev)
        for a, b in zip(want + want_terms + want_fine, got + got_terms + got_fine):
            assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("inner", ["plain", "terms", "terms+fine"])
def test_progress_alone_is_one_fma_on_the_cost(inner):
    """J_new == fma(nwp, s, J_old) per candidate - with w_bound = 0, so that J is what the rollout returns - and V is
    untouched; s is the along-track arc length at the last state, typed out here from the rows."""
    dp, coef, vehicle = _problem("monza", 20, 40, 5)
    dp["kw"] = dict(dp["kw"], w_bound=0.0)
    dp["U"][3, 2, 0] = np.nan
    weight = 1.75

    base = dict(plain=Settings(), terms=Settings(**TERMS))["terms" if inner != "plain" else "plain"]
    if inner == "terms+fine":
        base = base.replace(substeps=3, low_speed_blend=BLEND)
    u_prev = None if inner == "plain" else (0.01, 0.2)

    def run(settings, trace=None):
        return ds.spec_costs(orc, dp, coef, vehicle, nn_window=(2, 5), return_states=True, settings=settings, u_prev=u_prev,
                             trace=trace)

    J_old, V_old, X_old = run(base)
    trace = {}
    J_new, V_new, X_new = run(base.replace(progress_weight=weight), trace)
    s, j = trace["s"], trace["j"][:, -1]
    assert np.array_equal(_bits(V_old), _bits(V_new)) and np.array_equal(_bits(X_old), _bits(X_new))
    with np.errstate(all="ignore"):
        assert np.array_equal(_bits(J_new), _bits(fma32(-T(weight), s, J_old)))
    # s from the rows: positions relative to the first waypoint, q of the host's definition
    q = ds.progress_table(coef)
    X, Y = X_old[:, -1, 0] - coef[0, 0], X_old[:, -1, 1] - coef[0, 1]
    with np.errstate(all="ignore"):
        want = fma32(coef[j, 3], Y, fma32(coef[j, 2], X, q[j]))
    assert np.array_equal(_bits(s), _bits(want))
    ok = np.isfinite(s)
    assert ok.sum() == len(s) - 1 and np.all(s[ok] > 5.0)      # 19 steps at monza's speed: tens of metres made good
    assert np.isnan(J_new[3])


def test_ceiling_alone_changes_exactly_the_candidates_over_it():
    dp, coef, vehicle = _problem("monza", 20, 64, 6)
    old = ds.spec_costs(orc, dp, coef, vehicle, nn_window=(2, 5), return_states=True)
    ceiling = (1.0, 0.1)
    trace = {}
    new = ds.spec_costs(orc, dp, coef, vehicle, nn_window=(2, 5), return_states=True, settings=Settings(speed_ceiling=ceiling),
                        trace=trace)
    over = trace["over"]
    broke = (over > 0).any(axis=1)
    assert 4 < broke.sum() < len(broke) - 4                     # (the inputs have both kinds)
    changed = _bits(old[0]) != _bits(new[0])
    assert np.array_equal(changed, broke)
    assert np.array_equal(_bits(old[1]) != _bits(new[1]), broke) and np.all(new[1][broke] > old[1][broke])
    assert np.array_equal(_bits(old[2]), _bits(new[2]))
    # a NaN v_ref is no ceiling: h = max(NaN, 0) = 0
    blind = coef.copy()
    blind[:, 6] = np.nan
    nov = ds.spec_costs(orc, dp, blind, vehicle, nn_window=(2, 5), settings=Settings(speed_ceiling=ceiling))
    assert np.array_equal(_bits(nov[1]), _bits(ds.spec_costs(orc, dp, blind, vehicle, nn_window=(2, 5))[1]))
    # a scale of 0 with offset 0 is a ceiling of 0 m/s: every moving candidate is over it
    assert np.all(ds.spec_costs(orc, dp, coef, vehicle, nn_window=(2, 5), settings=Settings(speed_ceiling=0.0))[1] > 0)


def test_negative_costs_are_ordered_as_floats():
    """A progress weight large enough that EVERY cost is negative: pick_best and the keys pick the most negative, ties to
    the lower index; -inf and NaN rank last; -0 sorts below +0 in the keys only."""
    from acmpc_amd import _capi
    dp, coef, vehicle = _problem("monza", 20, 48, 8)
    dp["kw"] = dict(dp["kw"], w_bound=10.0)      # (a violation of the planted candidates does not outweigh the reward)
    dp["U"][7] = dp["U"][2]                      # a tie: candidates 2 and 7 are the same controls
    cost, V = ds.spec_costs(orc, dp, coef, vehicle, nn_window=(2, 5), settings=Settings(progress_weight=5000.0))
    assert np.all(cost < 0) and np.all(np.isfinite(cost)) and cost[2] == cost[7]
    best = orc.pick_best(cost)[0]
    assert best == int(np.argmin(cost)) and cost[best] == cost.min()
    keys = [_capi.pack_key(float(c), i) for i, c in enumerate(cost)]
    assert keys == [dss.pack_key(c, i) for i, c in enumerate(cost)]
    assert int(np.argmin(keys)) == best and _capi.key_index(min(keys)) == best
    assert sorted(range(len(cost)), key=lambda i: keys[i]) == sorted(range(len(cost)), key=lambda i: (cost[i], i))
    assert _capi.key_cost(min(keys)) == float(cost[best])
    # the tie goes to the lower index, whichever of the two is best overall
    forced = cost.copy()
    forced[[2, 7]] = cost.min() * T(2.0)
    assert orc.pick_best(forced)[0] == 2
    assert _capi.key_index(min(_capi.pack_key(float(c), i + 1000) for i, c in enumerate(forced))) == 1002
    # non-finite costs rank last, -inf included; a large index does not leak into the cost word
    for worst in (-INF, INF, NAN):
        assert _capi.pack_key(worst, 0) > max(keys)
        assert _capi.pack_key(worst, 0) == dss.pack_key(T(worst), 0)
        mixed = cost.copy()
        mixed[best] = worst
        assert orc.pick_best(mixed)[0] == int(np.argmin(np.where(np.arange(len(cost)) == best, INF, cost)))
    assert _capi.pack_key(-1.0, 0xfffffffe) < _capi.pack_key(-0.5, 0) < _capi.pack_key(-0.0, 5) < _capi.pack_key(0.0, 0)


# ---- the float64 mirror ----------------------------------------------------------------------------------------------------
def _mirror_case(case):
    """One case of test_dynamic_cost_float64.CASES under its first vehicle: the restatement's (cost, V, s, over) and the
    float64 side's (cost, V, s, the smallest |vx - cap| of each candidate, ceiling-feasible), the mirror applied to the
    float64 reference's states."""
    from acmpc_amd.dynamic_model import objective_terms
    track, kind, n, N, window, grips, _, _ = case
    N = min(N, 256)
    dp = ds.make_dynamic_problem(orc, track, n + 1, N, n, **c64.KINDS[kind])
    kw = dp["kw"]
    coef = orc.coefficients_temporal(dp["table"], kw["margin"])
    vehicle = c64._vehicle(grips[0])
    trace = {}
    c32, V32 = ds.spec_costs(orc, dp, coef.astype(T), vehicle, nn_window=window, settings=Settings(**MIRROR_OBJECTIVE), trace=trace)
    s32, over32 = trace["s"], trace["over"]
    ref = r64.reference_costs(dp, coef, vehicle, nn_window=window)
    table = dp["table"][:, :n]
    scale, offset = MIRROR_OBJECTIVE["speed_ceiling"]
    s64, extra = np.empty(N), np.empty(N)
    for c in range(N):
        s64[c], extra[c] = objective_terms(ref["states"][c], dp["U"][c], table, nn_window=window, **MIRROR_OBJECTIVE)
    over64 = ref["states"][:, 1:, 3] - (scale * table[6][ref["j"]] + offset)
    assert np.allclose(extra, np.sum(np.maximum(over64, 0.0) ** 2, axis=1), rtol=1e-9, atol=1e-12)   # (the mirror's own j agrees)
    V64 = ref["V"] + extra
    c64_ = ref["J"] - MIRROR_OBJECTIVE["progress_weight"] * s64 + float(kw["w_bound"]) * V64
    return dict(c32=c32.astype(np.float64), V32=V32, s32=s32.astype(np.float64), ok32=~(over32 > 0).any(axis=1),
                c64=c64_, V64=V64, s64=s64, ok64=~(over64 > 0).any(axis=1), near=np.abs(over64).min(axis=1))


def _mirror_figures(m):
    both = (m["V32"] == 0) & (m["V64"] == 0)
    rel = np.abs(m["c32"] - m["c64"]) / np.maximum(np.abs(m["c64"]), 1.0)
    return dict(s=float(np.abs(m["s32"] - m["s64"]).max()), rel=float(rel[both].max()) if both.any() else 0.0,
                feasible=int(both.sum()), differ=int(np.count_nonzero(m["ok32"] != m["ok64"])))


@pytest.mark.parametrize("case", c64.CASES, ids=c64._label)
def test_the_restatement_against_the_float64_mirror(case):
    standstill = int(case[1] == "standstill")
    m = _mirror_case(case)
    f = _mirror_figures(m)
    print("%s: |s32 - s64| %.3e m, rel cost %.3e over %d, feasibility differs at %d" % (c64._label(case), f["s"], f["rel"],
                                                                                       f["feasible"], f["differ"]))
    bar_s, bar_rel = 4 * MIRROR_S[standstill], 4 * MIRROR_REL[standstill]
    assert f["s"] <= bar_s
    assert f["rel"] <= bar_rel
    # the same candidates stay under the ceiling, those within the bar of it on the float64 side apart - and the inputs
    # keep those to 2 % of the candidates
    excepted = m["near"] <= bar_s
    assert np.count_nonzero(excepted) <= MIRROR_EXCEPTED_CAP * len(excepted), np.count_nonzero(excepted)
    assert np.array_equal(m["ok32"][~excepted], m["ok64"][~excepted])
    if case[2] > 2 and not standstill:   # (both kinds of candidate, but from a standstill and over two steps)
        assert 0 < np.count_nonzero(m["ok64"]) < len(excepted)


def test_mirror_counts_what_the_formulas_say():
    from acmpc_amd.dynamic_model import objective_terms
    table = _line_table(10, 0.0, spacing=2.0, origin=(0.0, 0.0))
    table[6] = np.linspace(10.0, 19.0, 10)
    states = np.zeros((4, 6))
    states[:, 0] = [0.0, 1.9, 4.2, 7.1]          # nearest waypoints of the three steps: 1, 2, 4
    states[:, 1] = [0.0, 0.5, -0.5, 0.3]
    states[:, 3] = [10.0, 12.0, 11.0, 16.0]
    U = np.zeros((3, 2))
    s, V = objective_terms(states, U, table, 3.0, (1.0, 0.5))
    assert s == pytest.approx(7.1) and V == pytest.approx((12.0 - 11.5) ** 2 + (16.0 - 14.5) ** 2)
    assert objective_terms(states, U, table) == (pytest.approx(7.1), 0.0)
    assert objective_terms(states, U, table, 0.0, 0.5)[1] == pytest.approx((12 - 5.5) ** 2 + (11 - 6) ** 2 + (16 - 7) ** 2)
    # a window that cannot reach the nearest waypoint: (0, 1) from 0 gets to waypoint 1, 2, 3
    s, V = objective_terms(states, U, table, 0.0, (1.0, 0.5), nn_window=(0, 1))
    assert s == pytest.approx(7.1) and V == pytest.approx(0.5 ** 2 + (16.0 - 13.5) ** 2)
    # past the last waypoint s keeps growing linearly
    states[-1, 0] = 30.0
    assert objective_terms(states, U, table)[0] == pytest.approx(30.0)


if __name__ == "__main__":
    worst = dict(s=[0.0, 0.0], rel=[0.0, 0.0], share=[0.0, 0.0])
    for case in c64.CASES:
        m = _mirror_case(case)
        f = _mirror_figures(m)
        k = int(case[1] == "standstill")
        share = float(np.mean(m["near"] <= 4 * MIRROR_S[k]))
        for key, value in (("s", f["s"]), ("rel", f["rel"]), ("share", share)):
            worst[key][k] = max(worst[key][k], value)
        print("%-52s feasible on both %4d  |s32 - s64| %.3e m  rel %.3e  under the ceiling %4d / %4d, differ %d, excepted %.4f"
              % (c64._label(case), f["feasible"], f["s"], f["rel"], np.count_nonzero(m["ok64"]), len(m["ok64"]), f["differ"], share))
    print("maxima (others | standstill): |s32 - s64| %.3e | %.3e m   rel %.3e | %.3e   excepted share %.4f | %.4f"
          % (*worst["s"], *worst["rel"], *worst["share"]))
