"""Mode D's rate and slip terms on the CPU ("Rate and slip terms"): the float32 restatement
(tests/dynamic_spec.py) with the terms off against its default, against its own formulas typed out for three steps,
against the float64 mirror (acmpc_amd.dynamic_model.stage_terms), the feasible sets of both under limits the inputs keep
clear of, and the refusals of the C ABI, the Engine and the solver's config (host-side: no device work).

`python tests/test_dynamic_terms.py` prints the measured maxima the mirror's tolerance comes from."""
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
import dynamic_spec as ds  # noqa: E402
from dynamic_spec import Settings  # noqa: E402
from acmpc_oracle import fma32  # noqa: E402

T = np.float32
EINVAL, ESTATE = -1, -5
INF = float("inf")
BLEND = (3.0, 5.0)
OFF = dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=None)
BOTH = dict(rate_weight=(0.3, 0.02), rate_max=(1.5, 6.0), slip_weight=40.0, slip_max=0.08)

# The float32 restatement against the float64 mirror: |a32 - a64| / max(|a64|, 1) of E and of the added violation, over the
# candidates feasible without the terms on both sides.  Measured maxima (NumPy 1.26, x86-64; this file's __main__):
#   the three cases that start at their path's speed or at 12 m/s     E 5.6e-7     added violation 5.9e-7
#   the start at 5 m/s (monza, 19 steps, a previous control set)      E 5.004e-4   added violation 3.406e-4
# At 5 m/s the single Euler step is unstable ("Sub-steps and the low-speed blend"): the two ROLLOUTS
# part in the last places of vy and r, b = (r lr - vy) / vx with them, and the rate part - controls alone - stays at 1e-7.
# The bar is 4 x the largest, the margin test_dynamic_cost_float64.py keeps over its own measurement: 2.0e-3, which is
# ABOVE that file's 1.5e-4 because of that one case (DESIGN.md section 6 says so).
MIRROR_MEASURED = 5.004e-4
MIRROR_RTOL = 4 * MIRROR_MEASURED
MIRROR_TERMS = dict(rate_weight=(0.3, 0.02), rate_max=(1.0, 5.0), slip_weight=40.0, slip_max=0.02)
MIRROR_CASES = [("monza", 20, 128, 0, None, None), ("monza", 20, 128, 1, 5.0, (0.05, -0.2)),
                ("silverstone", 50, 64, 2, None, (-0.1, 0.4)), ("monza", 8, 128, 3, 12.0, None)]


def _params():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams


def _bits(a):
    return np.asarray(a, dtype=T).view(np.uint32)


def _problem(track, H, N, seed, vx0=None):
    dp = ds.make_dynamic_problem(orc, track, H, N, seed, vx0=vx0)
    coef = orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(T)
    return dp, coef, _params().reference().coefficients()


def test_entry_points_are_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    lib = acmpc_amd.load_library()
    for name in ("acmpc_set_dynamics_terms", "acmpc_set_previous_control"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert hasattr(acmpc_amd.Engine, "set_dynamics_terms") and hasattr(acmpc_amd.Engine, "set_previous_control")


# ---- the terms off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track,H,N,seed,vx0,window", [("monza", 20, 33, 0, None, None), ("monza", 50, 17, 1, 0.0, (2, 5)),
                                                       ("monza", 8, 9, 2, 4.0, None)])
def test_terms_off_is_dynamic_spec_bit_for_bit(track, H, N, seed, vx0, window):
    """Costs, V and states, alone and with the integration block entered inside the terms' block; a previous control is not
    read while the rate part is off."""
    dp, coef, vehicle = _problem(track, H, N, seed, vx0)
    dp["U"][1, 0, 0] = np.nan
    dp["U"][4, H // 2, 1] = np.inf
    want = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True)
    want_fine = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True, settings=Settings(4, BLEND))
    for u_prev in (None, (np.nan, 0.5)):
        got = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True, settings=Settings(**OFF), u_prev=u_prev)
        got_fine = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, return_states=True, settings=Settings(4, BLEND, **OFF),
                                 u_prev=u_prev)
        for a, b in zip(want + want_fine, got + got_fine):
            assert np.array_equal(_bits(a), _bits(b))
    # and with the terms on it is another result, under both integration settings (the restatement is not a pass-through)
    on = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, settings=Settings(**BOTH))
    assert not np.array_equal(_bits(want[0]), _bits(on[0]))
    on_fine = ds.spec_costs(orc, dp, coef, vehicle, nn_window=window, settings=Settings(4, BLEND, **BOTH))
    assert not np.array_equal(_bits(want_fine[0]), _bits(on_fine[0]))
    assert not np.array_equal(_bits(on[0]), _bits(on_fine[0]))


def test_which_parts_are_on():
    c = ds.constants(None, Settings(), 0.05)
    assert not c.rate and not c.slip
    assert c.inv_dt == T(20.0) and ds.constants(None, Settings(), 0.03).inv_dt == T(1.0 / 0.03)
    for kw, rate, slip in ((dict(rate_weight=(0.0, 1.0)), True, False), (dict(rate_max=(None, 3.0)), True, False),
                           (dict(rate_max=(INF, INF)), False, False), (dict(slip_weight=2.0), False, True),
                           (dict(slip_max=0.1), False, True), (dict(slip_max=INF, rate_weight=(1e-30, 0.0)), True, False)):
        c = ds.constants(None, Settings(**kw), 0.05)
        assert (c.rate, c.slip) == (rate, slip), kw
    c = ds.constants(None, Settings(rate_weight=(0.3, 3.0), rate_max=(1.5, None), slip_weight=0.7, slip_max=0.1), 0.05)
    assert (c.hwd, c.hwp, c.hws) == (T(0.5) * T(0.3), T(1.5), T(0.5) * T(0.7))
    assert (c.rd_max, c.rp_max, c.b_max) == (T(1.5), T(INF), T(0.1))


def test_constant_controls_from_their_own_previous_control_cost_nothing():
    """Identity: every candidate a constant control, u_prev equal to it (one problem per candidate) or absent, the slip part
    off, any rate weights and limits: every increment is +0, E == +0, and the costs are the parent's bits."""
    dp, coef, vehicle = _problem("monza", 20, 6, 7)
    n = dp["U"].shape[1]
    levels = np.array([[0.0, 0.0], [0.05, 0.3], [-0.2, -1.0], [0.3, 1.0], [-0.013, 0.7], [0.11, -0.4]], dtype=T)
    dp["U"] = np.ascontiguousarray(np.broadcast_to(levels[:, None, :], (6, n, 2)))
    want = ds.spec_costs(orc, dp, coef, vehicle, return_states=True)
    terms = dict(rate_weight=(7.0, 0.3), rate_max=(0.01, 0.02), slip_weight=0.0, slip_max=None)
    settings, trace = Settings(**terms), {}
    got = ds.spec_costs(orc, dp, coef, vehicle, return_states=True, settings=settings, trace=trace)   # no previous control: step 0's own
    assert np.array_equal(_bits(trace["E"]), _bits(np.zeros(6)))
    for a, b in zip(want, got):
        assert np.array_equal(_bits(a), _bits(b))
    for c in range(6):
        got = ds.spec_costs(orc, dp, coef, vehicle, U=dp["U"][c:c + 1], return_states=True, settings=settings, u_prev=levels[c],
                            trace=trace)
        assert np.array_equal(_bits(trace["E"]), _bits(np.zeros(1)))
        for a, b in zip(want, got):
            assert np.array_equal(_bits(a[c:c + 1]), _bits(b))
    # and a previous control that is NOT theirs costs something
    V = ds.spec_costs(orc, dp, coef, vehicle, settings=settings, u_prev=(0.05, 0.3))[1]
    assert V[1] == want[1][1] and np.all(np.delete(V, 1) > np.delete(want[1], 1))


def test_three_steps_typed_out():
    """n = 3, one candidate inside the box and the corridor: E and V against the formulas, every operation a float32 one."""
    dp, coef, vehicle = _problem("monza", 4, 1, 11, vx0=14.0)
    dp["x0"][4:] = (-1.2, 0.1)              # a start that slides: vy, r
    U = np.array([[[0.02, 0.3], [-0.05, 0.25], [-0.04, -0.6]]], dtype=T)
    u_prev = np.array([0.06, 0.1], dtype=T)
    rate_weight, rate_max, slip_weight, slip_max = (0.3, 0.02), (1.0, 8.0), 40.0, 0.03
    base_cost, base_V = ds.spec_costs(orc, dp, coef, vehicle, U=U)
    assert base_V[0] == 0.0
    trace = {}
    cost, V = ds.spec_costs(orc, dp, coef, vehicle, U=U, u_prev=u_prev, trace=trace, settings=Settings(rate_weight=rate_weight,
                            rate_max=rate_max, slip_weight=slip_weight, slip_max=slip_max))
    plain = ds.constants(vehicle, Settings(), dp["kw"]["dt"])
    k = plain.k
    inv_dt = T(1.0 / dp["kw"]["dt"])
    hwd, hwp, hws = T(0.5) * T(0.3), T(0.5) * T(0.02), T(0.5) * T(40.0)
    E, W = T(0.0), T(0.0)
    st = tuple(np.array([v], dtype=T) for v in (0.0, 0.0, dp["x0"][2], dp["x0"][3], dp["x0"][4], dp["x0"][5]))
    pd, pp = u_prev
    hinges = []
    for i in range(3):
        d, p = U[0, i]
        st = ds.dynamic_step(st, U[:, i, 0], U[:, i, 1], plain)
        rd = T(T(d - pd) * inv_dt)
        rp = T(T(p - pp) * inv_dt)
        b = T(T(T(st[5][0] * k["lr"]) - st[4][0]) / T(st[3][0] + T(1.0e-3)))
        E = fma32(T(hwd * rd), rd, E)
        E = fma32(T(hwp * rp), rp, E)
        E = fma32(T(hws * b), b, E)
        for a, limit in ((rd, T(1.0)), (rp, T(8.0)), (b, T(0.03))):
            h = max(T(abs(a) - limit), T(0.0))
            hinges.append(float(h))
            W = fma32(h, h, W)
        pd, pp = d, p
    assert np.array_equal(_bits(trace["E"]), _bits([E]))
    assert np.array_equal(_bits(V), _bits([W]))
    # each kind of hinge is exercised: steering above 1 rad/s at step 1 only, the pedal above 8 /s at step 2 only, the slip
    assert [h > 0 for h in hinges[0::3]] == [False, True, False]
    assert [h > 0 for h in hinges[1::3]] == [False, False, True]
    assert hinges[2] > 0
    assert cost[0] > base_cost[0] and np.isfinite(cost[0])


# ---- the float64 mirror -----------------------------------------------------------------------------------------------------
def _mirror_sides(case, terms):
    """Per candidate feasible without the terms on both sides: (E32, E64, added V32, added V64)."""
    from acmpc_amd.dynamic_model import stage_terms
    track, H, N, seed, vx0, u_prev = case
    dp, coef, vehicle = _problem(track, H, N, seed, vx0)
    assert dp["x0"][3] >= 5.0
    p = _params().reference()
    dt = dp["kw"]["dt"]
    base32 = ds.spec_costs(orc, dp, coef, vehicle)[1]
    base64 = r64.reference_costs(dp, coef, vehicle)["V"]
    keep = np.flatnonzero((base32 == 0) & (base64 == 0))
    trace = {}
    V32 = ds.spec_costs(orc, dp, coef, vehicle, settings=Settings(**terms), u_prev=u_prev, trace=trace)[1]
    rows = []
    for c in keep:
        U = dp["U"][c].astype(np.float64)
        states = p.rollout(dp["x0"].astype(np.float64), U, dt)
        E64, V64 = stage_terms(states, U, dt, None if u_prev is None else np.asarray(u_prev, dtype=T), p, **terms)
        rows.append((float(trace["E"][c]), E64, float(V32[c]), V64))
    return np.array(rows)


def _deviation(rows):
    e = np.abs(rows[:, 0] - rows[:, 1]) / np.maximum(np.abs(rows[:, 1]), 1.0)
    v = np.abs(rows[:, 2] - rows[:, 3]) / np.maximum(np.abs(rows[:, 3]), 1.0)
    return float(e.max()), float(v.max())


@pytest.mark.parametrize("case", MIRROR_CASES, ids=lambda c: "%s-H%d-seed%d" % (c[0], c[1], c[3]))
def test_float32_terms_track_the_float64_mirror(case):
    rows = _mirror_sides(case, MIRROR_TERMS)
    assert len(rows) >= 32                                        # (most candidates are feasible without the terms)
    assert np.count_nonzero(rows[:, 3] > 0) >= 8 and rows[:, 1].min() > 0   # (and the limits bite on some of them)
    e, v = _deviation(rows)
    print("%s: E %.3g, added violation %.3g over %d candidates" % (case, e, v, len(rows)))
    assert e <= MIRROR_RTOL and v <= MIRROR_RTOL


# ---- the feasible set under limits ----------------------------------------------------------------------------------------------
LIMITS = dict(rate_weight=(0.0, 0.0), rate_max=(0.5, 4.0), slip_weight=0.0, slip_max=0.08)


def _clear_controls(rng, N, n, dt):
    """Candidates whose every increment is at most half the rate limit or at least twice it: small random steps, and in
    every other candidate one or two jumps; amplitudes that stay inside the input box."""
    U = np.zeros((N, n, 2))
    for c in range(N):
        for q, limit in enumerate(LIMITS["rate_max"]):
            small = rng.uniform(-0.45, 0.45, n) * limit * dt
            small -= small.mean()                       # (no drift towards the box)
            small = np.clip(small, -0.49 * limit * dt, 0.49 * limit * dt)
            inc = small.copy()
            if c % 2 == 1:
                at = rng.choice(np.arange(1, n), size=min(2, n - 1), replace=False)
                jump = rng.uniform(2.1, 2.6) * limit * dt
                inc[at[0]] = jump
                if len(at) > 1:
                    inc[at[1]] = -jump
            U[c, :, q] = np.cumsum(inc) - inc[0]
    return U.astype(T)


@pytest.mark.parametrize("vy0,r0,n", [(0.0, 0.0, 12), (-5.0, 0.0, 2), (4.5, -0.3, 2), (-0.15, 0.02, 5)])
def test_feasible_sets_are_equal_under_limits_the_inputs_keep_clear_of(vy0, r0, n):
    from acmpc_amd.dynamic_model import stage_terms
    N = 64
    dp, coef, vehicle = _problem("monza", n + 1, N, 30 + n, vx0=14.0)
    dp["x0"][4:] = (vy0, r0)
    dt = dp["kw"]["dt"]
    U = _clear_controls(np.random.default_rng(900 + n), N, n, dt)
    u_prev = U[0, 0].copy()                      # candidate c starts at U[c, 0] = 0 too: step 0's increment is 0
    p = _params().reference()
    base32 = ds.spec_costs(orc, dp, coef, vehicle, U=U)[1]
    base64 = r64.reference_costs(dp, coef, vehicle, U=U)["V"]
    assert np.all(base32 == 0) and np.all(base64 == 0)            # nothing but the terms decides feasibility here
    V32 = ds.spec_costs(orc, dp, coef, vehicle, U=U, settings=Settings(**LIMITS), u_prev=u_prev)[1]
    feasible64 = np.empty(N, dtype=bool)
    for c in range(N):
        U64 = U[c].astype(np.float64)
        states = p.rollout(dp["x0"].astype(np.float64), U64, dt)
        # the float64 side alone satisfies the construction: every rate and every |b| clear of its limit by a factor 2
        rates = np.abs(np.diff(np.concatenate([u_prev[None].astype(np.float64), U64]), axis=0)) / dt
        b = np.abs((states[1:, 5] * p.lr - states[1:, 4]) / (states[1:, 3] + 1e-3))
        for values, limit in ((rates[:, 0], 0.5), (rates[:, 1], 4.0), (b, 0.08)):
            assert np.all((values <= 0.5 * limit) | (values >= 2.0 * limit)), (c, values, limit)
        feasible64[c] = stage_terms(states, U64, dt, u_prev, p, **LIMITS)[1] == 0.0
    assert np.array_equal(V32 == 0, feasible64)
    expect_any = abs(vy0) < 1.0                  # a sliding start is over the slip limit whatever the controls
    assert feasible64[0::2].all() == expect_any and not feasible64[1::2].any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _engine(**extra):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    kw = dict(dp["kw"])
    kw.update(extra)
    return Engine(**kw), dp


def _call(eng, rate_weight, rate_max, slip_weight, slip_max):
    w, m = np.array(rate_weight, dtype=np.float64), np.array(rate_max, dtype=np.float64)
    return eng._lib.acmpc_set_dynamics_terms(eng._ctx, w.ctypes.data, m.ctypes.data, float(slip_weight), float(slip_max))


def test_set_dynamics_terms_refusals():
    """Each bad argument gives ACMPC_EINVAL and leaves the setting as it was: the solve that follows (refused for its P,
    before any device work) reports through the same handle, and the Engine's own check agrees with the ABI's."""
    from acmpc_amd import EngineError
    eng, dp = _engine()
    good = ((0.3, 0.02), (1.5, INF), 40.0, 0.08)
    assert _call(eng, *good) == 0
    nan = float("nan")
    bad = [((-1.0, 0.0), (1.0, 1.0), 0.0, 1.0), ((0.0, nan), (1.0, 1.0), 0.0, 1.0), ((INF, 0.0), (1.0, 1.0), 0.0, 1.0),
           ((0.0, 1e39), (1.0, 1.0), 0.0, 1.0), ((0.0, 0.0), (0.0, 1.0), 0.0, 1.0), ((0.0, 0.0), (1.0, -2.0), 0.0, 1.0),
           ((0.0, 0.0), (nan, 1.0), 0.0, 1.0), ((0.0, 0.0), (1.0, 1.0), -0.5, 1.0), ((0.0, 0.0), (1.0, 1.0), nan, 1.0),
           ((0.0, 0.0), (1.0, 1.0), 0.0, 0.0), ((0.0, 0.0), (1.0, 1.0), 0.0, nan), ((0.0, 0.0), (1.0, 1.0), 0.0, -INF),
           ((0.0, 0.0), (1.0, 1e-50), 0.0, 1.0)]
    for args in bad:
        assert _call(eng, *args) == EINVAL, args
        assert b"rate and slip terms" in eng._lib.acmpc_last_error(eng._ctx)
        with pytest.raises(ValueError):
            eng.set_dynamics_terms(*args)
    assert eng._lib.acmpc_set_dynamics_terms(eng._ctx, None, None, 0.0, 1.0) == EINVAL
    for args in (((0.0, 0.0), (INF, INF), 0.0, INF), ((-0.0, 0.0), (1e-30, 5.0), -0.0, 3.0), good):
        assert _call(eng, *args) == 0, args
    eng.set_dynamics_terms()
    eng.set_dynamics_terms((1.0, 0.0), (None, 2.0), 0.5, None)
    eng.set_dynamics_terms(rate_max=None, slip_max=0.1)
    for wrong in (dict(rate_weight=(1.0,)), dict(rate_weight=1.0), dict(rate_max=(1.0, 2.0, 3.0)), dict(slip_weight="x")):
        with pytest.raises(ValueError):
            eng.set_dynamics_terms(**wrong)
    # the setting does not depend on a vehicle or on the integration setting: taken before, between and after them
    vehicle = _params().reference()
    eng.set_dynamics(vehicle)
    eng.set_dynamics_terms(**BOTH)
    eng.set_dynamics_ensemble([vehicle, vehicle.with_grip(0.6)])
    eng.set_dynamics_integration(4, BLEND)
    eng.set_dynamics_terms()
    eng.close()
    for mode in (0, 1):
        other, _ = _engine(mode=mode)
        with pytest.raises(EngineError) as e:
            other.set_dynamics_terms(**BOTH)
        assert e.value.code == EINVAL
        with pytest.raises(EngineError) as e:
            other.set_previous_control([0.0, 0.0])
        assert e.value.code == EINVAL
        other.close()


def test_previous_control_refusals_and_the_mismatch_of_P():
    from acmpc_amd import EngineError, _capi
    eng, dp = _engine(max_problems=3)
    eng.set_dynamics(_params().reference())
    eng.set_paths(dp["table"])                                    # P = 1
    lib, ctx = eng._lib, eng._ctx
    two = np.zeros((2, 2), dtype=T)
    assert lib.acmpc_set_previous_control(ctx, two.ctypes.data, 0) == EINVAL
    assert lib.acmpc_set_previous_control(ctx, two.ctypes.data, 4) == EINVAL      # beyond max_problems
    with pytest.raises(ValueError):
        eng.set_previous_control(np.zeros((2, 3)))
    n = dp["U"].shape[1]
    x0, U = dp["x0"][None], dp["U"][None]
    costs = np.empty((1, 8), dtype=T)
    best = np.empty(1, dtype=np.int32)

    def solve():
        return lib.acmpc_solve(ctx, _capi._f32(x0), _capi._f32(U), 1, 8, n, 0, _capi._f32(costs),
                               best.ctypes.data_as(_capi._I32P), None)

    eng.set_previous_control(two)                                 # stored P = 2, the tables' P = 1
    assert solve() == ESTATE and b"acmpc_set_previous_control" in lib.acmpc_last_error(ctx)
    with pytest.raises(EngineError) as e:
        eng.optimize(x0, np.zeros((1, n, 2), dtype=T), None, 8, 1, (0.05, 0.3))
    assert e.value.code == ESTATE
    # cleared, or replaced by one of the right P, the same call gets past the check (and then finds no device here, or runs)
    eng.set_previous_control(None)
    assert solve() != ESTATE
    eng.set_previous_control(two[:1])
    assert solve() != ESTATE
    eng.close()


@pytest.mark.parametrize("bad", [dict(rate_cost=(-1.0, 0.0)), dict(rate_cost=(0.0, float("nan"))), dict(rate_cost=1.0),
                                 dict(rate_limit=(0.0, 1.0)), dict(rate_limit=(1.0, float("nan"))), dict(rate_limit=(1.0,)),
                                 dict(slip_cost=-2.0), dict(slip_cost=float("inf")), dict(slip_limit=0.0),
                                 dict(slip_limit=-0.1), dict(slip_limit=float("nan"))])
def test_solver_config_is_checked_before_any_handle_exists(bad, monkeypatch):
    from acmpc_amd import _capi
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver

    def no_engine(*args, **kwargs):
        raise AssertionError("a handle was created for a config that must be refused")

    monkeypatch.setattr(_capi, "Engine", no_engine)
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(horizon=20, n_candidates=64, **bad))


def test_mirror_counts_what_the_formulas_say():
    from acmpc_amd.dynamic_model import stage_terms
    p = _params().reference()
    U = np.array([[0.0, 0.0], [0.05, 0.0], [0.05, -0.5]])
    states = np.zeros((4, 6))
    states[:, 3] = 10.0 - 1e-3
    states[2, 4] = -1.0                                            # b = 0.1 at step 1
    E, V = stage_terms(states, U, 0.05, (0.0, 0.25), p, rate_weight=(2.0, 4.0), rate_max=(0.5, None), slip_weight=8.0,
                       slip_max=0.04)
    assert E == pytest.approx(0.5 * (2.0 * 1.0 ** 2 + 4.0 * (5.0 ** 2 + 10.0 ** 2) + 8.0 * 0.1 ** 2))
    assert V == pytest.approx((1.0 - 0.5) ** 2 + (0.1 - 0.04) ** 2)
    assert stage_terms(states, U, 0.05, None, p, rate_weight=(2.0, 4.0))[0] == pytest.approx(0.5 * (2.0 + 4.0 * 100.0))


if __name__ == "__main__":
    worst = [0.0, 0.0]
    for case in MIRROR_CASES:
        e, v = _deviation(_mirror_sides(case, MIRROR_TERMS))
        print("%-50s E %.3e   added violation %.3e" % (case, e, v))
        worst = [max(worst[0], e), max(worst[1], v)]
    print("maxima: E %.3e, added violation %.3e -> bar 4 x %.3e" % (worst[0], worst[1], max(worst)))
