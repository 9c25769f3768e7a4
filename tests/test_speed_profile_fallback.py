"""Every problem the two sweeps of the exact speed profile hand back (csrc/acmpc_admm.h: exact_profile -> solve), on the
host: what the sweeps leave behind when they reject, and what the splitting says about the problem afterwards.

A problem is handed back for one of these reasons:
  a rate bound of the wrong sign (a_min > 0, a_max < 0) - still a QP with an optimum: the splitting must SOLVE it;
  an empty box (some ceiling below v_min: a row with l > u) - no optimum: the splitting must never say "solved";
  a non-finite ceiling, a spacing that is not positive and finite - not a problem at all: never "solved" either.
The sizes are the ones at which the code changes its form: 64 / 65 (an element per lane against the workspace scan on the
device), 128 / 129 (cyclic reduction against the sequential sweeps), 1000 (the lap profile's path), and the smallest.
No GPU work; tests/test_gpu_tick_fallback.py runs the same problems through the tick."""
import numpy as np
import pytest

import acmpc_oracle as orc

SIZES = (2, 3, 49, 64, 65, 99, 128, 129, 1000)
A_MIN, A_MAX, V_MIN = -1.3, 1.0, 8.0
CAP = 4000                      # the controller's iteration cap (and the C API's default)
SENTINEL = -12345.678


def feasible_problem(n):
    """A wavy ceiling strictly inside (v_min, 30], end velocity 14, uneven spacing: feasible (every ceiling is above v_min and
    a_min <= 0 <= a_max), with rate rows active."""
    rng = np.random.default_rng(n)
    v_hi = np.clip(20 + 8 * np.sin(np.arange(n) / 7.0) + rng.normal(0, 1.5, n), 9.0, 30.0)
    v_hi[-1] = 14.0
    return dict(v_hi=v_hi, ds=rng.uniform(2.0, 3.5, n), a_min=A_MIN, a_max=A_MAX, v_min=V_MIN)


def _with(problem, **changes):
    out = dict(problem)
    for key, (index, value) in changes.items():
        if index is None:
            out[key] = value
        else:
            out[key] = problem[key].copy()
            out[key][index] = value
    return out


def rejected_problem(reason, n):
    """(the rejected problem, its feasible neighbour).  Ceilings change at the last index (the end velocity) or at n // 2,
    spacings at row (n - 1) // 2 - the only row of n = 2."""
    base = feasible_problem(n)
    row = (n - 1) // 2
    if reason == "a_min>0":
        return _with(base, a_min=(None, 0.02)), base
    if reason == "a_max<0":
        return _with(base, a_max=(None, -0.05)), base
    if reason.startswith("end-"):
        return _with(base, v_hi=(-1, V_MIN - float(reason[4:]))), base
    if reason == "all-below":        # the localised solver with v_max < v_min: a constant ceiling
        return _with(base, v_hi=(slice(None), V_MIN - 0.5)), _with(base, v_hi=(slice(None), 28.0))
    if reason.startswith("ceiling-"):
        return _with(base, v_hi=(n // 2, dict(nan=np.nan, inf=np.inf)[reason[8:]])), base
    value = {"ds-zero": 0.0, "ds-negative": -2.5, "ds-nan": np.nan, "ds-inf": np.inf}[reason]
    return _with(base, ds=(row, value)), base


SIGN = ("a_min>0", "a_max<0")
EMPTY_BOX = ("end-1e-5", "end-0.5", "end-6", "all-below")
NOT_A_PROBLEM = ("ceiling-nan", "ceiling-inf", "ds-zero", "ds-negative", "ds-nan", "ds-inf")
REASONS = SIGN + EMPTY_BOX + NOT_A_PROBLEM


def args_of(p):
    return p["v_hi"], p["ds"], p["a_min"], p["a_max"], p["v_min"]


def warm_starts(neighbour):
    """None (cold), the neighbour's exact profile (y = 0), the neighbour's splitting iterate (y != 0)."""
    from acmpc_amd import _capi
    swept = _capi.speed_profile_exact(*args_of(neighbour))
    assert swept is not None and not swept[1].any()
    x, y, status, _ = _capi.speed_profile_qp(*args_of(neighbour))
    assert status == "solved" and y.any()
    return {"cold": None, "exact": swept, "iterate": (x, y)}


def sign_problem(which, n=49):
    """The two sign-rejected problems with an optimum: a straight at constant spacing, ceiling 30, end velocity 14."""
    v_hi = np.full(n, 30.0)
    v_hi[-1] = 14.0
    p = dict(v_hi=v_hi, ds=np.full(n, 2.45), a_min=A_MIN, a_max=A_MAX, v_min=V_MIN)
    return _with(p, a_max=(None, -0.05)) if which == "a_max<0" else _with(p, a_min=(None, 0.02)), p


def dense_rows(p):
    """A, l, u of the QP as the reference assembles them (speed_profile.py:45-51)."""
    n = p["v_hi"].shape[0]
    gain = 1.0 / (2.0 * p["ds"][:n - 1])
    A = np.zeros((2 * n - 1, n))
    rows = np.arange(n - 1)
    A[rows, rows], A[rows, rows + 1] = -gain, gain
    A[n - 1 + np.arange(n), np.arange(n)] = 1.0
    lower = np.concatenate([np.full(n - 1, p["a_min"]), np.full(n, p["v_min"])])
    upper = np.concatenate([np.full(n - 1, p["a_max"]), p["v_hi"]])
    return A, lower, upper


# ---- 1. the contract of the sweeps ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("reason", REASONS)
def test_rejecting_sweeps_leave_the_iterate_untouched(reason, n):
    """acmpc_speed_profile_exact returns 1 and writes nothing: v and y are the caller's warm iterate, which the splitting
    that runs next must start from.  (Before this was fixed, v came back as the swept profile on every infeasible, non-finite
    and bad-spacing problem - only the two sign returns left it alone.)  The oracle's restatement rejects the same inputs
    and accepts the feasible neighbour of each."""
    from acmpc_amd import _capi
    problem, neighbour = rejected_problem(reason, n)
    v_hi = np.ascontiguousarray(problem["v_hi"])
    ds = np.ascontiguousarray(problem["ds"])
    v, y = np.full(n, SENTINEL), np.full(2 * n - 1, SENTINEL)
    rc = _capi.load_library().acmpc_speed_profile_exact(v_hi.ctypes.data, ds.ctypes.data, n, problem["a_min"], problem["a_max"],
                                                        problem["v_min"], v.ctypes.data, y.ctypes.data)
    assert rc == 1
    assert (v == SENTINEL).all(), "v written at %s" % np.flatnonzero(v != SENTINEL)[:5]
    assert (y == SENTINEL).all()
    assert orc.speed_profile_exact(*args_of(problem)) is None
    want = orc.speed_profile_exact(*args_of(neighbour))
    got = _capi.speed_profile_exact(*args_of(neighbour))
    assert want is not None and got is not None
    np.testing.assert_array_equal(got[0], want)


def test_accepting_sweeps_write_every_entry():
    """(the other half of the contract: on success nothing of the caller's buffers is left)"""
    from acmpc_amd import _capi
    for n in SIZES:
        p = feasible_problem(n)
        v, y = np.full(n, SENTINEL), np.full(2 * n - 1, SENTINEL)
        v_hi, ds = np.ascontiguousarray(p["v_hi"]), np.ascontiguousarray(p["ds"])
        rc = _capi.load_library().acmpc_speed_profile_exact(v_hi.ctypes.data, ds.ctypes.data, n, p["a_min"], p["a_max"], p["v_min"],
                                                            v.ctypes.data, y.ctypes.data)
        assert rc == 0 and (v != SENTINEL).all() and not y.any()


# ---- 2. an empty box is never "solved" --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("reason", EMPTY_BOX)
def test_an_empty_box_is_never_solved(reason, n):
    """Some ceiling below v_min: the box row has l > u and the QP no feasible point - by 1e-5 (below every tolerance of the
    solver), 0.5 and 6 m/s at the end velocity, and everywhere.  The splitting runs to its cap whatever the cap, the
    stride of its stopping test and its start.  (Before the fix, at the cap of 4000 every one of these stopped "solved"
    after 60 - 180 iterations, except n = 64 by 6 m/s; e.g. n = 49 by 6 m/s: 150 iterations, v[-1] = 2.003.)"""
    from acmpc_amd import _capi
    problem, neighbour = rejected_problem(reason, n)
    for name, warm in warm_starts(neighbour).items():
        for cap in (CAP, 60):
            for check_every in (1, 10):
                _, _, status, iters = _capi.speed_profile_qp(*args_of(problem), max_iter=cap, check_every=check_every, warm=warm)
                assert status != "solved", (name, cap, check_every, iters)
                assert iters == cap, (name, cap, check_every)


@pytest.mark.parametrize("n", SIZES)
def test_an_equality_row_is_not_an_empty_box(n):
    """The ceiling EQUAL to v_min (l == u: the row OSQP gives the thousandfold step size) has exactly one feasible value and
    is solved - at the end velocity and at an interior point.  The iterate x sits within the stopping test's own tolerance of
    that value: |x - z| <= eps_abs + eps_rel max(|Ax|, |z|) with z = v_min on that row.  At the controller's 1e-3 that bound is
    3e-2 (measured over these sizes: 7e-11 to 1e-5); the 1e-9 this test holds follows from it at eps = 1e-11 (3.1e-10 with
    |x| <= 30; measured <= 8e-14)."""
    from acmpc_amd import _capi
    base = feasible_problem(n)
    for index in (n - 1, n // 2):
        problem = _with(base, v_hi=(index, V_MIN))
        assert _capi.speed_profile_exact(*args_of(problem)) is not None
        for check_every in (1, 10):
            x, _, status, iters = _capi.speed_profile_qp(*args_of(problem), check_every=check_every)
            assert status == "solved" and 0 < iters < CAP
            assert abs(x[index] - V_MIN) <= 1e-3 + 1e-3 * max(np.abs(x).max(), problem["v_hi"].max())
        x, _, status, iters = _capi.speed_profile_qp(*args_of(problem), max_iter=400000, eps_abs=1e-11, eps_rel=1e-11)
        assert status == "solved" and 0 < iters < 400000
        print("n %d index %d: x - v_min = %.3e after %d iterations" % (n, index, x[index] - V_MIN, iters))
        assert abs(x[index] - V_MIN) <= 1e-9


# ---- 3. what is not a problem at all ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("reason", NOT_A_PROBLEM)
def test_a_non_finite_ceiling_or_a_bad_spacing_is_never_solved(reason, n):
    """Never "solved", and the same verdict and count from every start.  (A zero or NaN spacing and a non-finite ceiling put
    NaN into the iterate, which no comparison accepts; a NEGATIVE spacing flips its rate row and an INFINITE one cuts the chain
    - QPs of their own, which the splitting used to solve: 30 - 80 iterations cold, 10 - 80 warm.)"""
    from acmpc_amd import _capi
    problem, neighbour = rejected_problem(reason, n)
    for cap in (CAP, 60):
        seen = set()
        for name, warm in warm_starts(neighbour).items():
            _, _, status, iters = _capi.speed_profile_qp(*args_of(problem), max_iter=cap, warm=warm)
            assert status != "solved", (name, cap, iters)
            seen.add((status, iters))
        assert seen == {("maximum iterations reached", cap)}


# ---- 4. a rate bound of the wrong sign: a QP like any other ---------------------------------------------------------------
@pytest.mark.parametrize("which", SIGN)
def test_sign_rejected_problems_are_solved(which):
    """n = 49, spacing 2.45, ceiling 30, end velocity 14.  a_max = -0.05 (the car must lose 0.245 m/s per waypoint) and
    a_min = +0.02 (must gain 0.098) are feasible QPs the sweeps do not take; warm from the exact profile of the same ceiling
    at a_max = 1.0 the splitting stops "solved" after 1710 and 3450 iterations, and its iterate meets every row of A, l, u to
    its own stopping tolerance eps_abs + eps_rel max|Ax|."""
    from acmpc_amd import _capi
    problem, neighbour = sign_problem(which)
    assert _capi.speed_profile_exact(*args_of(problem)) is None
    warm = _capi.speed_profile_exact(*args_of(neighbour))
    x, y, status, iters = _capi.speed_profile_qp(*args_of(problem), warm=warm)
    print("%s: %s after %d iterations" % (which, status, iters))
    assert status == "solved" and 0 < iters < CAP
    A, lower, upper = dense_rows(problem)
    Ax = A @ x
    tolerance = 1e-3 + 1e-3 * np.abs(Ax).max()
    print("row excess %.3e of %.3e" % (max((lower - Ax).max(), (Ax - upper).max()), tolerance))
    assert (Ax >= lower - tolerance).all() and (Ax <= upper + tolerance).all()


@pytest.mark.parametrize("which", SIGN)
def test_sign_rejected_problems_against_the_dense_restatement(which):
    """Both problems at 1e-10 (cap 400 000, as test_speed_profile_exact.py does for the golden problems): the native
    tridiagonal splitting against the oracle's dense restatement of OSQP, atol 2e-6 (that file's bound; measured here:
    1.6e-10 for a_min = +0.02 and 9.4e-10 for a_max = -0.05, after 21 000 - 22 000 iterations on either side).  The restatement
    runs with the paper's step-size update, as the native solver always does: with a fixed step size it has not reached
    1e-10 on either problem after 400 000 iterations (0.6 m/s off)."""
    from acmpc_amd import _capi
    problem, _ = sign_problem(which)
    x, _, status, iters = _capi.speed_profile_qp(*args_of(problem), max_iter=400000, eps_abs=1e-10, eps_rel=1e-10)
    assert status == "solved", iters
    A, lower, upper = dense_rows(problem)
    n = x.shape[0]
    ref = orc.osqp_restated(np.ones(n), -problem["v_hi"], A, lower, upper, max_iter=400000, eps_abs=1e-10, eps_rel=1e-10,
                            check_every=10, adaptive_rho=True)
    print("native %d iterations; restated %s after %d; gap %.3e" % (iters, ref.info.status, ref.info.iter, np.abs(x - ref.x).max()))
    assert ref.info.status == "solved"
    np.testing.assert_allclose(x, ref.x, rtol=0, atol=2e-6)
    Ax = A @ x
    assert (Ax >= lower - 1e-8).all() and (Ax <= upper + 1e-8).all()


# ---- 5. the host solver object ----------------------------------------------------------------------------------------------
def _straight_path(n=49, spacing=2.45):
    from acmpc_amd import _capi
    from acmpc_amd.reference_path import ReferencePath
    y = spacing * np.arange(n + 1)
    return ReferencePath.from_table(_capi.waypoint_table(np.stack([np.zeros(n + 1), y, np.full(n + 1, 8.0)], axis=1)))


@pytest.mark.parametrize("change,solved", [(dict(v_min=20.0), False), (dict(a_max=-0.05), True)])
def test_the_solver_object_keeps_its_iterate_over_an_unsolved_call(change, solved):
    """feasible, rejected, feasible on one `SpeedProfileSolver` ("exact").  An unsolved call (the end velocity 14 under
    v_min 20) leaves `_warm` what it was; a solved fallback (a_max < 0) makes it that call's (x, y)."""
    from acmpc_amd.speed_profile import SpeedProfileSolver
    cons = dict(a_min=A_MIN, a_max=A_MAX, v_min=V_MIN, v_max=28.0, ay_max=4.0, ki_min=1e-3, end_velocity=14.0)
    solver = SpeedProfileSolver({"control_horizon": 49, "max_iterations": CAP, "constraints": cons})
    path = _straight_path()
    first = solver.solve(path, cons["end_velocity"])
    assert first.info.status == "solved" and first.info.iter == 0
    kept = tuple(a.copy() for a in solver._warm)
    np.testing.assert_array_equal(kept[0], first.x)
    original = dict(cons)
    cons.update(change)                                        # the live dict, as the control process rewrites it
    second = solver.solve(path, cons["end_velocity"])
    if solved:
        assert second.info.status == "solved" and second.info.iter > 0
        np.testing.assert_array_equal(solver._warm[0], second.x)
        np.testing.assert_array_equal(solver._warm[1], second.y)
        assert second.y.any()
    else:
        assert second.info.status != "solved" and second.info.iter == CAP
        np.testing.assert_array_equal(solver._warm[0], kept[0])
        np.testing.assert_array_equal(solver._warm[1], kept[1])
    cons.update(original)
    third = solver.solve(path, cons["end_velocity"])
    assert third.info.status == "solved" and third.info.iter == 0
    np.testing.assert_array_equal(third.x, first.x)
