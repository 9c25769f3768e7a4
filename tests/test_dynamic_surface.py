"""Mode D's surface table (acmpc_set_surface), CPU only: the float32 restatement with a table (tests/dynamic_surface_spec.py)
against dynamic_spec without one and against itself (the two properties the GPU tests rest on), the handle's refusals and
persistence without a device, dynamic_model.surface_table, the float64 mirror (dynamic_model.trace(..., surface=)) against the
restatement, and one physics statement re-derived from the mirror: full braking into a patch of half the grip.

`python tests/test_dynamic_surface.py` prints the measured figures the mirror's bound and DESIGN.md's numbers come from."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "ac-mpc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acmpc_oracle as orc  # noqa: E402
import dynamic_spec as ds  # noqa: E402
import dynamic_surface_spec as dss  # noqa: E402
import test_gpu_dynamic_coupling as tgc  # noqa: E402
import test_gpu_dynamic_load_transfer as tgl  # noqa: E402
from dynamic_spec import Settings  # noqa: E402

T = np.float32
NAN, INF = float("nan"), float("inf")
EINVAL, ESTATE = -1, -5
H, N, SEED = 13, 300, 2401
n = H - 1
FEW = 64                      # candidates where a test runs many settings: the forced ones (10 .. 14, 5, 7) are among them
LOAD = tgl.LOAD
AERO = (7.35e-4, 1.1025e-3, 100.0)
DEFAULT, FINE = tgc.DEFAULT, tgc.FINE
OFF, ALL_FOUR = tgc.OFF, tgc.ALL_FOUR
_same_where_finite = tgl._same_where_finite
TIERS = {"none": dict(), "coupled": dict(coupling=(1.0, 1.0)), "loaded-coupled": dict(coupling=(0.9, 1.1), load_transfer=LOAD),
         "all-with-downforce": dict(coupling=(0.9, 1.1), load_transfer=LOAD, downforce=AERO)}

# max |J32 - J64| / max(|J64|, 1) over the candidates feasible on both sides, the float32 restatement against the float64 mirror on
# the dense problem under the three tables of test_the_float64_mirror..., as this file's __main__ measures it (NumPy 1.26, x86-64;
# DESIGN.md section 6); four times that is allowed, as tests/test_dynamic_cost_float64.py allows it
MIRROR_MEASURED = 3.869e-7
MIRROR_RTOL = 4 * MIRROR_MEASURED


def _vehicle():
    from acmpc_amd import DynamicBicycleParams
    return DynamicBicycleParams.reference()


def _dense(vx0=None, seed=SEED, N=N):
    dp = dss.make_dense_problem(orc, H, N, seed, vx0=vx0)
    return dp, orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(T)


def _standard(seed=2400, N=N):
    dp = ds.make_dynamic_problem(orc, "monza", H, N, seed)
    return dp, orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(T)


def _reaches_several_waypoints(dp, coef, **kw):
    """The conditions a test of the table relies on: the nearest index reaches 3, and some step has lanes on different waypoints."""
    trace = {}
    dss.spec_costs(orc, dp, coef, _vehicle().coefficients(), trace=trace, **kw)
    j = trace["j"]
    assert j.max() >= 3, j.max()
    assert any(len(np.unique(j[:, i])) > 1 for i in range(j.shape[1]))
    return j


# ---- 1: no table, dynamic_spec's bits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", list(TIERS))
def test_without_a_table_the_restatement_is_dynamic_spec(tier):
    vehicle = _vehicle().coefficients()
    for name, (dp, coef) in (("standard", _standard(N=FEW)), ("dense", _dense(N=FEW))):
        tgc._force_pedals(dp["U"], n)
        discs = ds.make_obstacles(dp, n, 2, 7)
        u_prev = (0.02, -0.1)
        for integration in (DEFAULT, FINE):
            for setting, prev in ((OFF, None), (ALL_FOUR, u_prev)):
                for obstacles in (None, discs):
                    for window in (None, (2, 5)):
                        s = Settings(*integration, **setting[0], **setting[1], clearance_weight=40.0, clearance_margin=1.0, **TIERS[tier])
                        kw = dict(nn_window=window, settings=s, u_prev=prev, obstacles=obstacles, return_states=True)
                        want, got = {}, {}
                        a = ds.spec_costs(orc, dp, coef, vehicle, trace=want, **kw)
                        b = dss.spec_costs(orc, dp, coef, vehicle, trace=got, **kw)
                        label = (name, tier, integration, prev is not None, obstacles is not None, window)
                        for x, y in zip(a, b):
                            assert np.array_equal(ds.bits(x), ds.bits(y)), label
                        for key in ("states", "terms", "totals", "j", "e_y", "E"):
                            assert np.array_equal(np.asarray(want[key]).view(np.uint32 if want[key].dtype == T else want[key].dtype),
                                                  np.asarray(got[key]).view(np.uint32 if got[key].dtype == T else got[key].dtype)), label


# ---- 2: the two properties ------------------------------------------------------------------------------------------------------
def test_a_table_of_ones_is_the_handle_with_downforce_and_the_plain_handle():
    vehicle = _vehicle().coefficients()
    ones = np.ones((n, 2), dtype=T)
    problems = [_standard(2400, N=FEW), _standard(2401, N=FEW), _dense(N=FEW), _dense(vx0=0.0, N=FEW)]
    for dp, coef in problems:
        tgc._force_pedals(dp["U"], n)     # (the two infeasible candidates among them: a NaN pedal, an inf steering)
    for q, (dp, coef) in enumerate(problems):
        for integration, setting in ((DEFAULT, OFF), (FINE, ALL_FOUR)):
            base = dict(zip(("substeps", "low_speed_blend"), integration), **setting[0], **setting[1])
            for tier, step in TIERS.items():
                s = Settings(**base, **step)
                got = dss.spec_costs(orc, dp, coef, vehicle, settings=s, surface=ones, return_states=True, nn_window=(2, 5))
                # bit for bit: the same handle with the downforce on (k = 0 where it is off) and no table
                aero = ds.spec_costs(orc, dp, coef, vehicle, settings=dss.surface_settings(s), return_states=True, nn_window=(2, 5))
                for x, y in zip(got, aero):
                    assert np.array_equal(ds.bits(x), ds.bits(y)), (q, tier)
                # where finite: the handle as it is
                plain = ds.spec_costs(orc, dp, coef, vehicle, settings=s, return_states=True, nn_window=(2, 5))
                for x, y in zip(got[:2], plain[:2]):
                    _same_where_finite(x, y, (q, tier))
    # a plain handle: every candidate of the standard problems, the two infeasible ones included
    for dp, coef in (_standard(2400), _standard(2401)):
        tgc._force_pedals(dp["U"], n)
        got = dss.spec_costs(orc, dp, coef, vehicle, surface=ones)
        plain = ds.spec_costs(orc, dp, coef, vehicle)
        for x, y in zip(got, plain):
            assert np.array_equal(np.isnan(x), np.isnan(y))
            _same_where_finite(x, y)
        assert np.isnan(plain[0][5]) and not np.isfinite(plain[0][7])


@pytest.mark.parametrize("scales", [(0.5, 0.5), (0.5, 0.25)])
def test_a_uniform_power_of_two_table_is_the_grip_scaled_vehicle(scales):
    v = _vehicle()
    scaled = (v.with_grip(scales[0]) if scales[0] == scales[1] else v.with_axle_grip(*scales)).coefficients()
    table = np.tile(np.asarray(scales, dtype=T), (n, 1))
    for dp, coef in (_dense(N=FEW), _standard(N=FEW)):
        tgc._force_pedals(dp["U"], n)
        for integration in (DEFAULT, FINE):
            for tier, step in TIERS.items():
                s = Settings(*integration, **ALL_FOUR[0], **ALL_FOUR[1], **step)
                got = dss.spec_costs(orc, dp, coef, v.coefficients(), settings=s, surface=table, return_states=True)
                want = ds.spec_costs(orc, dp, coef, scaled, settings=s, return_states=True)
                if tier == "all-with-downforce":
                    for x, y in zip(got, want):
                        assert np.array_equal(ds.bits(x), ds.bits(y)), tier
                else:
                    for x, y in zip(got[:2], want[:2]):
                        _same_where_finite(x, y, tier)


def test_a_random_table_reaches_every_cost_of_the_dense_problem():
    dp, coef = _dense()
    _reaches_several_waypoints(dp, coef)
    vehicle = _vehicle().coefficients()
    plain = ds.spec_costs(orc, dp, coef, vehicle)[0]
    got = dss.spec_costs(orc, dp, coef, vehicle, surface=dss.random_table(n, 1))[0]
    assert np.count_nonzero(ds.bits(got) != ds.bits(plain)) == N
    assert orc.pick_best(got)[0] != orc.pick_best(plain)[0]
    # the scale lags by one control step: a table that differs from 1 only at waypoints no candidate has left by the last
    # step's start changes nothing
    trace = {}
    dss.spec_costs(orc, dp, coef, vehicle, trace=trace)
    late = np.ones((n, 2), dtype=T)
    late[trace["j"][:, : n - 1].max() + 1:] = T(0.5)
    assert np.array_equal(ds.bits(dss.spec_costs(orc, dp, coef, vehicle, surface=late)[0]),
                          ds.bits(dss.spec_costs(orc, dp, coef, vehicle, surface=np.ones((n, 2), dtype=T))[0]))


# ---- 3: the handle, without a device --------------------------------------------------------------------------------------------
def _engine(mode=2, P=2, steps=5):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", steps + 1, 4, 21)
    return Engine(**dict(dp["kw"], mode=mode, max_problems=P, max_candidates=4, max_steps=steps)), dp


def _set(eng, grip, P, steps):
    grip = None if grip is None else np.ascontiguousarray(grip, dtype=T)
    return eng._lib.acmpc_set_surface(eng._ctx, None if grip is None else grip.ctypes.data, P, steps)


def _solve_code(eng, dp, P, steps):
    """The code the next solve of shape (P, steps) ends with on this machine: the shape check comes before any device work."""
    from acmpc_amd import EngineError
    eng.set_paths(np.stack([dp["table"][:, :steps]] * P))
    try:
        eng.solve(np.stack([dp["x0"]] * P), np.zeros((P, 4, steps, 2), dtype=T))
    except EngineError as e:
        return e.code
    return 0


def _trace_code(eng, dp, P, steps):
    from acmpc_amd import EngineError
    eng.set_paths(np.stack([dp["table"][:, :steps]] * P))
    try:
        eng.trace_plans(np.stack([dp["x0"]] * P), np.zeros((P, 1, steps, 2), dtype=T))
    except EngineError as e:
        return e.code
    return 0


def test_the_entry_point_is_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    lib = acmpc_amd.load_library()
    assert "acmpc_set_surface" in _capi.SIGNATURES and hasattr(lib, "acmpc_set_surface")
    assert hasattr(acmpc_amd.Engine, "set_surface")


def test_refusals_leave_the_handle_as_it_was_and_the_table_survives_the_other_setters():
    from acmpc_amd import EngineError
    P, steps = 2, 5
    eng, dp = _engine(P=P, steps=steps)
    eng.set_dynamics(_vehicle())
    good = np.full((P, steps, 2), 0.7, dtype=T)
    # nothing set: a solve of any shape passes the table's check (and ends at the missing device, or runs)
    assert _solve_code(eng, dp, 1, 4) != ESTATE
    assert _set(eng, good, P, steps) == 0
    assert _solve_code(eng, dp, P, steps) != ESTATE
    assert _solve_code(eng, dp, P, steps - 1) == ESTATE and b"acmpc_set_surface" in eng._lib.acmpc_last_error(eng._ctx)
    assert _solve_code(eng, dp, P - 1, steps) == ESTATE
    assert _trace_code(eng, dp, P, steps - 1) == ESTATE and _trace_code(eng, dp, P, steps) != ESTATE
    # refused tables: the handle keeps the (P, n) it had
    for bad in (0.0, -0.5, NAN, INF, -INF):
        g = np.full((1, 3, 2), 0.7, dtype=T)
        g[0, 2, 1] = bad
        assert _set(eng, g, 1, 3) == EINVAL, bad
        assert b"grip scale" in eng._lib.acmpc_last_error(eng._ctx)
    assert _set(eng, good, P + 1, steps) == EINVAL and _set(eng, good, 0, steps) == EINVAL
    assert _set(eng, good, P, steps + 1) == EINVAL and _set(eng, good, P, 0) == EINVAL
    assert _solve_code(eng, dp, P, steps) != ESTATE and _solve_code(eng, dp, 1, 3) == ESTATE
    with pytest.raises(EngineError) as e:
        eng.set_surface(np.zeros((P, steps, 2), dtype=T))
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        eng.set_surface(np.ones((P, steps, 3), dtype=T))
    # the Engine's shorter forms: [n, 2] and [n] are one problem's
    eng.set_surface(good[0])
    assert _solve_code(eng, dp, 1, steps) != ESTATE and _solve_code(eng, dp, P, steps) == ESTATE
    eng.set_surface(np.full(3, 0.5))
    assert _solve_code(eng, dp, 1, 3) != ESTATE and _solve_code(eng, dp, 1, steps) == ESTATE
    # None, or NULL, clears it
    for clear in (lambda: eng.set_surface(None), lambda: _set(eng, None, 0, 0)):
        eng.set_surface(good)
        assert _solve_code(eng, dp, 1, 3) == ESTATE
        assert clear() in (0, None)
        assert _solve_code(eng, dp, 1, 3) != ESTATE
    # it survives the other setters
    eng.set_surface(good)
    eng.set_dynamics_integration(3, (3.0, 5.0))
    eng.set_dynamics_terms((0.3, 0.02), (1.5, 6.0), 40.0, 0.08)
    eng.set_dynamics_objective(3.0, (1.05, 0.0))
    eng.set_dynamics_coupling((0.9, 1.1))
    eng.set_dynamics_load_transfer(0.35)
    eng.set_dynamics_downforce(AERO)
    eng.set_dynamics_downforce(None)
    eng.set_dynamics_clearance(40.0, 1.0)
    eng.set_obstacles(np.zeros((P, steps, 2, 2), dtype=T), np.ones((P, 2), dtype=T))
    eng.set_obstacles(None)
    eng.set_previous_control(np.zeros((P, 2), dtype=T))
    eng.set_previous_control(None)
    eng.set_dynamics_ensemble([_vehicle(), _vehicle().with_grip(0.6)])
    eng.set_dynamics(_vehicle())
    assert _solve_code(eng, dp, 1, 3) == ESTATE and _solve_code(eng, dp, P, steps) != ESTATE
    lib = eng._lib
    eng.close()
    for mode in (0, 1):
        other, _ = _engine(mode=mode)
        assert _set(other, good, P, steps) == ESTATE and _set(other, None, 0, 0) == ESTATE
        with pytest.raises(EngineError) as e:
            other.set_surface(good)
        assert e.value.code == ESTATE
        other.close()
    assert lib.acmpc_set_surface(None, None, 0, 0) == EINVAL


def test_the_solver_takes_the_argument_without_device_work():
    import inspect
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    assert "surface" in inspect.signature(DynamicSamplingSolver.solve).parameters
    assert "surface=" in sys.modules[DynamicSamplingSolver.__module__].__doc__


# ---- 4: surface_table -----------------------------------------------------------------------------------------------------------
def test_surface_table():
    from acmpc_amd.dynamic_model import surface_table
    s = np.arange(10) * 10.0
    plain = surface_table(s, [])
    assert plain.dtype == T and plain.shape == (10, 2) and np.all(plain == 1.0)
    wet = surface_table(s, [(40.0, 70.0, 0.6)])
    assert np.array_equal(wet[:, 0], wet[:, 1])
    assert np.array_equal(wet[:, 0], np.array([1, 1, 1, 1, 0.6, 0.6, 0.6, 0.6, 1, 1], dtype=T))   # both ends inclusive
    # overlaps: the later patch wins where both lie; two scales per patch; a patch outside the path does nothing
    both = surface_table(s, [(40.0, 70.0, 0.6), (60.0, 200.0, 0.9, 0.8), (500.0, 600.0, 0.1), (-50.0, -1.0, 0.1)])
    assert np.array_equal(both[:, 0], np.array([1, 1, 1, 1, 0.6, 0.6, 0.9, 0.9, 0.9, 0.9], dtype=T))
    assert np.array_equal(both[:, 1], np.array([1, 1, 1, 1, 0.6, 0.6, 0.8, 0.8, 0.8, 0.8], dtype=T))
    assert np.array_equal(surface_table(s, [(60.0, 200.0, 0.9, 0.8), (40.0, 70.0, 0.6)])[:, 0],
                          np.array([1, 1, 1, 1, 0.6, 0.6, 0.6, 0.6, 0.9, 0.9], dtype=T))
    for bad in ([(0.0, 1.0)], [(0.0, 1.0, 0.0)], [(0.0, 1.0, 0.5, NAN)], [(0.0, 1.0, -1.0, 1.0)], [(0.0, 1.0, 1.0, 1.0, 1.0)]):
        with pytest.raises(ValueError):
            surface_table(s, bad)


# ---- 5: the float64 mirror ------------------------------------------------------------------------------------------------------
MIRROR_CANDIDATES = 96
MIRROR_SETTINGS = dict(coupling=(1.0, 1.0), load_transfer=LOAD, downforce=AERO)


def _mirror_tables():
    step = np.ones((n, 2), dtype=T)
    step[2:] = T(0.5)
    return {"random": dss.random_table(n, 5), "step to 0.5": step, "uniform 0.5": np.full((n, 2), 0.5, dtype=T)}


def _mirror_cost(dp, U, table):
    """(cost, V) of one plan from dynamic_model.trace in float64: the weighted sums of what its lines saw."""
    from acmpc_amd import dynamic_model as dm
    kw = dp["kw"]
    # (the input box as the handle holds it, float32: a control clipped to it in float32 lies ON the bound, not 1e-8 outside)
    out = dm.trace(_vehicle(), dp["x0"], U, dp["table"], dt=kw["dt"], u_min=np.asarray(kw["u_min"], dtype=T),
                   u_max=np.asarray(kw["u_max"], dtype=T), margin=kw["margin"], wheelbase=kw["wheelbase"], surface=table,
                   **MIRROR_SETTINGS)
    Q, R, QN = (np.asarray(kw[k], dtype=np.float64) for k in ("step_cost", "r_term", "final_cost"))
    tN = n * kw["dt"]
    stage = 0.5 * (Q[0] * np.sum(out["e_y"] ** 2) + Q[1] * np.sum(out["e_psi"] ** 2) + R[0] * np.sum(out["dv"] ** 2)
                   + R[1] * np.sum(out["dk"] ** 2))
    terminal = 0.5 * (QN[0] * out["e_y"][-1] ** 2 + QN[1] * out["e_psi"][-1] ** 2 + QN[2] * tN ** 2)
    V = float(out["V"][-1])
    return stage + terminal + kw["w_bound"] * V, V, out["j"]


def _mirror_figures():
    dp, coef = _dense()
    U = dp["U"][:MIRROR_CANDIDATES]
    figures = {}
    for name, table in _mirror_tables().items():
        trace = {}
        c32, V32 = dss.spec_costs(orc, dp, coef, _vehicle().coefficients(), U=U, settings=Settings(**MIRROR_SETTINGS), surface=table,
                                  trace=trace)
        assert trace["j"].max() >= 3 and any(len(np.unique(trace["j"][:, i])) > 1 for i in range(n))
        c64, V64, j64 = (np.array(a) for a in zip(*[_mirror_cost(dp, u, table) for u in U]))
        both = (V32 == 0) & (V64 == 0)
        rel = np.abs(c32.astype(np.float64) - c64) / np.maximum(np.abs(c64), 1.0)
        figures[name] = dict(same_feasible=bool(np.array_equal(V32 == 0, V64 == 0)), feasible=int(both.sum()),
                             rel=float(rel[both].max()), same_j=float(np.mean(np.stack(j64) == trace["j"])))
    return figures


def test_the_float64_mirror_against_the_restatement():
    for name, f in _mirror_figures().items():
        assert f["same_feasible"] and f["feasible"] > MIRROR_CANDIDATES // 2, (name, f)
        assert f["rel"] <= MIRROR_RTOL, (name, f)


def test_the_mirrors_grip_argument_is_the_grip_scaled_vehicle():
    v = _vehicle()
    state, u = np.array([0.0, 0.0, 0.1, 20.0, 0.3, 0.1]), np.array([0.05, -0.6])
    a = v.predict_next_state(state, u, 0.05, grip=(0.7, 0.6), **MIRROR_SETTINGS)
    b = v.with_axle_grip(0.7, 0.6).predict_next_state(state, u, 0.05, **MIRROR_SETTINGS)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    U = np.tile(u, (5, 1))
    assert np.array_equal(v.rollout(state, U, grip=(0.7, 0.6), substeps=2), v.with_axle_grip(0.7, 0.6).rollout(state, U, substeps=2))
    assert np.array_equal(v.rollout(state, U, grip=(1.0, 1.0)), v.rollout(state, U))


# ---- 6: braking into a patch of half the grip -----------------------------------------------------------------------------------
BRAKE_V0 = 40.0
BRAKE_STEPS = 12


def _braking_speeds():
    """Full braking in a straight line from 40 m/s with tyre_coupling (1, 1), on waypoints 1.5 m apart along +x: the speed after 12
    steps on a table of ones and on one that is 0.5 from the fifth waypoint on."""
    from acmpc_amd import dynamic_model as dm
    steps = BRAKE_STEPS
    table = np.zeros((7, steps))
    table[0] = 1.5 * np.arange(steps)
    table[4], table[5], table[6] = 1.5, 8.0, BRAKE_V0
    U = np.tile([0.0, -1.0], (steps, 1))
    state = np.array([0.0, 0.0, 0.0, BRAKE_V0, 0.0, 0.0])
    patch = np.ones((steps, 2))
    patch[4:] = 0.5
    dry = dm.trace(_vehicle(), state, U, table, coupling=(1.0, 1.0), surface=np.ones((steps, 2)))
    wet = dm.trace(_vehicle(), state, U, table, coupling=(1.0, 1.0), surface=patch)
    return dry, wet


def test_full_braking_onto_a_patch_of_half_the_grip_sheds_less_speed():
    v = _vehicle()
    dry, wet = _braking_speeds()
    # the car is past the fifth waypoint after the first step (2 m a step against 1.5 m a waypoint) and at the last waypoint from
    # the sixth on: step 0 runs on waypoint 0's scale (the lag), every later step on the patch
    assert np.all(wet["j"] >= 1) and wet["j"][-1] == BRAKE_STEPS - 1
    first_on_patch = 1 + int(np.argmax(wet["j"] >= 4))
    assert first_on_patch <= 4
    assert np.array_equal(dry["states"][:first_on_patch + 1], wet["states"][:first_on_patch + 1])
    v_dry, v_wet = dry["states"][:, 3], wet["states"][:, 3]
    assert np.all(v_wet[first_on_patch + 1:] > v_dry[first_on_patch + 1:])
    # re-derived: in a straight line there is no side force, and each axle brakes with what the brake map asks of it or with its cap
    # rho P mu, whichever is less: the deceleration is (min(b bias, Pf mu) + min(b (1 - bias), Pr mu) + drag) / mass.  The front
    # axle is at its cap on both tables; the rear one only on the patch
    dt = 0.05
    for i in range(first_on_patch, BRAKE_STEPS):
        for run, mu in ((dry, 1.0), (wet, 0.5)):
            vx = run["states"][i, 3]
            brake = v.Cb1 - v.Cb2 * vx - v.Cb3 * vx ** 2
            assert brake * v.brake_bias > v.peak_front * mu
            assert (brake * (1 - v.brake_bias) > v.peak_rear * mu) == (mu == 0.5)
            drag = v.Cfric1 + v.Cfric2 * vx + v.Cfric3 * vx ** 2
            tyres = min(brake * v.brake_bias, v.peak_front * mu) + min(brake * (1 - v.brake_bias), v.peak_rear * mu)
            want = vx - dt * (tyres + drag) / v.mass
            assert abs(run["states"][i + 1, 3] - want) < 1e-9, (i, mu)
    assert 1.0 < v_wet[-1] - v_dry[-1] < 10.0


if __name__ == "__main__":
    for name, f in _mirror_figures().items():
        print("mirror, %-12s feasible on both sides %3d of %d, same set %s, max relative cost difference %.3e, same j %.4f"
              % (name, f["feasible"], MIRROR_CANDIDATES, f["same_feasible"], f["rel"], f["same_j"]))
    dry, wet = _braking_speeds()
    print("braking from %.0f m/s, %d steps: all 1 -> %.4f m/s, 0.5 from the fifth waypoint on -> %.4f m/s, difference %.4f m/s"
          % (BRAKE_V0, BRAKE_STEPS, dry["states"][-1, 3], wet["states"][-1, 3], wet["states"][-1, 3] - dry["states"][-1, 3]))
    print("j (patch):", wet["j"])
