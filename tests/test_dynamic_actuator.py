"""Mode D's actuator lag (acmpc_set_dynamics_actuator, acmpc_set_actuator_state), CPU only: the float64 mirror against the closed
forms of a first-order lag under a held command; the two identities of the float32 restatement (tests/dynamic_actuator_spec.py)
that the GPU tests repeat on the device - tau = (0, 0) and a constant command from its own position are the handle without the
setting; the handle's refusals and persistence without a device; the restatement against the float64 mirror on the problems of
tests/test_gpu_dynamic_actuator.py; and one physics statement: a steering step reaches less yaw through a lagging rack.

`python tests/test_dynamic_actuator.py` prints the measured figures the mirror's bound and DESIGN.md's numbers come from."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "ac-mpc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acmpc_oracle as orc  # noqa: E402
import dynamic_actuator_spec as das  # noqa: E402
import dynamic_spec as ds  # noqa: E402
import dynamic_surface_spec as dss  # noqa: E402
import test_dynamic_surface as tds  # noqa: E402
import test_gpu_dynamic_coupling as tgc  # noqa: E402
from dynamic_spec import Settings  # noqa: E402

T = np.float32
NAN, INF = float("nan"), float("inf")
EINVAL, ESTATE = -1, -5
DT = 0.05
TAU = (0.12, 0.06)            # the setting of every device case: 2.4 and 1.2 control steps
LOAD, AERO = tds.LOAD, tds.AERO
DEFAULT, FINE = tds.DEFAULT, tds.FINE
OFF, ALL_FOUR = tds.OFF, tds.ALL_FOUR
TIERS = tds.TIERS
FEW = 64
_same_where_finite = tds._same_where_finite
_vehicle = tds._vehicle

# max |J32 - J64| / max(|J64|, 1) over the candidates feasible on both sides (every candidate that is feasible on either: the test
# asserts it), the float32 restatement against the float64 mirror on the device tests' problems at N = 257, as this file's
# __main__ measures it (NumPy 1.26, x86-64): 3.704e-4, on the problem that starts from a standstill with
# n = 20 - the slip angles divide by vx + 1e-3 there, and the same problem without the lag measures 7.5e-4; the problems that
# start at the path's speed measure 6.4e-7.  Four times the worst is allowed for other seeds and compilers: 1.48e-3, below the
# 2.0e-3 of tests/test_dynamic_composed_float64.py (which leaves the standstill out)
MIRROR_MEASURED = 3.704e-4
MIRROR_RTOL = 4 * MIRROR_MEASURED


# ---- the problems of the device tests (tests/test_gpu_dynamic_actuator.py imports them) -----------------------------------------
SEED = 2801
_cache = {}


def problems(n, N, seed=SEED):
    """P = 2 dense problems (waypoints 1.5 m apart) of n steps and N candidates: problem 0 from a standstill, problem 1 at the
    path's speed, the forced candidates of test_gpu_dynamic_coupling among them (a NaN pedal, an inf steering, full brake and
    full drive).  Shared, never changed: a test that plants controls takes a copy."""
    key = (n, N, seed)
    if key not in _cache:
        _cache[key] = [dss.make_dense_problem(orc, n + 1, N, seed + p, vx0=v) for p, v in enumerate((0.0, None))]
        for d in _cache[key]:
            if N > 14:
                tgc._force_pedals(d["U"], n)
    return _cache[key]


def positions(P, seed):
    """[P, 2] float32 actuator positions inside the input box, different per problem."""
    rng = np.random.default_rng(8900 + seed)
    return np.column_stack([rng.uniform(-0.15, 0.15, P), rng.uniform(-0.5, 0.6, P)]).astype(T)


def coefficients_of(dp):
    return orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(T)


# ---- 1: the float64 mirror against the closed forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.0, 0.2, 1.0, 4.0])
def test_the_mirror_under_a_held_command_is_the_closed_form(ratio):
    from acmpc_amd import dynamic_model as dm
    n = 25
    tau = (ratio * DT, 0.5 * ratio * DT)
    k, m = dm.actuator_coefficients(tau, DT)
    for ch in range(2):
        if tau[ch] == 0.0:
            assert k[ch] == 0.0 and m[ch] == 0.0
        else:
            assert 0.0 < k[ch] < m[ch] < 1.0
            assert abs(k[ch] - np.exp(-DT / tau[ch])) <= 1e-15 and abs(m[ch] - tau[ch] / DT * (1.0 - k[ch])) <= 1e-15
    c, a0 = np.array([0.1, -0.6]), np.array([-0.05, 0.3])
    applied, pos = dm.actuator_response(np.tile(c, (n, 1)), a0, tau, DT)
    assert applied.shape == (n, 2) and pos.shape == (n + 1, 2)
    i = np.arange(n + 1)[:, None]
    assert np.max(np.abs(pos - (c - (c - a0) * k ** i))) <= 1e-12
    assert np.max(np.abs(applied - (c - m * (c - a0) * k ** i[:n]))) <= 1e-12
    if ratio == 0.0:
        assert np.array_equal(applied, np.tile(c, (n, 1))) and np.array_equal(pos[1:], np.tile(c, (n, 1)))
    # cleared positions: the first command stands for them, and a held command is then applied as it is
    applied, pos = dm.actuator_response(np.tile(c, (n, 1)), None, tau, DT)
    assert np.array_equal(applied, np.tile(c, (n, 1))) and np.array_equal(pos, np.tile(c, (n + 1, 1)))
    for bad in ((-0.1, 0.0), (0.1, NAN), (INF, 0.1)):
        with pytest.raises(ValueError):
            dm.actuator_coefficients(bad, DT)


def test_the_interval_mean_is_the_integral_of_the_exact_response():
    """m: the mean over [0, dt] of exp(-t / tau), by a fine quadrature of the exact first-order response."""
    from acmpc_amd import dynamic_model as dm
    tau = (0.12, 0.03)
    k, m = dm.actuator_coefficients(tau, DT)
    t = (np.arange(200000) + 0.5) * (DT / 200000)
    for ch in range(2):
        assert abs(np.mean(np.exp(-t / tau[ch])) - m[ch]) <= 1e-10


def test_the_restatements_filter_is_the_mirror_rounded():
    from acmpc_amd import dynamic_model as dm
    rng = np.random.default_rng(5)
    U = np.column_stack([rng.uniform(-0.3, 0.3, 40), rng.uniform(-1, 1, 40)]).astype(T)
    for a0 in (None, (0.1, -0.2)):
        got = das.filter_controls(U, a0, TAU, DT)
        want = dm.actuator_response(U, a0, TAU, DT)
        for g, w in zip(got, want):
            assert g.dtype == T and np.max(np.abs(g - w)) <= 2e-6
    k, m = das.coefficients(TAU, DT)
    k64, m64 = dm.actuator_coefficients(TAU, DT)
    assert k == tuple(T(v) for v in k64) and m == tuple(T(v) for v in m64)


# ---- 2: the identities of the restatement ---------------------------------------------------------------------------------------
def _same_values(got, want, label):
    """`==` on every candidate whose reference value is not a NaN, a NaN where it is one."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), label
    assert np.array_equal(got[~nan], want[~nan]), label


def _identity(dp, coef, s, surface, label, **lag):
    vehicle = _vehicle().coefficients()
    kw = dict(nn_window=(2, 5), return_states=True, u_prev=(0.02, -0.1) if s.rate_max is not None else None)
    got = das.spec_costs(orc, dp, coef, vehicle, settings=s, surface=surface, **lag, **kw)
    # the same handle with the setting off: the top-tier step it takes under the setting, on the command
    off = dss.spec_costs(orc, dp, coef, vehicle, settings=dss.surface_settings(s), surface=surface, **kw)
    for x, y in zip(got[:2], off[:2]):
        _same_values(x, y, label)
    # the trajectories of the candidates with a cost (a NaN command stays in the actuator's position, so that a candidate that
    # has one - its cost is a NaN either way - is rolled on NaN controls from there on)
    fine = ~np.isnan(off[0])
    _same_values(got[2][fine], off[2][fine], label)
    # and the plain handle, wherever that one's values are finite
    if surface is None:
        plain = ds.spec_costs(orc, dp, coef, vehicle, settings=s, **kw)
        for x, y in zip(got[:2], plain[:2]):
            _same_where_finite(x, y, label)
    return got


def _settings(integration, setting, step):
    return Settings(*integration, **setting[0], **setting[1], **step)


@pytest.mark.parametrize("tier", list(TIERS))
def test_zero_time_constants_are_the_handle_without_the_setting(tier):
    n = tds.n
    for name, (dp, coef) in (("standard", tds._standard(N=FEW)), ("dense", tds._dense(N=FEW))):
        tgc._force_pedals(dp["U"], n)
        for integration, setting in ((DEFAULT, OFF), (FINE, ALL_FOUR)):
            s = _settings(integration, setting, TIERS[tier])
            for surface in (None, dss.random_table(n, 3)):
                for a0 in (None, (0.1, -0.4)):
                    _identity(dp, coef, s, surface, (name, tier, integration, surface is not None, a0), actuator=(0.0, 0.0), a0=a0)


@pytest.mark.parametrize("tier", ["none", "all-with-downforce"])
def test_a_constant_command_from_its_own_position_is_the_handle_without_the_setting(tier):
    n = tds.n
    dp, coef = tds._dense(N=FEW)
    held = dict(dp, U=np.repeat(dp["U"][:, :1], n, axis=1))          # every plan holds its own first command
    one = dict(dp, U=np.tile(np.array([0.04, 0.3], dtype=T), (FEW, n, 1)))
    for integration, setting in ((DEFAULT, OFF), (FINE, ALL_FOUR)):
        s = _settings(integration, setting, TIERS[tier])
        for surface in (None, dss.random_table(n, 4)):
            label = (tier, integration, surface is not None)
            _identity(held, coef, s, surface, label, actuator=TAU, a0=None)                 # cleared: e = +0 in every step
            _identity(one, coef, s, surface, label, actuator=(0.5, 0.01), a0=(0.04, 0.3))   # given: the command itself
    # and the lag does something as soon as the command moves
    vehicle = _vehicle().coefficients()
    lagged = das.spec_costs(orc, dp, coef, vehicle, actuator=TAU)[0]
    plain = das.spec_costs(orc, dp, coef, vehicle, actuator=(0.0, 0.0))[0]
    assert np.count_nonzero(ds.bits(lagged) != ds.bits(plain)) > FEW // 2


def test_without_the_setting_the_restatement_is_the_surface_restatement():
    n = tds.n
    dp, coef = tds._dense(N=FEW)
    vehicle = _vehicle().coefficients()
    for surface in (None, dss.random_table(n, 3)):
        a = das.spec_costs(orc, dp, coef, vehicle, surface=surface, return_states=True)
        b = dss.spec_costs(orc, dp, coef, vehicle, surface=surface, return_states=True)
        for x, y in zip(a, b):
            assert np.array_equal(ds.bits(x), ds.bits(y))
    assert ds.control_step.__module__ == "dynamic_spec" and ds.control_step.__name__ == "control_step"   # (put back)


def test_the_trace_keeps_the_command_in_its_slots_and_the_lagged_trajectory_in_its_states():
    n = tds.n
    dp, coef = tds._dense(N=FEW)
    vehicle = _vehicle().coefficients()
    s = _settings(FINE, ALL_FOUR, TIERS["all-with-downforce"])
    on, off = {}, {}
    a0 = (0.1, -0.4)
    das.spec_costs(orc, dp, coef, vehicle, settings=s, u_prev=(0.02, -0.1), actuator=TAU, a0=a0, trace=on)
    dss.spec_costs(orc, dp, coef, vehicle, settings=dss.surface_settings(s), u_prev=(0.02, -0.1), trace=off)
    assert ds.TERM_FLOATS == 22
    assert not np.array_equal(ds.bits(on["states"][:, 1:]), ds.bits(off["states"][:, 1:]))
    lo, hi = np.asarray(dp["kw"]["u_min"], dtype=T), np.asarray(dp["kw"]["u_max"], dtype=T)
    U = dp["U"]
    # slots 5, 6: the box's hinges on the command; 8, 9: the rates' hinges, the same numbers with and without the lag
    assert np.array_equal(ds.bits(on["terms"][..., ds.BOX]), ds.bits(U[..., 0] - np.fmin(np.fmax(U[..., 0], lo[0]), hi[0])))
    assert np.array_equal(ds.bits(on["terms"][..., ds.BOX + 1]), ds.bits(U[..., 1] - np.fmin(np.fmax(U[..., 1], lo[1]), hi[1])))
    assert np.array_equal(ds.bits(on["terms"][..., ds.RATE:ds.RATE + 2]), ds.bits(off["terms"][..., ds.RATE:ds.RATE + 2]))
    # slot 4: dk = delta_i - delta_ref of the waypoint this (lagged) trajectory is nearest to
    delta_ref = ds.atan_spec(T(dp["kw"]["wheelbase"]) * coef[:, 5])
    assert np.array_equal(ds.bits(on["terms"][..., ds.DK]), ds.bits(U[..., 0] - delta_ref[on["j"]]))
    assert np.array_equal(ds.bits(ds.replay(on["terms"])), ds.bits(on["terms"][..., ds.V_SLOT]))


# ---- 5: the handle, without a device --------------------------------------------------------------------------------------------
def _set_tau(eng, tau):
    tau = None if tau is None else np.ascontiguousarray(tau, dtype=np.float64)
    return eng._lib.acmpc_set_dynamics_actuator(eng._ctx, None if tau is None else tau.ctypes.data)


def _set_state(eng, a0, P):
    a0 = None if a0 is None else np.ascontiguousarray(a0, dtype=T)
    return eng._lib.acmpc_set_actuator_state(eng._ctx, None if a0 is None else a0.ctypes.data, P)


def test_the_entry_points_are_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    lib = acmpc_amd.load_library()
    for name in ("acmpc_set_dynamics_actuator", "acmpc_set_actuator_state"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert hasattr(acmpc_amd.Engine, "set_dynamics_actuator") and hasattr(acmpc_amd.Engine, "set_actuator_state")


def test_refusals_leave_the_handle_as_it_was_and_the_setting_survives_the_other_setters():
    from acmpc_amd import EngineError
    P, steps = 2, 5
    eng, dp = tds._engine(P=P, steps=steps)
    eng.set_dynamics(_vehicle())
    state = np.full((P, 2), 0.1, dtype=T)
    assert tds._solve_code(eng, dp, 1, 4) != ESTATE
    assert _set_tau(eng, TAU) == 0 and _set_state(eng, state, P) == 0
    assert tds._solve_code(eng, dp, P, steps) != ESTATE
    # positions for another P: the next call is refused, whichever it is, and says why
    assert tds._solve_code(eng, dp, P - 1, steps) == ESTATE and b"acmpc_set_actuator_state" in eng._lib.acmpc_last_error(eng._ctx)
    assert tds._trace_code(eng, dp, P - 1, steps) == ESTATE and tds._trace_code(eng, dp, P, steps) != ESTATE
    # refused time constants: EINVAL, and the handle keeps what it had
    for bad in ((-0.1, 0.1), (0.1, -1e-9), (NAN, 0.1), (0.1, NAN), (INF, 0.1), (0.1, -INF)):
        assert _set_tau(eng, bad) == EINVAL, bad
        assert b"tau" in eng._lib.acmpc_last_error(eng._ctx)
    with pytest.raises(EngineError) as e:
        eng.set_dynamics_actuator((0.1, -0.2))
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        eng.set_dynamics_actuator((0.1, 0.2, 0.3))
    assert _set_state(eng, state, P + 1) == EINVAL and _set_state(eng, state, 0) == EINVAL
    assert tds._solve_code(eng, dp, P, steps) != ESTATE and tds._solve_code(eng, dp, 1, steps) == ESTATE
    # the Engine's shorter form: [2] is one problem's
    eng.set_actuator_state((0.1, -0.2))
    assert tds._solve_code(eng, dp, 1, steps) != ESTATE and tds._solve_code(eng, dp, P, steps) == ESTATE
    # None, or NULL, clears the positions; the shape check goes with them
    for clear in (lambda: eng.set_actuator_state(None), lambda: _set_state(eng, None, 0)):
        eng.set_actuator_state(state)
        assert tds._solve_code(eng, dp, 1, steps) == ESTATE
        assert clear() in (0, None)
        assert tds._solve_code(eng, dp, 1, steps) != ESTATE
    # (0, 0) is a setting, None turns it off; both are accepted, and so is the other form of each
    for tau in ((0.0, 0.0), None, (0.0, 0.2), TAU):
        assert _set_tau(eng, tau) == 0
    eng.set_dynamics_actuator(None)
    eng.set_dynamics_actuator(TAU)
    # the positions are kept while the setting is off, and both survive the other setters
    eng.set_actuator_state(state)
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
    eng.set_surface(np.full((P, steps, 2), 0.7, dtype=T))
    eng.set_surface(None)
    eng.set_previous_control(np.zeros((P, 2), dtype=T))
    eng.set_previous_control(None)
    eng.set_dynamics_ensemble([_vehicle(), _vehicle().with_grip(0.6)])
    eng.set_dynamics(_vehicle())
    assert tds._solve_code(eng, dp, 1, steps) == ESTATE and tds._solve_code(eng, dp, P, steps) != ESTATE
    lib = eng._lib
    eng.close()
    for mode in (0, 1):
        other, _ = tds._engine(mode=mode)
        assert _set_tau(other, TAU) == ESTATE and _set_tau(other, None) == ESTATE
        assert _set_state(other, state, P) == ESTATE and _set_state(other, None, 0) == ESTATE
        with pytest.raises(EngineError) as e:
            other.set_dynamics_actuator(TAU)
        assert e.value.code == ESTATE
        other.close()
    assert lib.acmpc_set_dynamics_actuator(None, None) == EINVAL and lib.acmpc_set_actuator_state(None, None, 0) == EINVAL


def test_the_solver_and_the_controller_take_the_key_without_device_work():
    import inspect
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    assert "actuator_state" in inspect.signature(DynamicSamplingSolver.solve).parameters
    assert "actuator_lag" in sys.modules[DynamicSamplingSolver.__module__].__doc__


# ---- 6: float32 against float64 -------------------------------------------------------------------------------------------------
MIRROR_N = 257
MIRROR_SETTINGS = dict(coupling=(0.9, 1.1), load_transfer=LOAD, downforce=AERO)
MIRROR_CASES = [(3, True, True), (20, True, False), (20, False, True)]      # (n, a surface table, positions given)


def _mirror_cost(dp, U, n, table, actuator):
    """(cost, V) of one plan from dynamic_model.trace in float64 under the lag: the weighted sums of what its lines saw."""
    from acmpc_amd import dynamic_model as dm
    kw = dp["kw"]
    out = dm.trace(_vehicle(), dp["x0"], U, dp["table"], dt=kw["dt"], u_min=np.asarray(kw["u_min"], dtype=T),
                   u_max=np.asarray(kw["u_max"], dtype=T), margin=kw["margin"], wheelbase=kw["wheelbase"], surface=table,
                   actuator=actuator, **MIRROR_SETTINGS)
    Q, R, QN = (np.asarray(kw[k], dtype=np.float64) for k in ("step_cost", "r_term", "final_cost"))
    tN = n * kw["dt"]
    stage = 0.5 * (Q[0] * np.sum(out["e_y"] ** 2) + Q[1] * np.sum(out["e_psi"] ** 2) + R[0] * np.sum(out["dv"] ** 2)
                   + R[1] * np.sum(out["dk"] ** 2))
    terminal = 0.5 * (QN[0] * out["e_y"][-1] ** 2 + QN[1] * out["e_psi"][-1] ** 2 + QN[2] * tN ** 2)
    V = float(out["V"][-1])
    return stage + terminal + kw["w_bound"] * V, V


def _mirror_figures():
    figures = {}
    for n, with_table, with_state in MIRROR_CASES:
        for p, dp in enumerate(problems(n, MIRROR_N)):
            coef = coefficients_of(dp)
            table = dss.random_table(n, 70 + p) if with_table else None
            a0 = positions(2, 71)[p] if with_state else None
            c32, V32 = das.spec_costs(orc, dp, coef, _vehicle().coefficients(), settings=Settings(**MIRROR_SETTINGS), surface=table,
                                      actuator=TAU, a0=a0)
            ok = np.isfinite(dp["U"]).all(axis=(1, 2))      # (the mirror is not asked about a NaN pedal or an inf steering)
            c64, V64 = np.full(MIRROR_N, NAN), np.full(MIRROR_N, NAN)
            for c in np.flatnonzero(ok):
                c64[c], V64[c] = _mirror_cost(dp, dp["U"][c], n, table, (TAU, a0))
            assert not np.isfinite(c32[~ok]).any()
            both = (V32 == 0) & (V64 == 0)
            rel = np.abs(c32.astype(np.float64) - c64) / np.maximum(np.abs(c64), 1.0)
            figures[(n, with_table, with_state, p)] = dict(same_feasible=bool(np.array_equal((V32 == 0)[ok], (V64 == 0)[ok])),
                                                           feasible=int(both.sum()), rel=float(rel[both].max()))
    return figures


def test_the_restatement_against_the_float64_mirror():
    for case, f in _mirror_figures().items():
        assert f["same_feasible"] and f["feasible"] > MIRROR_N // 2, (case, f)     # none left out, and most are compared
        assert f["rel"] <= MIRROR_RTOL, (case, f)


STEER_V0, STEER_TO, STEER_TAU, STEER_STEPS = 25.0, 0.1, 0.15, 10


def steering_step_problem():
    """A straight path along +x, waypoints 1.5 m apart, and the plan that steps the steering from 0 to 0.1 rad at step 0 with the
    pedal at 0, from 25 m/s with the rack at 0: (dp, coef, U [1, n, 2], a0)."""
    n = STEER_STEPS
    dp = dict(problems(n, MIRROR_N)[1])
    table = np.array(dp["table"], dtype=np.float64)
    table[0] = table[0, 0] + 1.5 * np.arange(table.shape[1])
    table[1], table[2], table[3] = table[1, 0], 0.0, 0.0
    table[4], table[6] = 1.5, STEER_V0
    x0 = np.array([table[0, 0], table[1, 0], 0.0, STEER_V0, 0.0, 0.0], dtype=T)
    dp.update(table=table.astype(dp["table"].dtype), x0=x0)
    U = np.tile(np.array([STEER_TO, 0.0], dtype=T), (1, n, 1))
    return dp, coefficients_of(dp), U, np.zeros(2, dtype=T)


def _steering_yaws():
    """Yaw after the ten steps with tau_d = 0.15 and with tau_d = 0: (float64 mirror, float32 restatement)."""
    dp, coef, U, a0 = steering_step_problem()
    out = []
    for tau in ((STEER_TAU, 0.0), (0.0, 0.0)):
        s64 = _vehicle().rollout(dp["x0"].astype(np.float64), U[0].astype(np.float64), DT, actuator=(tau, a0))
        trace = {}
        das.spec_costs(orc, dp, coef, _vehicle().coefficients(), U=U, actuator=tau, a0=a0, trace=trace)
        out.append((float(s64[-1, 2]), float(trace["states"][0, -1, 2])))
    return out


def test_a_steering_step_reaches_less_yaw_through_a_lagging_rack():
    (lag64, lag32), (now64, now32) = _steering_yaws()
    assert 0.0 < lag64 < now64 and 0.0 < lag32 < now32
    assert abs(lag32 - lag64) < 1e-4 and abs(now32 - now64) < 1e-4
    # re-derived: the rack has covered 1 - m k^i of the step during control step i
    from acmpc_amd import dynamic_model as dm
    k, m = dm.actuator_coefficients((STEER_TAU, 0.0), DT)
    applied, _ = dm.actuator_response(np.tile([STEER_TO, 0.0], (STEER_STEPS, 1)), (0.0, 0.0), (STEER_TAU, 0.0), DT)
    assert np.max(np.abs(applied[:, 0] - STEER_TO * (1.0 - m[0] * k[0] ** np.arange(STEER_STEPS)))) < 1e-15
    assert np.array_equal(applied[:, 1], np.zeros(STEER_STEPS))


if __name__ == "__main__":
    worst = 0.0
    for case, f in _mirror_figures().items():
        worst = max(worst, f["rel"])
        print("mirror, n %2d table %-5s positions %-5s problem %d: feasible on both sides %3d of %d, same set %s, max relative "
              "cost difference %.3e" % (case + (f["feasible"], MIRROR_N, f["same_feasible"], f["rel"])))
    print("worst %.3e (tests/test_dynamic_composed_float64.py allows 2.0e-3)" % worst)
    (lag64, lag32), (now64, now32) = _steering_yaws()
    print("steering step 0 -> %.1f rad from %.0f m/s, yaw after %d steps: tau_d = %.2f -> %.6f (float32 %.6f), tau_d = 0 -> %.6f "
          "(float32 %.6f)" % (STEER_TO, STEER_V0, STEER_STEPS, STEER_TAU, lag64, lag32, now64, now32))
