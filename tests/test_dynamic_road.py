"""Mode D's road table (acmpc_set_road), CPU only: the float32 restatement (tests/dynamic_road_spec.py) pinned against the
restatements it extends under the neutral row (0, 0, 1), its power-of-two identity against the surface table, the physics of the
float64 mirror (dynamic_model's `road=`), dynamic_model.road_table, the mirror against the restatement over the committed runs
of tests/test_dynamic_trace.py with a seeded road table, and every refusal of acmpc_set_road on a handle without a device.

`python tests/test_dynamic_road.py` prints the measured figures the mirror's bounds and DESIGN.md's numbers come from."""
import functools
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
import dynamic_road_spec as drs  # noqa: E402
import dynamic_spec as ds  # noqa: E402
import dynamic_surface_spec as dss  # noqa: E402
import test_dynamic_surface as tds  # noqa: E402
import test_dynamic_trace as tdt  # noqa: E402
import test_gpu_dynamic_coupling as tgc  # noqa: E402
from dynamic_spec import Settings  # noqa: E402

T = np.float32
NAN, INF = float("nan"), float("inf")
EINVAL, ESTATE = -1, -5
n = tds.n
FEW = tds.FEW
TAU = (0.12, 0.06)
DEFAULT, FINE = tds.DEFAULT, tds.FINE
OFF, ALL_FOUR = tds.OFF, tds.ALL_FOUR
TIERS = tds.TIERS
_vehicle = tds._vehicle
_same_where_finite = tds._same_where_finite
NEUTRAL = np.tile(np.array([0.0, 0.0, 1.0], dtype=T), (n, 1))

# Worst |float64 mirror - float32 restatement| over the committed runs below - the sixteen of tests/test_dynamic_trace.py (four
# settings x all / windowed search x with / without discs, four plans of twelve steps each), every one under the seeded road
# table and once more with a seeded surface table beside it: thirty-two runs - as this file's __main__ measures them (NumPy 1.26,
# x86-64): the six states MEASURED_STATE, the hinges and the cost lines' operands MEASURED_HINGE.  Held at
# 4x the measured value, the project's convention: other seeds, other compilers' libm.
MEASURED_STATE, MEASURED_HINGE = 7.1e-6, 7.1e-6     # (7.00e-6 both, under "terms" with the surface table)
STATE_TOL, HINGE_TOL = 4 * MEASURED_STATE, 4 * MEASURED_HINGE


def _bits_differ_only_in_the_sign_of_a_zero(a, b, label):
    """Bit-identical, except where both sides are a zero (x + (+0) turns a -0 into +0); returns the count of such places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != T:
        assert np.array_equal(a, b), label
        return 0
    differ = ds.bits(a) != ds.bits(b)
    assert np.all((a[differ] == 0) & (b[differ] == 0)), label
    return int(np.count_nonzero(differ))


# ---- 1: pinning the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", list(TIERS))
def test_with_the_neutral_row_the_restated_step_is_dynamic_specs(tier):
    rng = np.random.default_rng(3001)
    count = 512
    state = [rng.uniform(-5, 5, count), rng.uniform(-5, 5, count), rng.uniform(-3, 3, count), rng.uniform(0, 40, count),
             rng.uniform(-2, 2, count), rng.uniform(-1, 1, count)]
    state = [np.asarray(s, dtype=T) for s in state]
    state[3][:8] = 0.0                                  # standstill lanes, two of them with nothing moving at all
    state[4][:2] = state[5][:2] = 0.0
    delta, pedal = rng.uniform(-0.3, 0.3, count).astype(T), rng.uniform(-1, 1, count).astype(T)
    delta[:2], pedal[:2] = 0.0, (0.0, -0.0)
    zeros = 0
    for vehicle in (_vehicle(), _vehicle().with_grip(0.5)):
        c = ds.constants(vehicle.coefficients(), Settings(**TIERS[tier]), 0.05)
        for h in (None, T(0.0125)):
            want = ds.dynamic_step(state, delta, pedal, c, h)
            got = drs.road_step(state, delta, pedal, c, T(0.0), T(0.0), h)
            for q in range(6):
                zeros += _bits_differ_only_in_the_sign_of_a_zero(got[q], want[q], (tier, q))
            moved = drs.road_step(state, delta, pedal, c, T(0.5), T(-0.7), h)
            dt = c.h if h is None else h
            assert all(np.array_equal(ds.bits(moved[q]), ds.bits(want[q])) for q in (0, 1, 2, 5))
            assert np.allclose(moved[4] - want[4], T(-0.7) * dt, atol=1e-6) and np.all(moved[3] >= want[3])
    assert zeros <= 2 * 2 * 2 * 2                       # at most vx' and vy' of the two lanes at rest, per vehicle and step


@pytest.mark.parametrize("tier", list(TIERS))
def test_with_the_neutral_table_the_rollout_is_the_actuators_restatement(tier):
    vehicle = _vehicle().coefficients()
    zeros, cases = 0, 0
    for name, (dp, coef) in (("standard", tds._standard(N=FEW)), ("dense", tds._dense(N=FEW)), ("standstill", tds._dense(vx0=0.0, N=FEW))):
        tgc._force_pedals(dp["U"], n)
        discs = ds.make_obstacles(dp, n, 2, 7)
        for integration, setting, prev in ((DEFAULT, OFF, None), (FINE, ALL_FOUR, (0.02, -0.1))):
            for surface in (None, dss.random_table(n, 3)):
                for obstacles in (None, discs):
                    for actuator, a0, window in ((None, None, None), (TAU, (0.05, 0.2), (2, 5))):
                        s = Settings(*integration, **setting[0], **setting[1], clearance_weight=40.0, clearance_margin=1.0,
                                     **TIERS[tier])
                        kw = dict(nn_window=window, settings=s, u_prev=prev, obstacles=obstacles, surface=surface,
                                  actuator=actuator, a0=a0, return_states=True)
                        want, got = {}, {}
                        b = drs.spec_costs(orc, dp, coef, vehicle, road=NEUTRAL, trace=got, **kw)
                        # the neutral table takes the top-tier step, as a surface table does: against that, bit for bit
                        # up to the sign of a zero; against the handle as it is, wherever its values are finite
                        a = das.spec_costs(orc, dp, coef, vehicle, trace=want, **dict(kw, settings=dss.surface_settings(s)))
                        label = (name, tier, integration, surface is not None, obstacles is not None, actuator, window)
                        for x, y in zip(a, b):
                            zeros += _bits_differ_only_in_the_sign_of_a_zero(y, x, label)
                        for key in ("states", "terms", "totals", "j", "E"):
                            zeros += _bits_differ_only_in_the_sign_of_a_zero(got[key], want[key], label)
                        assert np.array_equal(got["road_j"][:, 1:], got["j"][:, :-1]) and not got["road_j"][:, 0].any()
                        plain = das.spec_costs(orc, dp, coef, vehicle, **kw)
                        for x, y in zip(b[:2], plain[:2]):
                            finite = np.isfinite(y)
                            assert np.array_equal(np.isfinite(x), finite), label
                            assert np.array_equal(x[finite], y[finite]), label
                        cases += 1
    assert cases == 3 * 2 * 2 * 2 * 2
    print("neutral table, tier %s: %d cases, %d values differ in the sign of a zero" % (tier, cases, zeros))


def test_without_a_table_the_restatement_is_the_actuators_bit_for_bit():
    dp, coef = tds._dense(N=FEW)
    vehicle = _vehicle().coefficients()
    s = Settings(*FINE, **ALL_FOUR[0], **ALL_FOUR[1], **TIERS["loaded-coupled"])
    for actuator in (None, TAU):
        kw = dict(settings=s, u_prev=(0.02, -0.1), surface=dss.random_table(n, 3), actuator=actuator, return_states=True)
        for x, y in zip(drs.spec_costs(orc, dp, coef, vehicle, **kw), das.spec_costs(orc, dp, coef, vehicle, **kw)):
            assert np.array_equal(ds.bits(x), ds.bits(y))


# ---- 2: the power-of-two identity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", list(TIERS))
def test_a_uniform_power_of_two_load_factor_is_the_surface_table_of_that_scale(tier):
    vehicle = _vehicle().coefficients()
    road = lambda nz: np.tile(np.array([0.0, 0.0, nz], dtype=T), (n, 1))      # noqa: E731
    mu = lambda m: np.full((n, 2), m, dtype=T)                                # noqa: E731
    for dp, coef in (tds._dense(N=FEW), tds._standard(N=FEW)):
        tgc._force_pedals(dp["U"], n)
        for integration in (DEFAULT, FINE):
            s = Settings(*integration, **ALL_FOUR[0], **ALL_FOUR[1], **TIERS[tier])
            kw = dict(settings=s, u_prev=(0.02, -0.1), nn_window=(2, 5), return_states=True)
            pairs = ((dict(road=road(0.5)), dict(road=NEUTRAL, surface=mu(0.5))),
                     (dict(road=road(0.25), surface=mu(0.5)), dict(road=NEUTRAL, surface=mu(0.125))))
            for got_kw, want_kw in pairs:
                got = drs.spec_costs(orc, dp, coef, vehicle, **kw, **got_kw)
                want = drs.spec_costs(orc, dp, coef, vehicle, **kw, **want_kw)
                for x, y in zip(got, want):
                    assert np.array_equal(ds.bits(x), ds.bits(y)), (tier, integration)
            # and the neutral road over a surface table is that surface table alone, up to the sign of a zero
            alone = dss.spec_costs(orc, dp, coef, vehicle, surface=mu(0.5), **kw)
            for x, y in zip(drs.spec_costs(orc, dp, coef, vehicle, road=NEUTRAL, surface=mu(0.5), **kw), alone):
                _bits_differ_only_in_the_sign_of_a_zero(x, y, tier)


def test_a_random_table_reaches_every_cost_and_lags_by_one_step():
    dp, coef = tds._dense()
    vehicle = _vehicle().coefficients()
    road = drs.random_road(n, 1)
    trace = {}
    got = drs.spec_costs(orc, dp, coef, vehicle, road=road, trace=trace)[0]
    j = trace["j"]
    assert j.max() >= 3 and any(len(np.unique(j[:, i])) > 1 for i in range(n))
    assert np.array_equal(trace["road_j"][:, 1:], j[:, :-1]) and not trace["road_j"][:, 0].any()
    plain = drs.spec_costs(orc, dp, coef, vehicle, road=NEUTRAL)[0]
    finite = np.isfinite(plain)
    assert np.count_nonzero(ds.bits(got)[finite] != ds.bits(plain)[finite]) == np.count_nonzero(finite)
    # the row lags by one control step: a table that is neutral at every waypoint a candidate has left from by the last step's
    # start changes nothing
    flat = {}
    again = drs.spec_costs(orc, dp, coef, vehicle, road=NEUTRAL, trace=flat)[0]
    last = int(flat["road_j"].max())
    late = NEUTRAL.copy()
    late[last + 1:] = drs.random_road(n, 2)[last + 1:]
    assert np.array_equal(ds.bits(drs.spec_costs(orc, dp, coef, vehicle, road=late)[0]), ds.bits(again))


# ---- 3: physics, on the float64 mirror ------------------------------------------------------------------------------------------
MIRROR_STEP = dict(coupling=(1.0, 1.0), load_transfer=tds.LOAD, downforce=tds.AERO)


def test_the_road_adds_its_two_accelerations_and_nothing_else():
    v = _vehicle()
    state, u = np.array([0.0, 0.0, 0.1, 20.0, 0.3, 0.1]), np.array([0.05, -0.6])
    for step in (dict(), MIRROR_STEP):
        flat = v.predict_next_state(state, u, 0.05, **step)
        for a_x, a_y in ((0.59, 0.0), (-0.59, 1.1), (0.0, -1.1)):
            road = v.predict_next_state(state, u, 0.05, road=(a_x, a_y, 1.0), **step)
            assert abs(road[1][3] - flat[1][3] - a_x) < 1e-12 and abs(road[1][4] - flat[1][4] - a_y) < 1e-12
            assert road[1][5] == flat[1][5] and np.array_equal(road[1][:3], flat[1][:3]) and road[2] == flat[2]
            assert np.allclose(road[0], state + road[1] * 0.05, rtol=0, atol=1e-15)
        # n_z scales the peaks and only them: the step of the vehicle with both peak factors scaled, composed with the surface's
        a = v.predict_next_state(state, u, 0.05, road=(0.3, -0.2, 0.9), grip=(0.7, 0.6), **step)
        b = v.with_axle_grip(0.7 * 0.9, 0.6 * 0.9).predict_next_state(state, u, 0.05, road=(0.3, -0.2, 1.0), **step)
        assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    U = np.tile(u, (5, 1))
    assert np.array_equal(v.rollout(state, U, road=(0.0, 0.0, 1.0), substeps=2), v.rollout(state, U, substeps=2))
    assert not np.array_equal(v.rollout(state, U, road=(0.5, 0.0, 1.0), substeps=2), v.rollout(state, U, substeps=2))


COAST_V0, COAST_T, COAST_GRADE = 20.0, 2.0, 0.06


def _coast():
    """Coasting in a straight line from 20 m/s for 2 s on the flat, on a 6 % downhill and on the 6 % uphill: the three final
    speeds, a_x, and the bound on what the drag's speed dependence takes from a_x t."""
    v = _vehicle()
    steps = int(round(COAST_T / 0.05))
    theta = np.arctan(COAST_GRADE)
    a_x, n_z = v.g * np.sin(theta), np.cos(theta)
    state, U = np.array([0.0, 0.0, 0.0, COAST_V0, 0.0, 0.0]), np.zeros((steps, 2))
    flat = v.rollout(state, U, 0.05)[-1, 3]
    down = v.rollout(state, U, 0.05, road=(a_x, 0.0, n_z))[-1, 3]
    up = v.rollout(state, U, 0.05, road=(-a_x, 0.0, n_z))[-1, 3]
    # With D(v) = Cfric1 + Cfric2 v + Cfric3 v^2 the drag and D' = Cfric2 + 2 Cfric3 v >= 0 its slope, the difference e of two
    # Euler runs obeys e' = a_x - (D(v_a) - D(v_b)) / m: 0 <= a_x t - e <= (D'max / m) a_x t^2 / 2, D'max the slope at the
    # highest speed either run can reach, v0 + a_x t
    slope = (v.Cfric2 + 2.0 * v.Cfric3 * (COAST_V0 + a_x * COAST_T)) / v.mass
    return flat, down, up, a_x, slope * a_x * COAST_T ** 2 / 2.0


def test_coasting_downhill_ends_faster_and_uphill_slower_by_gravity_times_time():
    flat, down, up, a_x, slack = _coast()
    assert up < flat < down
    assert 0.5 < a_x < 0.6 and 0.0 < slack < 0.25 * a_x * COAST_T
    for gained in (down - flat, flat - up):
        assert a_x * COAST_T - slack - 1e-9 <= gained <= a_x * COAST_T + 1e-9, (gained, a_x * COAST_T, slack)


BANK_V, BANK_R, BANK = 15.0, 60.0, 0.10
UNDERSTEER = (0.8, 1.0)       # the front axle's grip scaled down: a car that understeers, as road cars are set up to


def _steady_steering(vehicle, road):
    """(delta, vy) that hold the left circle of radius 60 m at 15 m/s with the pedal at 0: xd4 = xd5 = 0 at r = v / R, by Newton's
    method on the mirror's x_dot with a numerical Jacobian."""
    r = BANK_V / BANK_R

    def residual(z):
        x_dot = vehicle.predict_next_state(np.array([0.0, 0.0, 0.0, BANK_V, z[1], r]), (z[0], 0.0), 0.05, road=road)[1]
        return np.array([x_dot[4], x_dot[5]])

    z = np.array([(vehicle.lf + vehicle.lr) / BANK_R, 0.0])
    for _ in range(50):
        f = residual(z)
        J = np.stack([(residual(z + e) - f) / 1e-7 for e in (np.array([1e-7, 0.0]), np.array([0.0, 1e-7]))], axis=1)
        z = z - np.linalg.solve(J, f)
    assert np.max(np.abs(residual(z))) < 1e-9
    return z


def test_a_left_hand_bank_needs_less_steering_for_the_same_left_circle():
    """The steady steering angle is the Ackermann angle L / R plus the difference of the axles' slip angles, and a bank takes
    lateral force - and with it slip angle - off both axles.  So on a car that understeers (the front slips more: delta above
    L / R on the flat) the banked corner needs LESS steering, which is the statement; the reference block as it stands oversteers
    slightly at this speed (delta below L / R on the flat: its rear axle carries more load per unit of cornering stiffness), and
    there the same bank brings delta UP towards L / R.  Both are asserted: the angle moves towards L / R, from whichever side."""
    for vehicle, understeers in ((_vehicle().with_axle_grip(*UNDERSTEER), True), (_vehicle(), False)):
        ackermann = (vehicle.lf + vehicle.lr) / BANK_R
        road = (0.0, vehicle.g * np.sin(BANK), np.cos(BANK))
        flat, banked = _steady_steering(vehicle, None)[0], _steady_steering(vehicle, road)[0]
        assert (flat > ackermann) == understeers, (flat, ackermann)
        assert abs(banked - ackermann) < abs(flat - ackermann), (flat, banked, ackermann)
        if understeers:
            assert 0.0 < ackermann < banked < flat, (banked, flat)
        # and in both the tyres' side force is smaller: the sideslip velocity the circle needs moves with it
        off_camber = _steady_steering(vehicle, (0.0, -road[1], road[2]))[0]
        assert abs(off_camber - ackermann) > abs(flat - ackermann)


# ---- 4: road_table --------------------------------------------------------------------------------------------------------------
def test_road_table():
    from acmpc_amd.dynamic_model import road_table
    rng = np.random.default_rng(3002)
    theta, beta = rng.uniform(-0.3, 0.3, 40), rng.uniform(-0.4, 0.4, 40)
    theta[0] = beta[0] = 0.0
    for g in (9.81, 3.71):
        rows = road_table(theta, beta, g=g)
        assert rows.dtype == T and rows.shape == (40, 3)
        assert np.array_equal(rows[:, 0], (-g * np.sin(theta)).astype(T))
        assert np.array_equal(rows[:, 1], (g * np.cos(theta) * np.sin(beta)).astype(T))
        assert np.array_equal(rows[:, 2], (np.cos(theta) * np.cos(beta)).astype(T))
        assert np.array_equal(rows, drs.road_rows(theta, beta, g))
    assert np.array_equal(road_table(theta, beta)[0], np.array([0.0, 0.0, 1.0], dtype=T))
    assert road_table(theta)[3, 1] == 0.0 and road_table(theta, beta)[3, 0] == road_table(theta)[3, 0]
    # signs: downhill is positive a_x, a road that falls to the left positive a_y
    assert road_table([-0.06], [0.0])[0, 0] > 0 and road_table([0.0], [0.1])[0, 1] > 0
    for bad in ((theta, beta[:-1]), (theta[None], beta[None]), ([NAN], [0.0]), ([0.0], [INF]), ([np.pi / 2], [0.0]), ([0.0], [-2.0])):
        with pytest.raises(ValueError):
            road_table(*bad)
    # patches along the arc length: "6 % downhill from 40 m to 120 m"
    s = np.arange(16) * 10.0
    down = -np.arctan(0.06)
    rows = road_table([(40.0, 120.0, down), (100.0, 130.0, 0.0, 0.1)], arc_length=s)
    inside = (s >= 40.0) & (s < 100.0)
    assert np.array_equal(rows[inside], np.tile(road_table([down], [0.0]), (inside.sum(), 1)))
    assert np.array_equal(rows[(s >= 100.0) & (s <= 130.0)], np.tile(road_table([0.0], [0.1]), (4, 1)))
    assert np.array_equal(rows[(s < 40.0) | (s > 130.0)], np.tile(np.array([0.0, 0.0, 1.0], dtype=T), (6, 1)))
    for bad in ([(0.0, 1.0)], [(0.0, 1.0, 0.1, 0.1, 0.1)], [(0.0, 1000.0, 2.0)]):
        with pytest.raises(ValueError):
            road_table(bad, arc_length=s)
    with pytest.raises(ValueError):
        road_table([(0.0, 1.0, 0.1)], beta[:16], arc_length=s)


# ---- 5: the float64 mirror against the restatement ------------------------------------------------------------------------------
MIRROR_RUNS = [(name, window, discs, surface) for name in tdt.MIRROR_CASES for window in (None, (2, 5)) for discs in (False, True)
               for surface in (False, True)]
MIRROR_STEPS = 12
# the road table's seed: of the seeds 5 .. 10 the one whose runs keep every hinge of the float64 side farthest from its kink
# (1.4e-4; seeds 5 and 10 leave one within 2.3e-5, inside the bound) - chosen on the float64 side alone, as the test below checks
MIRROR_ROAD_SEED = 8


@functools.lru_cache(maxsize=None)
def _mirror(name, window, with_discs, with_surface):
    """tests/test_dynamic_trace.py's _mirror under the seeded road table (and a seeded surface table): the worst differences
    and the nearest kink of the float64 side."""
    from acmpc_amd.dynamic_model import trace
    s = tdt.MIRROR_CASES[name]
    dp, coef = tdt._problem(seed=73, width=tdt.MIRROR_WIDTH)
    kw = dp["kw"]
    discs = ds.make_obstacles(dp, MIRROR_STEPS, 3, 9) if with_discs else None
    road = drs.random_road(MIRROR_STEPS, MIRROR_ROAD_SEED)
    mu = dss.random_table(MIRROR_STEPS, 6) if with_surface else None
    u_prev = (0.01, 0.2)
    f32 = drs.trace_plans(dp, coef, dp["U"], [_vehicle().coefficients()], s, window, u_prev, discs, surface=mu, road=road)
    worst = dict(state=0.0, hinge=0.0, kink=INF, rows=set())
    for m in range(dp["U"].shape[0]):
        f64 = trace(_vehicle(), dp["x0"].astype(np.float64), dp["U"][m].astype(np.float64), dp["table"], kw["dt"],
                    u_min=kw["u_min"], u_max=kw["u_max"], margin=kw["margin"], wheelbase=kw["wheelbase"], nn_window=window,
                    substeps=s.substeps, low_speed_blend=s.low_speed_blend, coupling=s.coupling,
                    load_transfer=s.load_transfer, downforce=s.downforce, u_prev=u_prev, rate_max=s.rate_max, slip_max=s.slip_max,
                    speed_ceiling=s.speed_ceiling, obstacles=None if discs is None else discs[0],
                    radii=None if discs is None else discs[1], surface=mu, road=road)
        row = f32["terms"][m, 0].astype(np.float64)
        # the nearest waypoint is the same at every step: no run and no step is left out
        assert np.array_equal(f64["j"], row[:, ds.J].astype(np.int64)), (name, m)
        hinges = np.concatenate([f64["box"], f64["corridor"][:, None], f64["rate"], f64["slip"][:, None],
                                 f64["ceiling"][:, None], f64["obstacles"]], axis=1)
        worst["state"] = max(worst["state"], float(np.abs(f64["states"] - f32["states"][m, 0]).max()))
        worst["hinge"] = max(worst["hinge"], float(np.abs(hinges - row[:, ds.HINGES]).max()))
        worst["kink"] = min(worst["kink"], float(f64["kink"].min()))
        worst["rows"] |= set(int(q) for q in f64["j"][:-1]) | {0}
        for key, slot in (("e_y", ds.EY), ("e_psi", ds.EPSI), ("dv", ds.DV), ("dk", ds.DK)):
            worst["hinge"] = max(worst["hinge"], float(np.abs(f64[key] - row[:, slot]).max()))
    return worst


@pytest.mark.parametrize("name,window,with_discs,with_surface", MIRROR_RUNS)
def test_the_float64_mirror_against_the_restatement(name, window, with_discs, with_surface):
    worst = _mirror(name, window, with_discs, with_surface)
    assert len(worst["rows"]) > 1                       # the plan used more than one road row
    assert worst["state"] <= STATE_TOL and worst["hinge"] <= HINGE_TOL, (name, worst)


@pytest.mark.parametrize("name,window,with_discs,with_surface", MIRROR_RUNS)
def test_no_hinge_of_the_float64_side_lies_within_the_bound_of_its_kink(name, window, with_discs, with_surface):
    """On the float64 side alone: a hinge nearer its kink than the bound could be zero on one side and not on the other."""
    assert _mirror(name, window, with_discs, with_surface)["kink"] > HINGE_TOL


# ---- 6: the handle, without a device --------------------------------------------------------------------------------------------
def _set(eng, road, P, steps):
    road = None if road is None else np.ascontiguousarray(road, dtype=T)
    return eng._lib.acmpc_set_road(eng._ctx, None if road is None else road.ctypes.data, P, steps)


def test_the_entry_point_is_exported():
    import inspect
    import acmpc_amd
    from acmpc_amd import _capi
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    lib = acmpc_amd.load_library()
    assert "acmpc_set_road" in _capi.SIGNATURES and hasattr(lib, "acmpc_set_road")
    assert hasattr(acmpc_amd.Engine, "set_road")
    assert "road" in inspect.signature(DynamicSamplingSolver.solve).parameters
    assert "road=" in sys.modules[DynamicSamplingSolver.__module__].__doc__


def test_every_refusal_leaves_the_handle_as_it_was_and_the_table_survives_the_other_setters():
    from acmpc_amd import EngineError
    P, steps = 2, 5
    solve, trace = tds._solve_code, tds._trace_code
    good = np.tile(np.array([0.3, -0.2, 0.98], dtype=T), (P, steps, 1))
    # off mode D, in the header's order the first refusal
    for mode in (0, 1):
        other, _ = tds._engine(mode=mode)
        assert _set(other, good, P, steps) == ESTATE and _set(other, None, 0, 0) == ESTATE
        assert b"acmpc_set_road" in other._lib.acmpc_last_error(other._ctx)
        with pytest.raises(EngineError) as e:
            other.set_road(good)
        assert e.value.code == ESTATE
        other.close()
    eng, dp = tds._engine(P=P, steps=steps)
    eng.set_dynamics(_vehicle())
    # nothing set: a solve of any shape passes the table's check (and ends at the missing device, or runs)
    assert solve(eng, dp, 1, 4) != ESTATE
    assert _set(eng, good, P, steps) == 0

    def kept():
        """The handle still holds the (P, steps) table: that shape passes, another is refused with the setter's name."""
        assert solve(eng, dp, P, steps) != ESTATE and trace(eng, dp, P, steps) != ESTATE
        assert solve(eng, dp, 1, 3) == ESTATE and b"acmpc_set_road" in eng._lib.acmpc_last_error(eng._ctx)
        assert trace(eng, dp, P, steps - 1) == ESTATE and solve(eng, dp, P - 1, steps) == ESTATE

    kept()
    # P out of range, n out of range
    for bad_P in (0, -1, P + 1):
        assert _set(eng, good, bad_P, steps) == EINVAL
        kept()
    for bad_n in (0, -1, steps + 1):
        assert _set(eng, good, P, bad_n) == EINVAL
        kept()
    # a NaN, an infinity (in each of the three columns), n_z = 0, n_z < 0
    small = np.tile(np.array([0.3, -0.2, 0.98], dtype=T), (1, 3, 1))
    for column in range(3):
        for bad in (NAN, INF, -INF):
            r = small.copy()
            r[0, 2, column] = bad
            assert _set(eng, r, 1, 3) == EINVAL, (column, bad)
            assert b"finite" in eng._lib.acmpc_last_error(eng._ctx)
            kept()
    for bad in (0.0, -0.0, -0.5):
        r = small.copy()
        r[0, 1, 2] = bad
        assert _set(eng, r, 1, 3) == EINVAL, bad
        assert b"n_z" in eng._lib.acmpc_last_error(eng._ctx)
        kept()
    r = small.copy()
    r[0, 0, :2] = (-3.0, 0.0)                           # the two accelerations may have any sign, or be zero
    assert _set(eng, r, 1, 3) == 0 and solve(eng, dp, 1, 3) != ESTATE
    assert _set(eng, good, P, steps) == 0
    with pytest.raises(EngineError) as e:
        eng.set_road(np.zeros((P, steps, 3), dtype=T))
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        eng.set_road(np.ones((P, steps, 2), dtype=T))
    kept()
    # the Engine's shorter form: [n, 3] is one problem's
    eng.set_road(good[0])
    assert solve(eng, dp, 1, steps) != ESTATE and solve(eng, dp, P, steps) == ESTATE
    # None, or NULL, clears it
    for clear in (lambda: eng.set_road(None), lambda: _set(eng, None, 0, 0)):
        eng.set_road(good)
        assert solve(eng, dp, 1, 3) == ESTATE
        assert clear() in (0, None)
        assert solve(eng, dp, 1, 3) != ESTATE
    # it survives the other setters, the surface table's and the actuator's among them, and they survive it
    eng.set_road(good)
    eng.set_dynamics_integration(3, (3.0, 5.0))
    eng.set_dynamics_terms((0.3, 0.02), (1.5, 6.0), 40.0, 0.08)
    eng.set_dynamics_objective(3.0, (1.05, 0.0))
    eng.set_dynamics_coupling((0.9, 1.1))
    eng.set_dynamics_load_transfer(0.35)
    eng.set_dynamics_downforce(tds.AERO)
    eng.set_dynamics_downforce(None)
    eng.set_dynamics_clearance(40.0, 1.0)
    eng.set_obstacles(np.zeros((P, steps, 2, 2), dtype=T), np.ones((P, 2), dtype=T))
    eng.set_obstacles(None)
    eng.set_previous_control(np.zeros((P, 2), dtype=T))
    eng.set_previous_control(None)
    eng.set_surface(np.full((P, steps, 2), 0.7, dtype=T))
    eng.set_surface(None)
    eng.set_dynamics_actuator((0.1, 0.05))
    eng.set_actuator_state(np.zeros((P, 2), dtype=T))
    eng.set_actuator_state(None)
    eng.set_dynamics_actuator(None)
    eng.set_dynamics_ensemble([_vehicle(), _vehicle().with_grip(0.6)])
    eng.set_dynamics(_vehicle())
    kept()
    eng.set_surface(np.full((1, 3, 2), 0.7, dtype=T))   # the two tables are checked each by its own name
    assert solve(eng, dp, P, steps) == ESTATE and b"acmpc_set_surface" in eng._lib.acmpc_last_error(eng._ctx)
    eng.set_surface(None)
    kept()
    lib = eng._lib
    eng.close()
    assert lib.acmpc_set_road(None, None, 0, 0) == EINVAL


if __name__ == "__main__":
    worst = dict(state=0.0, hinge=0.0, kink=INF)
    for run in MIRROR_RUNS:
        w = _mirror(*run)
        print("mirror, %-13s window %-7s discs %-5s surface %-5s state %.3e hinge %.3e nearest kink %.3e rows %d"
              % (run + (w["state"], w["hinge"], w["kink"], len(w["rows"]))))
        worst = dict(state=max(worst["state"], w["state"]), hinge=max(worst["hinge"], w["hinge"]), kink=min(worst["kink"], w["kink"]))
    print("worst over %d runs: state %.3e, hinge %.3e; nearest kink of the float64 side %.3e" % (len(MIRROR_RUNS), worst["state"],
                                                                                                worst["hinge"], worst["kink"]))
    flat, down, up, a_x, slack = _coast()
    print("coasting %.0f s from %.0f m/s: flat %.4f, 6 %% downhill %.4f (+%.4f), uphill %.4f (-%.4f); a_x t = %.4f, slack %.4f"
          % (COAST_T, COAST_V0, flat, down, down - flat, up, flat - up, a_x * COAST_T, slack))
    for label, vehicle in (("reference", _vehicle()), ("front grip x 0.8", _vehicle().with_axle_grip(*UNDERSTEER))):
        road = (0.0, vehicle.g * np.sin(BANK), np.cos(BANK))
        print("steady steering, %s, left circle R = %.0f m at %.0f m/s (L / R = %.6f): flat %.6f rad, banked %.2f rad %.6f rad"
              % (label, BANK_R, BANK_V, (vehicle.lf + vehicle.lr) / BANK_R, _steady_steering(vehicle, None)[0], BANK,
                 _steady_steering(vehicle, road)[0]))
