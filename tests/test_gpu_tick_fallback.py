"""The ticks whose speed profile the two sweeps hand back to the splitting (csrc/acmpc_admm.h: exact_profile -> solve in
prologue_kernel), on the device against the host solver object that mirrors it.

Every test drives one handle through a short sequence of ticks and a host `SpeedProfileSolver` through the same sequence,
fed the tick's own table rows (curvature -> ceiling, spacing): the inputs are then the same bits, the two sides run one
statement of the algorithm, and the comparisons are exact - profile, verdict, iteration count, and through the count of the
tick AFTER a rejected one, the iterate each side kept.  tests/test_speed_profile_fallback.py holds the host side of the same
problems to the reference's rows."""
import copy

import numpy as np
import pytest

from test_gpu_tick import _engine, _tick
from test_speed_profile_fallback import (A_MAX, A_MIN, CAP, EMPTY_BOX, SIGN, V_MIN, args_of, rejected_problem, warm_starts)
from test_support import RACING, PlaceholderVehicle

pytestmark = pytest.mark.gpu

CONS = dict(RACING["monza"]["speed_profile_constraints"], v_max=28.0)   # v_min 8, a_min -1.3, a_max 1.0, end velocity 14


def lane_change(H, spacing=2.45):
    """H points of a lane change (curvature-limited ceilings in the middle), about `spacing` apart."""
    y = spacing * np.arange(H)
    x = 5.0 / (1.0 + np.exp(-0.1 * (y - 0.5 * y[-1])))
    return np.stack([x, y, np.linspace(10, 6, H)], axis=1)


def straight(H, spacing=2.45):
    return np.stack([np.zeros(H), spacing * np.arange(H), np.linspace(10, 6, H)], axis=1)


class HostMirror:
    """The host statement of the prologue's speed-profile step: one solver object per ceiling kind, as the device keeps one
    iterate per kind; the method (the tick's qp_method) may change from tick to tick on the same iterate."""

    def __init__(self, n, max_iter=CAP, check_every=10):
        from acmpc_amd.speed_profile import LocalisedSpeedProfileSolver, SpeedProfileSolver
        self.cons = {}
        config = {"control_horizon": n, "max_iterations": max_iter, "constraints": self.cons, "check_every": check_every}
        self.solvers = {False: SpeedProfileSolver(config), True: LocalisedSpeedProfileSolver(config)}

    def tick(self, table, cons, localised=False, qp_method=0):
        from acmpc_amd.reference_path import ReferencePath
        self.cons.clear()
        self.cons.update(cons)
        solver = self.solvers[localised]
        solver._method = "exact" if qp_method == 0 else "admm"
        return solver.solve(ReferencePath.from_table(table), cons["end_velocity"])


def run(eng, mirror, H, coords, cons, localised=False, qp_method=0):
    """One tick on the device and on the mirror; asserts that they agree exactly and returns (info, table, host result)."""
    out = eng.control_tick(_tick(H, cons, localised=localised, qp_method=qp_method), coords, None)
    info, table = out["info"], out["table"]
    host = mirror.tick(table, cons, localised, qp_method)
    assert (info[4] == 0) == (host.info.status == "solved"), (info[4], host.info.status)
    assert int(info[5]) == host.info.iter
    np.testing.assert_array_equal(table[6], host.x if host.info.status == "solved" else np.zeros(H - 1))
    return info, table, host


# ---- 1. an empty box ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qp_method", [0, 1])
@pytest.mark.parametrize("kind", ["end-1e-5", "end-0.5", "end-6", "localised"])
@pytest.mark.parametrize("H", [3, 50, 65, 66, 129])
def test_a_tick_with_an_empty_box_is_not_solved_and_keeps_the_iterate(H, kind, qp_method):
    """feasible, rejected, feasible.  The rejected tick - the end velocity below v_min by 1e-5, 0.5 or 6 m/s, or the localised
    ceiling v_max below v_min - runs the splitting to the default cap of 4000 and reports status 1 and zero velocities (it
    reported "solved" and a profile metres per second outside its bounds); the tick after it equals the host's, which under
    qp_method 1 is the warm re-solve of the first tick's problem: the first stopping test, 10 iterations."""
    n = H - 1
    coords = lane_change(H)
    localised = kind == "localised"
    bad = dict(CONS, v_max=V_MIN - 0.5) if localised else dict(CONS, end_velocity=V_MIN - float(kind[4:]))
    eng, _, _ = _engine(n)
    mirror = HostMirror(n)
    first, _, _ = run(eng, mirror, H, coords, CONS, localised, qp_method)
    assert first[4] == 0 and (first[5] == 0 if qp_method == 0 else first[5] >= 10)
    info, table, host = run(eng, mirror, H, coords, bad, localised, qp_method)
    assert info[4] != 0 and info[5] == CAP and np.all(table[6] == 0.0)
    assert host.info.status != "solved"
    third, table3, _ = run(eng, mirror, H, coords, CONS, localised, qp_method)
    assert third[4] == 0 and third[5] == (0 if qp_method == 0 else 10)
    eng.close()


# ---- 2. a rate bound of the wrong sign -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("before,change", [(0, dict(a_max=-0.05)), (1, dict(a_max=-0.05)), (0, dict(a_min=0.02))])
def test_a_sign_rejected_tick_is_solved_by_the_splitting_from_the_kept_iterate(before, change):
    """A straight, waypoints 2.45 m apart, ceiling 30, end velocity 14.  The a_max = -0.05 tick after an exact tick (the
    splitting starts from the exact profile and no multipliers) and after a qp_method 1 tick (from that tick's iterate), the
    a_min = +0.02 tick after an exact tick: status, iteration count and profile equal the host object's; and the feasible
    qp_method 1 tick behind it starts from what the fallback left - the same count as on the host, which differs from a cold
    solve's."""
    H, n = 50, 49
    coords = straight(H)
    eng, _, _ = _engine(n)
    mirror = HostMirror(n)
    first, _, _ = run(eng, mirror, H, coords, CONS, qp_method=before)
    assert first[4] == 0
    info, table, host = run(eng, mirror, H, coords, dict(CONS, **change), qp_method=0)
    assert info[4] == 0 and 10 < info[5] < CAP
    kept = tuple(a.copy() for a in mirror.solvers[False]._warm)
    np.testing.assert_array_equal(kept[0], table[6])
    after, _, _ = run(eng, mirror, H, coords, CONS, qp_method=1)
    from acmpc_amd import _capi
    ceiling = _capi.velocity_ceiling(table[3], CONS["ay_max"], CONS["ki_min"], CONS["v_min"], CONS["v_max"], False,
                                     CONS["end_velocity"])
    cold = _capi.speed_profile_qp(ceiling, table[4], A_MIN, A_MAX, V_MIN)
    warm = _capi.speed_profile_qp(ceiling, table[4], A_MIN, A_MAX, V_MIN, warm=kept)
    assert after[4] == 0 and int(after[5]) == warm[3] and warm[3] != cold[3]
    eng.close()


# ---- 3. not a problem at all -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["coincident", "nan", "inf"])
def test_coincident_waypoints_and_a_non_finite_end_velocity(what):
    """Two equal rows of `coords` (a spacing of zero) or an end velocity that is no number: not solved, zero velocities, the
    host's status and count; the next feasible tick is exact again."""
    H, n = 50, 49
    coords = lane_change(H)
    cons = dict(CONS)
    broken = coords.copy()
    if what == "coincident":
        broken[20] = broken[19]
    else:
        cons["end_velocity"] = float(what)
    eng, _, _ = _engine(n)
    mirror = HostMirror(n)
    first, _, _ = run(eng, mirror, H, coords, CONS)
    assert first[4] == 0 and first[5] == 0
    info, table, host = run(eng, mirror, H, broken, cons)
    assert info[4] != 0 and info[5] == CAP and np.all(table[6] == 0.0)
    if what == "coincident":
        assert table[4][19] == 0.0
    again, _, _ = run(eng, mirror, H, coords, CONS)
    assert again[4] == 0 and again[5] == 0
    eng.close()


# ---- 4. the splitting alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 49, 64, 65, 128])
def test_device_splitting_is_bit_identical_on_rejected_problems(n):
    """`speed_profile_qp_device` against the host solver on the empty-box and the sign-rejected problems of the host tests,
    cold and from a kept iterate: every bit of x and y, the status and the count (one slot per lane up to 64 points, two
    beyond)."""
    from acmpc_amd import _capi
    eng, _, _ = _engine(max(n, 8))
    for reason in EMPTY_BOX + SIGN:
        problem, neighbour = rejected_problem(reason, n)
        for name, warm in warm_starts(neighbour).items():
            if name == "exact":
                continue
            host = _capi.speed_profile_qp(*args_of(problem), warm=warm)
            dev = eng.speed_profile_qp_device(*args_of(problem), warm=warm)
            assert host[2:] == dev[2:], (reason, name)
            if reason in EMPTY_BOX:
                assert dev[2] != "solved" and dev[3] == CAP
            np.testing.assert_array_equal(dev[0], host[0], err_msg=reason + " " + name)
            np.testing.assert_array_equal(dev[1], host[1], err_msg=reason + " " + name)
    eng.close()


# ---- 5. the controller -----------------------------------------------------------------------------------------------------------------
def test_the_controller_keeps_its_speed_profile_over_unsolved_ticks():
    """The drop-in controller with the prologue on the device and with the host statements of the same steps, 12 ticks along
    monza; on ticks 4 - 6 `speed_profile_constraints["v_min"]` (the live dict) is above the end velocity.  Both keep tick 3's
    `speed_profile` over those ticks, and agree to the tolerances of the feasible-lap comparison on all others."""
    from acmpc_amd import workloads
    from acmpc_amd.mpc import build_mpc
    cfgs = []
    for device in (True, False):
        cfg = copy.deepcopy(workloads.RACING_CONTROL["monza"])
        cfg["speed_profile_constraints"]["v_max"] = float(cfg["unlocalised_max_speed"])
        cfg.update(device_prologue=device, n_candidates=4096, lq_candidate=False)
        cfgs.append(cfg)
    a, b = (build_mpc(c, PlaceholderVehicle()) for c in cfgs)
    circuit = workloads.synthetic_track("monza")
    v_min = cfgs[0]["speed_profile_constraints"]["v_min"]
    end_velocity = cfgs[0]["speed_profile_constraints"]["end_velocity"]
    kept = None
    for i in range(12):
        rejected = 4 <= i <= 6
        for mpc in (a, b):
            mpc.speed_profile_constraints["v_min"] = end_velocity + 6.0 if rejected else v_min
        centre = workloads.local_centreline(circuit, (i * 4) % len(circuit["centre"]), lateral_offset=0.2)
        path = workloads.reference_path_from_centreline(centre, cfgs[0]["horizon"])
        a.get_control(path, offset=0.2)
        b.get_control(path, offset=0.2)
        if rejected:
            np.testing.assert_array_equal(a.speed_profile, kept[0])
            np.testing.assert_array_equal(b.speed_profile, kept[1])
            continue
        kept = (a.speed_profile.copy(), b.speed_profile.copy())
        assert a.infeasibility_counter == 0 and b.infeasibility_counter == 0
        np.testing.assert_allclose(a.reference_path.table, b.reference_path.table, rtol=0, atol=1e-9)
        np.testing.assert_allclose(a.projected_control, b.projected_control, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(a.cum_time, b.cum_time, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(a.current_prediction, b.current_prediction, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(a.speed_profile, b.speed_profile, rtol=0, atol=1e-9)
        assert (a.speed_profile > 0.0).all()
