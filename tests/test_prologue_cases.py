"""The case list of the prologue tests (tests/prologue_cases.py) held to its own conditions - so that the GPU test cannot pass
by missing the edge it is there for - and the library's HOST statements of the prologue's steps (`acmpc_waypoint_table`,
`acmpc_velocity_ceiling`, `acmpc_speed_profile_exact`, `acmpc_set_paths`) over the same list against the same reference with
the same checks the kernel gets (tests/test_gpu_prologue_tables.py).  No GPU."""
import math

import numpy as np
import pytest

import acmpc_oracle as orc
import prologue_cases as pc


def test_the_reference_headings_are_wider_than_float64():
    assert np.finfo(np.longdouble).nmant >= 63, "the heading reference needs a long double wider than float64"


def test_the_case_list_covers_the_horizons_and_settings():
    assert {c.H for c in pc.CASES} == set(pc.HORIZONS) == {3, 4, 50, 64, 65, 66, 128, 129}
    assert len({c.name for c in pc.CASES}) == len(pc.CASES)
    for H in pc.HORIZONS:
        cases = pc.cases_at(H)
        assert {c.family for c in cases} == {"arc", "rotated", "wiggly"}
        open_road = [c for c in cases if not c.localised]
        assert {c.localised for c in cases} == {0, 1} and {c.has_end_velocity for c in open_road} == {0, 1}
        assert min(c.offset for c in cases) < 0 < max(c.offset for c in cases)
        for c in cases:
            assert c.coords.shape == (H, 3) and c.coords.dtype == np.float64
            np.testing.assert_array_equal(c.coords[:, 2], np.linspace(10, 6, H))
            gaps = np.hypot(*np.diff(c.coords[:, :2], axis=0).T)
            assert 2.3 < gaps.min() and gaps.max() < (2.5 if c.family != "wiggly" else 12.0), c.name


def test_every_case_has_a_feasible_profile():
    for case in pc.CASES:
        _, _, profile = pc.reference_table(case)
        assert profile is not None, case.name


@pytest.mark.parametrize("H", pc.HORIZONS)
def test_the_headings_cross_pi_and_rate_rows_are_active(H):
    """At every H >= 33 some case's neighbouring headings jump by more than pi (the left arcs); at every H >= 4 - here at
    H = 3 as well - a rotated case's do; and at every H, the shortest included (no waiver needed: the end velocity holds the
    waypoint before it below its ceiling), some case's profile is below its ceiling: a rate row is active."""
    cases = pc.cases_at(H)
    if H >= 33:
        assert any(pc.heading_jump(c) > math.pi for c in cases if c.family == "arc")
        assert all(pc.heading_jump(c) > math.pi for c in cases if c.name.endswith("left"))
    assert all(pc.heading_jump(c) > math.pi for c in cases if c.family == "rotated")
    for c in cases:
        if c.family == "rotated":       # the first pair already: psi[0] next to +-pi, psi[1] on the other side
            psi = pc.long_double_headings(c.coords)[:2].astype(np.float64)
            assert abs(abs(psi[0]) - (math.pi - 0.01)) < 1e-9 and psi[0] * psi[1] < 0 and abs(psi[1]) > 3.0
    held = 0
    for c in cases:
        _, ceiling, profile = pc.reference_table(c)
        held += int((profile < ceiling - 1e-9).any())
    assert held > 0


def test_the_start_state_needs_its_wrap_somewhere():
    """pi/2 - psi[0] leaves [-pi, pi) for the case that starts next to -pi: a start state without the wrap differs."""
    for H in pc.HORIZONS:
        assert any(math.pi / 2.0 - pc.reference_table(c)[0][orc.ROW_PSI, 0] >= math.pi for c in pc.cases_at(H))


def test_numpys_own_headings_against_the_long_double_ones():
    """The reference's float64 headings (`orc.construct_waypoints`: NumPy's arctan2) are within PSI_ULPS_HOST of the long
    double ones on every case - the figure the host bound rests on - and the reference table passes its own checks."""
    worst = 0.0
    for case in pc.CASES:
        table = orc.construct_waypoints(case.coords)
        _, profile = pc.reference_profile(case, table[orc.ROW_KAPPA], table[orc.ROW_DS])
        table[orc.ROW_V] = profile
        worst = max(worst, pc.check_tables(case, "S", table, pc.PSI_ULPS_HOST))
    assert worst <= pc.PSI_ULPS_HOST


def test_the_checks_reject_a_wrong_table():
    """`check_tables` is what both suites rely on: each of these single-entry changes to a right table must fail it."""
    case = [c for c in pc.cases_at(66) if c.name.endswith("arc_r15_left")][0]
    table, _, profile = pc.reference_table(case)
    table[orc.ROW_V] = profile
    pc.check_tables(case, "S", table, pc.PSI_ULPS_HOST)
    n = case.n
    for row, index, change in ((orc.ROW_PSI, n - 1, 1e-14), (orc.ROW_KAPPA, n - 1, 1e-13), (orc.ROW_KAPPA, 0, 1e-13),
                               (orc.ROW_WIDTH, n - 1, 1e-15), (orc.ROW_V, 64, 1e-14), (orc.ROW_DS, 64, 1e-15),
                               (orc.ROW_PSI, 30, 2 * math.pi)):
        wrong = table.copy()
        wrong[row, index] += change
        with pytest.raises(AssertionError):
            pc.check_tables(case, "S", wrong, pc.PSI_ULPS_HOST)


def _host_table(case):
    from acmpc_amd import _capi
    table = _capi.waypoint_table(case.coords)
    ceiling = _capi.velocity_ceiling(table[orc.ROW_KAPPA], pc.CONS["ay_max"], pc.CONS["ki_min"], pc.CONS["v_min"],
                                     pc.CONS["v_max"], bool(case.localised),
                                     pc.CONS["end_velocity"] if case.has_end_velocity else None)
    swept = _capi.speed_profile_exact(ceiling, table[orc.ROW_DS], pc.CONS["a_min"], pc.CONS["a_max"], pc.CONS["v_min"])
    assert swept is not None, case.name
    table[orc.ROW_V] = swept[0]
    return table, ceiling


@pytest.mark.parametrize("H", pc.HORIZONS)
def test_the_host_statements_against_the_reference(H):
    """`acmpc_waypoint_table` -> `acmpc_velocity_ceiling` -> `acmpc_speed_profile_exact` -> `acmpc_set_paths` (modes S and T) on
    every case of this horizon: the checks of the device's tables, with the C library's atan2 in place of the device's."""
    from acmpc_amd import Engine
    engines = {mode: Engine(mode=number, max_problems=1, max_candidates=1, max_steps=H - 1, step_cost=[1, 1, 0], r_term=[1, 1],
                            final_cost=[1, 0, 0], u_min=pc.BOX[0], u_max=pc.BOX[1], margin=pc.LIMITS.margin,
                            wheelbase=pc.LIMITS.length) for mode, (number, _) in pc.MODES.items() if mode != "Tw"}
    for case in pc.cases_at(H):
        table, ceiling = _host_table(case)
        pc.assert_bits(ceiling, pc.velocity_ceiling(table[orc.ROW_KAPPA], pc.CONS, case.localised, case.has_end_velocity),
                       case.name + " ceiling")
        for mode, eng in engines.items():
            eng.set_paths(table)
            pc.check_tables(case, mode, table, pc.PSI_ULPS_HOST, coef=eng.coefficients(0), what="host")
    for eng in engines.values():
        eng.close()
