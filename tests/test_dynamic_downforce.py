"""Mode D's aerodynamic downforce on the CPU ("Mode D, downforce"): the issue's table of hand figures
re-derived from the float64 mirror (DynamicBicycleParams.predict_next_state(..., downforce=)), the four identities of the float32
restatement (tests/dynamic_spec.py) bit for bit, the restatement against the mirror, the refusals of the C ABI on a handle
without a device, a fast corner and full braking on the mirror, and what the setting gives the grip identification on a log
driven with downforce.

`python tests/test_dynamic_downforce.py` prints the measured maxima of the restatement against the mirror, the braking figures
and what the identification picks without the setting."""
import dataclasses
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
import dynamic_spec as ds  # noqa: E402
import grip_spec as gs  # noqa: E402
from dynamic_spec import Settings  # noqa: E402
import test_dynamic_cost_float64 as t64  # noqa: E402
import test_dynamic_coupling as tdc  # noqa: E402
import test_gpu_dynamic_load_transfer as tgl  # noqa: E402

T = np.float32
EINVAL, ESTATE = -1, -5
INF, NAN = float("inf"), float("nan")
LOAD = (0.35, 0.9)
RATIOS = tdc.RATIOS
GRID = tdc.GRID
# C_L A = 3.0 m^2, air 1.225 kg/m^3, 40 % on the front axle, in kN per (m/s)^2: (7.35e-4, 1.1025e-3)
CL_A, BALANCE = 3.0, 0.4


def _params():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams


def _aero(v_sat=None):
    from acmpc_amd.dynamic_model import downforce_coefficients
    pair = downforce_coefficients(CL_A, BALANCE)
    return pair if v_sat is None else pair + (float(v_sat),)


def _bits(a):
    return np.asarray(a, dtype=T).view(np.uint32)


def _same_where_finite(got, want):
    """test_gpu_dynamic_load_transfer._same_where_finite: the same bits wherever the parent's value is finite, non-finite where
    the parent's is."""
    tgl._same_where_finite(np.asarray(got, dtype=T), np.asarray(want, dtype=T))
    return True


def _constants(vehicle, ratio, load, aero):
    return ds.constants(vehicle, Settings(coupling=ratio, load_transfer=load, downforce=aero), 0.05)


# ---- 1. the issue's table -----------------------------------------------------------------------------------------------------
# The tolerance is the figures' printed digits: half a unit of the last digit printed (0.005 kN, 0.0005 of a factor, 0.005 m/s^2).
TABLE = [  # vx, (d_f, d_r) kN, (factor f, r), (Pf + Pr) / mass
    (0.0, (0.0, 0.0), (1.0, 1.0), 11.40),
    (30.0, (0.66, 0.99), (1.098, 1.102), 12.54),
    (55.56, (2.27, 3.40), (1.314, 1.273), 14.74),
    (70.0, (3.60, 5.40), (1.471, 1.332), 15.95),
]


def test_the_coefficients_are_the_issues():
    k_f, k_r = _aero()
    assert k_f == pytest.approx(7.35e-4, rel=1e-12) and k_r == pytest.approx(1.1025e-3, rel=1e-12)
    from acmpc_amd.dynamic_model import downforce_coefficients
    assert downforce_coefficients(3.0, 0.4, force_unit=1.0) == pytest.approx((735e-3, 1102.5e-3), rel=1e-12)
    for bad in (dict(cl_a=-1.0, balance_front=0.4), dict(cl_a=NAN, balance_front=0.4), dict(cl_a=3.0, balance_front=1.5),
                dict(cl_a=3.0, balance_front=0.4, air_density=0.0), dict(cl_a=3.0, balance_front=0.4, force_unit=-1.0)):
        with pytest.raises(ValueError):
            downforce_coefficients(**bad)


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "vx %g" % r[0])
def test_the_table_from_the_mirror(row):
    vx, down, factor, total = row
    p = _params().reference()
    d_f, d_r = p.downforce_at(vx, _aero())
    assert d_f == pytest.approx(down[0], abs=0.005) and d_r == pytest.approx(down[1], abs=0.005)
    _, F_zf, F_zr = p.loaded_axles(0.0, 0.0, None, None, _aero(), vx)
    assert F_zf == p.F_zf + d_f and F_zr == p.F_zr + d_r
    Pf, Pr = p.peak("f", F_zf), p.peak("r", F_zr)
    assert Pf / p.peak_front == pytest.approx(factor[0], abs=0.0005) and Pr / p.peak_rear == pytest.approx(factor[1], abs=0.0005)
    assert (Pf + Pr) / p.mass == pytest.approx(total, abs=0.005)
    # and the step takes those peaks: a slip angle at which both axles give their peak's sine, pedal 0
    state = np.array([0.0, 0.0, 0.0, vx, 0.0, 0.3])
    f_on = p.predict_next_state(state, (0.05, 0.0), downforce=_aero())[2]
    f_off = p.predict_next_state(state, (0.05, 0.0))[2]
    if vx > 0:
        assert f_on[0] / f_off[0] == pytest.approx(Pf / p.peak_front, rel=1e-12) and f_on[1] / f_off[1] == pytest.approx(Pr / p.peak_rear, rel=1e-12)


def test_where_the_factors_reach_zero():
    """The issue's figures: the rear factor reaches zero 17.8 kN above static, the front 31.5 kN; the rear vertex is 5.95 kN
    above static."""
    p = _params().reference()
    c = ds.constants64(p.coefficients(), LOAD)
    for axle, zero in (("f", 31.5), ("r", 17.8)):
        a1, a2 = c["a1_" + axle], c["a2_" + axle]
        roots = np.roots([a2, a1, 1.0])
        assert roots[roots > 0].min() == pytest.approx(zero, abs=0.05)
    assert -c["a1_r"] / (2 * c["a2_r"]) == pytest.approx(5.95, abs=0.005)
    # the quadratic is the exact ratio of peaks over the whole range the downforce reaches
    x = np.linspace(0.0, 17.0, 2001)
    phi = 1 + x * (c["a1_r"] + c["a2_r"] * x)
    exact = np.array([p.peak("r", p.F_zr + v) for v in x]) / p.peak_rear
    assert np.max(np.abs(phi - exact)) <= 1e-12


# ---- 2. the four identities of the restatement, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("load", [LOAD, None])
@pytest.mark.parametrize("ratio", RATIOS + [None, (INF, 0.5)])
def test_zero_coefficients_are_the_parent_step(ratio, load):
    vehicle = _params().reference().with_grip(0.8).coefficients()
    st, delta, pedal = tdc._random_rows(4000, 21)
    want = tdc._step(_constants(vehicle, ratio, load, None), st, delta, pedal)    # the loaded, the coupled or the plain step
    zero = (0.0, 0.0, 30.0)
    got = tdc._step(_constants(vehicle, ratio, load, zero), st, delta, pedal)
    assert _same_where_finite(got, want)
    assert np.isnan(want).any() and np.isfinite(want).all(axis=1).sum() > 3000     # the NaN / inf rows are in there
    moved = tdc._step(_constants(vehicle, ratio, load, _aero()), st, delta, pedal)
    assert not np.array_equal(_bits(moved), _bits(want))                           # and a coefficient does something


@pytest.mark.parametrize("load", [LOAD, None])
@pytest.mark.parametrize("ratio", RATIOS + [None])
def test_standstill_is_the_parent_within_one_substep(ratio, load):
    vehicle = _params().reference().coefficients()
    st, delta, pedal = tdc._random_rows(4000, 22)
    still = st[:, 3] == 0
    assert still.sum() >= 80
    parent = tdc._step(_constants(vehicle, ratio, load, (0.0, 0.0)), st, delta, pedal)
    got = tdc._step(_constants(vehicle, ratio, load, _aero()), st, delta, pedal)
    assert _same_where_finite(got[still], parent[still])
    assert not np.array_equal(_bits(got[~still]), _bits(parent[~still]))


@pytest.mark.parametrize("load", [LOAD, None])
def test_above_v_sat_the_peaks_are_those_at_v_sat(load):
    vehicle = _params().reference().coefficients()
    v_sat = 26.0
    k = _constants(vehicle, (1.0, 1.0), load, _aero(v_sat)).k
    vx = np.array([5.0, 25.999, 26.0, 26.001, 40.0, 1e30, INF, NAN], dtype=T)
    F_fx, F_rx = np.full(vx.size, -3.0, dtype=T), np.full(vx.size, -1.0, dtype=T)
    Pf, Pr, w, d_f, d_r = ds.aero_peaks(vx, F_fx, F_rx, T(1.0), T(1.0), k)
    at = ds.aero_peaks(np.full(vx.size, v_sat, dtype=T), F_fx, F_rx, T(1.0), T(1.0), k)
    above = np.array([False, False, True, True, True, True, True, True])     # (a NaN vx takes v_sat: minNum)
    for a, b in zip((Pf, Pr, w, d_f, d_r), at):
        assert np.array_equal(_bits(a[above]), _bits(b[above]))
    assert np.all(Pf[:2] < Pf[2]) and np.all(Pr[:2] < Pr[2]) and np.all(np.isfinite(Pf)) and np.all(Pf > 0) and np.all(Pr > 0)
    # a rollout that starts above v_sat and one that starts below it: both sides in one trajectory set
    x0 = np.array([[0, 0, 0, 32.0, 0, 0], [0, 0, 0, 20.0, 0, 0]], dtype=T)
    U = np.stack([np.full((2, 12), 0.02), np.stack([np.full(12, -0.8), np.full(12, 0.9)])], axis=2).astype(T)
    capped = gs.rollout_states(x0, U, vehicle, 0.05, settings=Settings(coupling=(1.0, 1.0), load_transfer=load,
                               downforce=_aero(v_sat)))
    free = gs.rollout_states(x0, U, vehicle, 0.05, settings=Settings(coupling=(1.0, 1.0), load_transfer=load, downforce=_aero()))
    assert capped[0, 0, 3] > v_sat > capped[0, -1, 3] and capped[1, 0, 3] < v_sat
    assert not np.array_equal(_bits(capped[0]), _bits(free[0]))
    below = np.all(free[1, :-1, 3] <= v_sat)
    assert below and np.array_equal(_bits(capped[1]), _bits(free[1]))            # never above v_sat: the ceiling does nothing


@pytest.mark.parametrize("ratio", RATIOS + [None])
def test_without_the_load_transfer_the_w_lines_change_nothing(ratio):
    """c_h = w_max = 0: w = +-0 and x_a = d_a exactly (d_a >= +0), so a step that skips the w lines gives the same bits."""
    vehicle = _params().reference().coefficients()
    st, delta, pedal = tdc._random_rows(4000, 23)
    k = _constants(vehicle, ratio, None, _aero()).k
    assert k["c_h"] == 0 and k["w_max"] == 0 and k["a1_f"] > 0
    rho_f, rho_r = ds.ratios(ratio)
    vx = st[:, 3]
    with np.errstate(all="ignore"):
        F_fx = (pedal * T(9.0)).astype(T)
        Pf, Pr, w, d_f, d_r = ds.aero_peaks(vx, F_fx, F_fx, rho_f, rho_r, k)
        skip_f = k["Pf"] * (T(1.0) + d_f * (k["a1_f"] + k["a2_f"] * d_f))
        skip_r = k["Pr"] * (T(1.0) + d_r * (k["a1_r"] + k["a2_r"] * d_r))
    ok = ~np.isnan(pedal)        # (a NaN demand makes w NaN: the candidate is NaN through the other lines as before)
    assert np.all(w[ok] == 0)                   # (+0 or -0, whatever the clip leaves: d_a - w and d_a + w are d_a either way)
    assert np.array_equal(_bits(Pf[ok]), _bits(skip_f[ok])) and np.array_equal(_bits(Pr[ok]), _bits(skip_r[ok]))


def test_setting_none_falls_through_and_the_order_is_kept():
    vehicle = _params().reference().coefficients()
    k = _constants(vehicle, (1.0, 1.0), LOAD, None).k
    assert "c_h" in k and "k_f" not in k
    k = _constants(vehicle, None, None, _aero()).k
    assert k["k_f"] == T(7.35e-4) and k["k_r"] == T(1.1025e-3) and k["v_sat"] == T(100.0) and k["c_h"] == 0


# ---- 3. the float32 restatement against the float64 mirror --------------------------------------------------------------------
# The states and controls of tests/test_dynamic_cost_float64.py's cases (the first MIRROR_CANDIDATES candidates of each), under
# (1, 1) coupling, LOAD and the downforce, once with v_sat = 26 m/s - the monza cases start at 28 m/s and the silverstone ones at
# 32 m/s and brake through it, the standstill ones stay below - and once with v_sat = 100 m/s.  The figure is the worst
# |s32 - s64| / max(|s64|, 1) over the six states, every step and candidate.  Measured here (NumPy 1.26, x86-64; this file's
# __main__): see MIRROR_MEASURED; the test allows 4 x that (the project's standing margin: other NumPy builds' arctan / sin / cos
# differ in the last place of the float64 side).  The measurement is of the mirror against the restatement; neither is the code
# under test.  As in test_dynamic_cost_float64.py the standstill cases have a figure of their own: with vx near 0 the slip
# quotients divide by 1e-3 and the model itself amplifies the last place of its inputs.
MIRROR_CANDIDATES = 6
MIRROR_V_SATS = (26.0, 100.0)
MIRROR_MEASURED = 8.613e-5              # silverstone yaw n 128, v_sat 26 (r, after 6.4 s of open-loop noise); median case 1e-5
MIRROR_MEASURED_STANDSTILL = 5.434e-1   # both n = 20 standstill cases (r at vx < 1.1 m/s; 2.0e-7 at n = 2): no better than the model
MIRROR_FACTOR = 4.0


def _mirror_deviation(case, v_sat):
    track, kind, n, N, window, grips, reduce, weights = case
    dp = ds.make_dynamic_problem(orc, track, n + 1, N, n, **t64.KINDS[kind])
    dt = float(dp["kw"]["dt"])
    x0 = np.asarray(dp["x0"], dtype=T)
    U = np.asarray(dp["U"], dtype=T)[:MIRROR_CANDIDATES]
    worst, speeds = 0.0, []
    for g in grips:
        params = _params().reference() if g == 1.0 else _params().reference().with_grip(g)
        got = gs.rollout_states(np.repeat(x0[None], U.shape[0], axis=0), U, params.coefficients(), dt,
                                settings=Settings(coupling=(1.0, 1.0), load_transfer=LOAD, downforce=_aero(v_sat)))
        for c in range(U.shape[0]):
            want = params.rollout(x0.astype(np.float64), U[c].astype(np.float64), dt, coupling=(1.0, 1.0), load_transfer=LOAD,
                                  downforce=_aero(v_sat))
            rel = np.abs(got[c].astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
            worst = max(worst, float(rel.max()))
            speeds.append(want[:, 3])
    speeds = np.concatenate(speeds)
    return worst, float(speeds.min()), float(speeds.max())


def _mirror_figures():
    moving, still = {}, {}
    for case in t64.CASES:
        for v_sat in MIRROR_V_SATS:
            (still if case[1] == "standstill" else moving)[(t64._label(case), v_sat)] = _mirror_deviation(case, v_sat)
    return moving, still


def test_the_restatement_against_the_float64_mirror():
    moving, still = _mirror_figures()
    for name, figures in (("moving", moving), ("standstill", still)):
        for key, (worst, lo, hi) in figures.items():
            print("%s %s v_sat %g: worst relative deviation %.3e, vx %.1f .. %.1f" % ((name,) + key + (worst, lo, hi)))
    # speeds on both sides of the lower v_sat, in one case at least on both sides within it
    lo = min(v[1] for (_, v_sat), v in moving.items() if v_sat == 26.0)
    hi = max(v[2] for (_, v_sat), v in moving.items() if v_sat == 26.0)
    assert lo < 26.0 < hi
    assert MIRROR_MEASURED > 0 and MIRROR_MEASURED_STANDSTILL > 0
    assert max(v[0] for v in moving.values()) <= MIRROR_FACTOR * MIRROR_MEASURED
    assert max(v[0] for v in still.values()) <= MIRROR_FACTOR * MIRROR_MEASURED_STANDSTILL


# ---- 4. the mirror: a fast corner and full braking ----------------------------------------------------------------------------
def _steady_corner(p, vx, a_lat, downforce):
    """The steady state of a corner with lateral acceleration a_lat at the speed vx, pedal 0: (state, delta) with vy' = r' = 0
    on the mirror, or None when an axle cannot give the side force the corner needs at any slip angle."""
    r = a_lat / vx
    L = p.lf + p.lr
    need_r = p.mass * a_lat * p.lf / L
    d_f, d_r = p.downforce_at(vx, downforce)
    alphas = np.linspace(0.0, 0.5, 20001)
    delta = 0.0
    for _ in range(30):
        need_f = p.mass * a_lat * p.lr / L / np.cos(delta)
        F_f = p._lateral(alphas, p.Bf, p.Cf, p.Df, p.Ef, p.epsf, p.F_zf + d_f)
        F_r = p._lateral(alphas, p.Br, p.Cr, p.Dr, p.Er, p.epsr, p.F_zr + d_r)
        if F_f.max() < need_f or F_r.max() < need_r:
            return None
        a_f = np.interp(need_f, F_f[:F_f.argmax() + 1], alphas[:F_f.argmax() + 1])
        a_r = np.interp(need_r, F_r[:F_r.argmax() + 1], alphas[:F_r.argmax() + 1])
        vy = r * p.lr - (vx + 1e-3) * np.tan(a_r)
        delta = a_f + np.arctan((r * p.lf + vy) / (vx + 1e-3))
    return np.array([0.0, 0.0, 0.0, vx, vy, r]), delta


def test_a_fast_corner_the_static_peaks_cannot_hold_is_held():
    p = _params().reference()
    vx, a_lat = 55.0, 13.5
    assert (p.peak_front + p.peak_rear) / p.mass < a_lat            # 11.40 m/s^2: no steady state without the setting
    assert _steady_corner(p, vx, a_lat, None) is None
    state, delta = _steady_corner(p, vx, a_lat, _aero())
    _, xd, forces = p.predict_next_state(state, (delta, 0.0), downforce=_aero())
    assert abs(xd[4]) < 1e-4 and abs(xd[5]) < 1e-4                  # vy' = r' = 0: the corner is held
    assert (forces[1] + forces[0] * np.cos(delta)) / p.mass == pytest.approx(a_lat, abs=1e-3)
    # the same state and steering without the downforce: the car cannot follow (vy' < 0 means it runs wide)
    _, xd_off, _ = p.predict_next_state(state, (delta, 0.0))
    assert xd_off[4] < -1.0


def _braking_figures():
    p = _params().reference()
    state = np.array([0.0, 0.0, 0.0, 60.0, 0.0, 0.0])
    off = p.predict_next_state(state, (0.0, -1.0), coupling=(1.0, 1.0), load_transfer=LOAD)
    on = p.predict_next_state(state, (0.0, -1.0), coupling=(1.0, 1.0), load_transfer=LOAD, downforce=_aero())
    return off, on


def test_full_braking_from_high_speed_decelerates_harder():
    """Recorded (this file's __main__): full braking from 60 m/s under (1, 1) coupling and LOAD."""
    (_, xd_off, f_off), (_, xd_on, f_on) = _braking_figures()
    print("full braking from 60 m/s: vx' = %.3f m/s^2 without the downforce, %.3f with it" % (xd_off[3], xd_on[3]))
    assert xd_on[3] < xd_off[3] < 0
    assert f_on[2] < f_off[2] < 0             # the front axle is at its cap, and the cap is higher
    p = _params().reference()
    _, F_zf, _ = p.loaded_axles(f_on[2], f_on[3], (1.0, 1.0), LOAD, _aero(), 60.0)
    assert F_zf > p.F_zf + p.downforce_at(60.0, _aero())[0]         # load moved forward on top of the downforce
    # downforce=None is the parent's step, and k = 0 too
    assert np.array_equal(p.predict_next_state(np.array([0, 0, 0, 60.0, 0.3, 0.1]), (0.02, -1.0), coupling=1.0, load_transfer=LOAD,
                                               downforce=(0.0, 0.0))[1],
                          p.predict_next_state(np.array([0, 0, 0, 60.0, 0.3, 0.1]), (0.02, -1.0), coupling=1.0, load_transfer=LOAD)[1])
    for wrong in ((1.0,), (1.0, 2.0, 3.0, 4.0)):
        with pytest.raises(ValueError):
            p.downforce_at(10.0, wrong)


# ---- 5. identification --------------------------------------------------------------------------------------------------------
# A log driven on the mirror with the downforce at tied grip 0.7: sinusoidal steering of amplitude IDENT_AMPLITUDE (period 1 s)
# and a light brake that takes the car from 55 m/s to just above 45 m/s in two seconds.  The amplitude is chosen so that, on the CPU with the
# restated score, the grid WITH the setting has its best at 0.7 with E_best < 1e-6 < the next best - the bar of the braking-log
# tests; WITHOUT the setting the best is another grid point (recorded in DESIGN.md section 6: 0.90).  At 0.02 the
# car at grip 0.7 spins under the lighter pedals tried (yaw rate 0.8 rad/s): 0.01 keeps the peak lateral acceleration near 9.3 m/s^2,
# above the 8.0 m/s^2 that grip 0.7 has without downforce.
IDENT_AMPLITUDE = 0.01
IDENT_PEDAL = -0.2


def downforce_log(amplitude=IDENT_AMPLITUDE, pedal=IDENT_PEDAL, grip=0.7, steps=40, dt=0.05, vx0=55.0, period=20,
                  coupling=(1.0, 1.0), load=LOAD):
    """(states [W + 1, 3], controls [W, 2]) float32 of the log above."""
    t = np.arange(steps)
    controls = np.stack([amplitude * np.sin(2 * np.pi * t / period), np.full(steps, pedal)], axis=1).astype(T)
    traj = _params().reference().with_grip(grip).rollout(np.array([0.0, 0.0, 0.0, vx0, 0.0, 0.0]), controls.astype(np.float64), dt,
                                                         coupling=coupling, load_transfer=load, downforce=_aero())
    return traj[:, 3:].astype(T), controls


def _identification():
    from acmpc_amd.grip_estimator import grip_scales
    base = _params().reference()
    tied = grip_scales(GRID, "tied")
    states, controls = downforce_log()
    with_aero = gs.score(base.coefficients(), states, controls, 0.05, tied, settings=Settings(coupling=(1.0, 1.0), load_transfer=LOAD, downforce=_aero()))
    without = gs.score(base.coefficients(), states, controls, 0.05, tied, settings=Settings(coupling=(1.0, 1.0), load_transfer=LOAD))
    return tied, states, with_aero, without


def test_a_fast_log_finds_the_grip_only_with_the_setting():
    tied, states, (E, best), (E_off, best_off) = _identification()
    assert states[0, 0] == 55.0 and 45.0 <= states[:, 0].min() and states[:, 0].max() <= 55.0 and np.abs(states[:, 2]).max() > 0.05
    assert tied[best, 0] == pytest.approx(0.7) and E[best] < 1e-6 < np.sort(E)[1]
    assert best_off != best and tied[best_off, 0] > 0.7           # the static model reads the downforce as grip
    print("scored without the downforce: picks grip %.2f, error %.3e (with it: %.2f, %.3e, next %.3e)"
          % (tied[best_off, 0], E_off[best_off], tied[best, 0], E[best], np.sort(E)[1]))


def test_the_estimators_rule_is_unchanged():
    """GripEstimator picks from the errors it is given: the setting changes the errors, not the rule."""
    from acmpc_amd import grip_estimator
    import inspect
    assert "downforce" not in inspect.getsource(grip_estimator)


def test_the_segment_loop_without_the_setting_is_the_load_transfers():
    from acmpc_amd.grip_estimator import grip_scales
    base = _params().reference()
    tied = grip_scales(GRID, "tied")
    states, controls = downforce_log()
    loaded = Settings(substeps=2, low_speed_blend=(3.0, 5.0), coupling=(0.9, 1.1), load_transfer=LOAD)
    b = gs.score(base.coefficients(), states, controls, 0.05, tied, segment=8, settings=loaded)
    c = gs.score(base.coefficients(), states, controls, 0.05, tied, segment=8, settings=loaded.replace(downforce=(0.0, 0.0)))
    assert np.array_equal(_bits(c[0]), _bits(b[0])) and c[1] == b[1]
    d = gs.score(base.coefficients(), states, controls, 0.05, tied, segment=8, settings=loaded.replace(downforce=_aero()))
    assert not np.array_equal(_bits(d[0]), _bits(b[0]))


# ---- 6. host refusals ---------------------------------------------------------------------------------------------------------
def _engine(**extra):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    kw = dict(dp["kw"])
    kw.update(extra)
    return Engine(**kw), dp


def _call(eng, setting):
    r = None if setting is None else np.array(setting, dtype=np.float64)
    return eng._lib.acmpc_set_dynamics_downforce(eng._ctx, None if r is None else r.ctypes.data)


def _call_load(eng, setting):
    r = None if setting is None else np.array(setting, dtype=np.float64)
    return eng._lib.acmpc_set_dynamics_load_transfer(eng._ctx, None if r is None else r.ctypes.data)


K_F, K_R = 7.35e-4, 1.1025e-3
BAD = [(-1e-4, K_R, 100.0), (K_F, -1e-4, 100.0), (NAN, K_R, 100.0), (K_F, NAN, 100.0), (INF, K_R, 100.0), (K_F, INF, 100.0),
       (1e39, K_R, 100.0), (K_F, K_R, 0.0), (K_F, K_R, -5.0), (K_F, K_R, NAN), (K_F, K_R, INF), (K_F, K_R, 1e39), (K_F, K_R, 1e-50)]
# the rear factor reaches zero 17.8 kN above static: k_r v_sat^2 = 18.6 kN at 130 m/s swallows it, 11.0 kN at 100 m/s does not -
# and there the rear vertex (5.95 kN above static) lies inside the interval and is fine (a maximum: eps_r < 0)
SWALLOWS = (K_F, K_R, 130.0)
VERTEX_INSIDE = (K_F, K_R, 100.0)
NEARLY = (K_F, K_R, 120.0)         # 15.9 kN: fine alone; with LOAD's w_max = 4.9 kN on top the interval ends at 20.8 kN


def test_entry_point_is_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    lib = acmpc_amd.load_library()
    assert "acmpc_set_dynamics_downforce" in _capi.SIGNATURES and hasattr(lib, "acmpc_set_dynamics_downforce")
    assert hasattr(acmpc_amd.Engine, "set_dynamics_downforce")


def test_set_dynamics_downforce_refusals():
    from acmpc_amd import EngineError, _capi
    vehicle = _params().reference()
    no_front = dataclasses.replace(vehicle, Df=0.0)                     # a peak that is not > 0
    no_n = dataclasses.replace(vehicle, epsr=-vehicle.F_z0 / vehicle.F_zr)   # N_r = F_zr + e_r F_zr^2 = 0
    upward = dataclasses.replace(vehicle, epsr=0.02, epsf=0.02)          # a2 > 0: a vertex that is a minimum, far below -w_max
    eng, _ = _engine()
    # from off: a refused setting leaves it off - vehicles it would refuse are still taken
    for setting in BAD:
        assert _call(eng, setting) == EINVAL, setting
        assert b"k_f" in eng._lib.acmpc_last_error(eng._ctx) or b"v_sat" in eng._lib.acmpc_last_error(eng._ctx)
        with pytest.raises(ValueError):
            eng.set_dynamics_downforce(setting)
    eng.set_dynamics(no_front)
    assert _call(eng, VERTEX_INSIDE) == EINVAL and b"Pf, Pr" in eng._lib.acmpc_last_error(eng._ctx)
    eng.set_dynamics(no_n)
    assert _call(eng, VERTEX_INSIDE) == EINVAL and b"N = " in eng._lib.acmpc_last_error(eng._ctx)
    eng.set_dynamics(vehicle)
    assert _call(eng, SWALLOWS) == EINVAL and b"load range" in eng._lib.acmpc_last_error(eng._ctx)
    eng.set_dynamics_ensemble([vehicle.with_grip(0.5), vehicle])
    assert _call(eng, SWALLOWS) == EINVAL
    eng.set_dynamics(no_front)                                           # (still off: taken)
    eng.set_dynamics(vehicle)
    for setting in (VERTEX_INSIDE, (0.0, 0.0, 1.0), (-0.0, 0.0, 50.0), NEARLY, (K_F, 0.0, 200.0), (1e-50, 1e-50, 10.0)):
        assert _call(eng, setting) == 0, setting
    eng.set_dynamics(upward)                                             # either sign of a2 is looked at, and this one is fine
    eng.set_dynamics(vehicle)
    assert _call(eng, NEARLY) == 0
    # from on: a refused setting leaves it on.  NEARLY is kept: the load transfer that would push the interval over the rear
    # factor's zero is refused by acmpc_set_dynamics_load_transfer, a smaller one is taken
    for setting in BAD + [SWALLOWS]:
        assert _call(eng, setting) == EINVAL, setting
    assert _call_load(eng, LOAD) == EINVAL and b"load range" in eng._lib.acmpc_last_error(eng._ctx)
    assert _call_load(eng, (0.35, 0.2)) == 0                             # w_max = 1.09 kN: 17.0 kN, still below the zero
    assert _call(eng, (K_F, K_R, 125.0)) == EINVAL                       # 17.2 + 1.09 kN: refused with the load transfer on ...
    assert _call_load(eng, None) == 0
    assert _call(eng, (K_F, K_R, 125.0)) == 0                            # ... and taken without it (17.2 kN)
    assert _call_load(eng, (0.35, 0.2)) == EINVAL                        # which the load transfer now breaks: refused, still off
    assert _call(eng, NEARLY) == 0
    for bad_vehicle in (no_front, no_n, dataclasses.replace(vehicle, Dr=-4.0), dataclasses.replace(vehicle, mass=1.3 * vehicle.mass, epsr=-0.16)):
        with pytest.raises(EngineError) as e:
            eng.set_dynamics(bad_vehicle)
        assert e.value.code == EINVAL
        with pytest.raises(EngineError) as e:
            eng.set_dynamics_ensemble([vehicle, vehicle.with_grip(0.5), bad_vehicle])
        assert e.value.code == EINVAL
    # NULL / None turns it off, and the same vehicles are taken again
    assert _call(eng, None) == 0
    eng.set_dynamics(no_front)
    eng.set_dynamics(vehicle)
    # the Engine's forms; the setting survives the others
    eng.set_dynamics_downforce((K_F, K_R))
    eng.set_dynamics_downforce((K_F, K_R, 90.0))
    eng.set_dynamics_downforce((K_F, K_R), v_sat=90.0)
    for wrong in ("x", (1.0,), (1.0, 0.5, 3.0, 4.0), (1.0, "y"), 3.0):
        with pytest.raises(ValueError):
            eng.set_dynamics_downforce(wrong)
    eng.set_dynamics_ensemble([vehicle, vehicle.with_grip(0.6)])
    eng.set_dynamics_integration(4, (3.0, 5.0))
    eng.set_dynamics_terms(rate_weight=(0.3, 0.02), slip_max=0.08)
    eng.set_dynamics_objective(2.0, (1.1, 0.0))
    eng.set_dynamics_coupling((0.9, 1.1))
    eng.set_dynamics_coupling(None)
    eng.set_dynamics_load_transfer(0.35)
    eng.set_dynamics_load_transfer(None)
    eng.set_dynamics_clearance(2.0, 0.5)
    with pytest.raises(EngineError):
        eng.set_dynamics(no_n)                     # still on
    eng.set_dynamics_downforce(None)
    eng.set_dynamics(no_n)
    assert _capi.dynamics_downforce(None) is None and list(_capi.dynamics_downforce((K_F, K_R))) == [K_F, K_R, 100.0]
    assert list(_capi.dynamics_downforce((K_F, K_R, 80.0))) == [K_F, K_R, 80.0]
    eng.close()
    # before any vehicle: taken, and the first vehicle is then checked
    eng, _ = _engine()
    eng.set_dynamics_downforce(VERTEX_INSIDE)
    with pytest.raises(EngineError):
        eng.set_dynamics(no_front)
    eng.set_dynamics(vehicle)
    eng.close()
    for mode in (0, 1):
        other, _ = _engine(mode=mode)
        with pytest.raises(EngineError) as e:
            other.set_dynamics_downforce((K_F, K_R))
        assert e.value.code == ESTATE
        assert _call(other, None) == ESTATE
        other.close()
    assert _capi.load_library().acmpc_set_dynamics_downforce(None, None) == EINVAL


@pytest.mark.parametrize("bad", [dict(downforce=(-1e-4, 1e-3)), dict(downforce=(NAN, 1e-3)), dict(downforce=(1e-3, INF)),
                                 dict(downforce=(1e-3, 1e-3, 0.0)), dict(downforce=(1e-3, 1e-3, INF)),
                                 dict(downforce=(1e-3,)), dict(downforce=(1e-3, 1e-3, 50.0, 1.0)), dict(downforce="wing")])
def test_solver_config_is_checked_before_any_handle_exists(bad, monkeypatch):
    from acmpc_amd import _capi
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver

    def no_engine(*args, **kwargs):
        raise AssertionError("a handle was created for a config that must be refused")

    monkeypatch.setattr(_capi, "Engine", no_engine)
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(horizon=20, n_candidates=64, **bad))


def test_solver_takes_the_key_without_device_work():
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    for value in ((K_F, K_R), (K_F, K_R, 80.0), None):
        solver = DynamicSamplingSolver(dict(horizon=10, n_candidates=8, tyre_coupling=1.0, load_transfer=0.35, downforce=value,
                                            grip_ensemble=(0.5, 1.0)))
        solver.close()


if __name__ == "__main__":
    moving, still = _mirror_figures()
    for name, figures in (("moving", moving), ("standstill", still)):
        for key, (worst, lo, hi) in figures.items():
            print("%s %s v_sat %g: %.3e, vx %.1f .. %.1f" % ((name,) + key + (worst, lo, hi)))
        print("worst %s: %.3e" % (name, max(v[0] for v in figures.values())))
    (_, xd_off, _), (_, xd_on, _) = _braking_figures()
    print("full braking from 60 m/s: vx' = %.3f m/s^2 without the downforce, %.3f with it" % (xd_off[3], xd_on[3]))
    tied, states, (E, best), (E_off, best_off) = _identification()
    print("identification with the downforce: grip %.2f error %.3e next %.3e" % (tied[best, 0], E[best], np.sort(E)[1]))
    print("identification without it:         grip %.2f error %.3e next %.3e" % (tied[best_off, 0], E_off[best_off], np.sort(E_off)[1]))
