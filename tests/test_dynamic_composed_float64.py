"""Mode D's settings COMPOSED, CPU only: the float32 restatement under one Settings value with several parts on (tests/dynamic_spec.py
- what the kernels equal bit for bit) against ONE plain float64
evaluation of the same settings (tests/dynamic_reference64.py: rollout64 with substeps=, low_speed_blend=, coupling=,
load_transfer=, terms=, u_prev=, objective=).  Each setting is held to the float64 mirror on its own elsewhere; here an error
in how the pieces meet - which peaks the blend's kinematic target sees, which state the slip line and the ceiling read under
sub-steps, which step the progress is taken at - would part the two sides.

The float64 side's step is first held to DynamicBicycleParams.predict_next_state / rollout with the same keywords, and its
added cost lines (written from DESIGN.md section 2) to acmpc_amd.dynamic_model.stage_terms / objective_terms.

Eight composed cases on the non-standstill problems of tests/test_dynamic_cost_float64.CASES with n <= 49, N = min(N, 512).
`python tests/test_dynamic_composed_float64.py` prints the measured maxima the bars come from.  Measured (NumPy 1.26,
x86-64), the largest over the eight cases:
  |c32 - c64| / max(|c64|, 1) over the candidates feasible on both sides        2.903e-4 (F: K = 3, everything on)
  the lateral drift |e_y32 - e_y64| over every candidate, vehicle and step     1.623e-4 m (B; float32 states, float64 waypoint)
  the progress drift |s32 - s64| over every candidate and vehicle              4.056e-5 m (F)
  the speed drift |vx32 - vx64| and the slip drift |b32 - b64|, every step     2.584e-5 m/s (D), 1.129e-7 (F; where a slip part is on)
  the share of excepted candidates                                              0.2 % (F; none elsewhere)
The bars are 4 x those maxima (other NumPy builds' arctan / sin / cos differ in the last place of the float64 side; the
float32 side is exact arithmetic and the same everywhere).  A rate is a difference of two float32 controls times 20: both sides
agree to two float32 roundings of at most 40 /s, RATE_BAR.  A candidate whose float64 hinge argument comes within the bar of 0
at a hard limit (rate, slip, ceiling) may be feasible on one side only: those are excepted from the feasibility comparison
alone, and the limits are chosen so that they stay under MIRROR_EXCEPTED_CAP = 2 % of a case's candidates."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "ac-mpc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acmpc_oracle as orc  # noqa: E402
import dynamic_ensemble_spec as es  # noqa: E402
import dynamic_reference64 as r64  # noqa: E402
import dynamic_spec as ds  # noqa: E402
import grip_spec as gs  # noqa: E402
from dynamic_spec import Settings  # noqa: E402
import test_dynamic_cost_float64 as c64  # noqa: E402

T = np.float32
INF = float("inf")
MIRROR_EXCEPTED_CAP = 0.02
RATE_BAR = 1.0e-5                      # 2 roundings x 2^-24 x 40 /s = 4.8e-6, rounded up
NO_TERMS = dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=None)
NO_OBJECTIVE = dict(progress_weight=0.0, speed_ceiling=None)

# measured maxima over COMPOSED (this file's __main__), and the bars
REL, EY_M, S_M, VX, B = 2.903e-4, 1.623e-4, 4.056e-5, 2.584e-5, 1.129e-7
RTOL, EY_DRIFT_M, S_DRIFT_M, VX_DRIFT, B_DRIFT = 4 * REL, 4 * EY_M, 4 * S_M, 4 * VX, 4 * B

# (index into test_dynamic_cost_float64.CASES, settings): two with the load transfer (A, C, E, F: four), two one-sided ratios
# (B, C), M > 1 with the blend (B, D, F, G), K = 3 (F)
COMPOSED = {
    "A-loaded-coupled-terms-progress": (0, dict(
        load_transfer=(0.35, 0.9), coupling=(0.9, 1.1), u_prev=(0.02, 0.1), objective=dict(progress_weight=3.0, speed_ceiling=None),
        terms=dict(rate_weight=(0.3, 0.02), rate_max=None, slip_weight=40.0, slip_max=None))),
    "B-front-inf-M3-blend-ceiling-slip": (1, dict(
        coupling=(INF, 1.1), substeps=3, low_speed_blend=(3.0, 5.0), objective=dict(progress_weight=0.0, speed_ceiling=(1.0, 0.3)),
        terms=dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=40.0, slip_max=None))),
    "C-rear-inf-loaded-progress400-rate": (2, dict(
        coupling=(0.8, INF), load_transfer=0.5, u_prev=(-0.03, 0.3), objective=dict(progress_weight=400.0, speed_ceiling=None),
        terms=dict(rate_weight=(0.3, 0.02), rate_max=(None, 6.0), slip_weight=0.0, slip_max=None))),
    "D-M4-blend-limits-alone": (8, dict(
        substeps=4, low_speed_blend=(0.0, 8.0), terms=dict(rate_weight=(0.0, 0.0), rate_max=(1.5, 6.0), slip_weight=0.0, slip_max=0.08))),
    "E-loaded-uncoupled-ceiling": (11, dict(
        load_transfer=(0.3, 0.6), objective=dict(progress_weight=0.0, speed_ceiling=1.02))),
    "F-K3-everything-M2-blend": (12, dict(
        coupling=1.0, load_transfer=(0.35, 0.9), substeps=2, low_speed_blend=(3.0, 5.0), u_prev=(0.01, -0.2),
        objective=dict(progress_weight=3.0, speed_ceiling=(1.05, 0.0)),
        terms=dict(rate_weight=(0.3, 0.02), rate_max=(1.5, 6.0), slip_weight=40.0, slip_max=0.08))),
    "G-two-steps-M5-blend-everything": (5, dict(
        coupling=(0.9, 1.1), substeps=5, low_speed_blend=(3.0, 5.0), objective=dict(progress_weight=3.0, speed_ceiling=(1.0, 0.3)),
        terms=dict(rate_weight=(0.3, 0.02), rate_max=None, slip_weight=40.0, slip_max=0.08))),
    "H-coupled-M2-progress-alone": (0, dict(
        coupling=(1.1, 0.9), substeps=2, objective=dict(progress_weight=3.0, speed_ceiling=None))),
}


def _params(grip=1.0):
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    base = DynamicBicycleParams.reference()
    return base if grip == 1.0 else base.with_grip(grip)


# ---- the float64 side against the host mirror -------------------------------------------------------------------------------
STEP_SETTINGS = [dict(coupling=(0.9, 1.1)), dict(coupling=(INF, 0.8)), dict(coupling=0.7, load_transfer=(0.35, 0.9)),
                 dict(load_transfer=0.5), dict(coupling=(1.1, INF), load_transfer=(0.0, 0.5))]


@pytest.mark.parametrize("setting", STEP_SETTINGS, ids=repr)
def test_the_float64_step_is_the_host_mirror(setting):
    """step64 (arrays) with the coupling and the load transfer against predict_next_state + the vx clip, on 300 random states
    and controls with pedals that reach both caps."""
    rng = np.random.default_rng(41)
    for params in (_params(), _params(0.6)):
        state = np.column_stack([rng.uniform(-50, 50, 300), rng.uniform(-50, 50, 300), rng.uniform(-7, 7, 300),
                                 np.where(rng.random(300) < 0.1, 0.0, rng.uniform(0, 45, 300)), rng.uniform(-2, 2, 300),
                                 rng.uniform(-1, 1, 300)])
        u = np.column_stack([rng.uniform(-0.35, 0.35, 300), np.clip(rng.uniform(-1.6, 1.6, 300), -1.0, 1.0)])
        got = r64.step64(state.copy(), u[:, 0], u[:, 1], params.coefficients(), 0.05, **setting)
        for s, c, g in zip(state, u, got):
            want = params.predict_next_state(s, c, 0.05, **setting)[0]
            want[3] = max(want[3], 0.0)
            np.testing.assert_allclose(g, want, rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize("integration", [(3, (3.0, 5.0)), (4, None), (1, (0.0, 8.0)), (16, (3.0, 5.0))])
def test_the_float64_control_step_is_the_host_mirrors_rollout(integration):
    rng = np.random.default_rng(42)
    params = _params(0.8)
    setting = dict(coupling=(0.9, 1.1), load_transfer=(0.35, 0.9))
    x0 = np.column_stack([np.zeros(12), np.zeros(12), rng.uniform(-3, 3, 12), rng.uniform(0, 12, 12), np.zeros(12), np.zeros(12)])
    U = np.stack([rng.uniform(-0.3, 0.3, (12, 20)), rng.uniform(-1, 1, (12, 20))], axis=2)
    state = x0.copy()
    for i in range(20):
        state = r64.control_step64(state, U[:, i, 0], U[:, i, 1], params.coefficients(), 0.05, *integration, **setting)
    for b in range(12):
        want = params.rollout(x0[b], U[b], 0.05, substeps=integration[0], low_speed_blend=integration[1], **setting)[-1]
        np.testing.assert_allclose(state[b], want, rtol=1e-10, atol=1e-9)


def _problem(case):
    track, kind, n, N, window, grips, reduce, weights = case
    dp = ds.make_dynamic_problem(orc, track, n + 1, min(N, 512), n, **c64.KINDS[kind])
    return dp, orc.coefficients_temporal(dp["table"], dp["kw"]["margin"])


def test_the_added_cost_lines_are_the_host_mirrors():
    """rollout64's E, the terms' and the objective's additions to V, and s against dynamic_model.stage_terms /
    objective_terms applied to rollout64's own states, candidate by candidate; and the default keywords change nothing."""
    from acmpc_amd.dynamic_model import objective_terms, stage_terms
    case = c64.CASES[0]
    dp, coef = _problem(case)
    dp["U"] = dp["U"][:48]
    n, window = case[2], case[4]
    vehicle = _params().coefficients()
    terms = dict(rate_weight=(0.3, 0.02), rate_max=(1.5, None), slip_weight=40.0, slip_max=0.02)
    objective = dict(progress_weight=2.0, speed_ceiling=(1.0, 0.1))
    plain = r64.reference_costs(dp, coef, vehicle, nn_window=window)
    for u_prev in (None, (0.02, -0.1)):
        got = r64.reference_costs(dp, coef, vehicle, nn_window=window, terms=terms, u_prev=u_prev, objective=objective)
        assert np.array_equal(got["states"], plain["states"]) and np.array_equal(got["j"], plain["j"])
        for c in range(48):
            E, V_terms = stage_terms(got["states"][c], dp["U"][c], dp["kw"]["dt"], u_prev, _params(), **terms)
            s, V_obj = objective_terms(got["states"][c], dp["U"][c], dp["table"][:, :n], nn_window=window, **objective)
            assert got["E"][c] == pytest.approx(E, rel=1e-12, abs=1e-12)
            # (the mirror reads the float64 table, rollout64 the packed rows: float32 positions, 2^-24 of some hundred metres)
            assert got["s"][c] == pytest.approx(s, rel=1e-12, abs=1e-4)
            assert got["V"][c] == pytest.approx(plain["V"][c] + V_terms + V_obj, rel=1e-12, abs=1e-12)
            assert got["J"][c] == pytest.approx(plain["J"][c] + E - 2.0 * s, rel=1e-12, abs=2e-4)
        assert np.any(got["V"] > plain["V"]) and np.all(got["E"] > 0)
    again = r64.reference_costs(dp, coef, vehicle, nn_window=window, substeps=1, low_speed_blend=None, coupling=None,
                                load_transfer=None, terms=None, u_prev=None, objective=None)
    for key in ("cost", "J", "V", "e_y", "states"):
        assert np.array_equal(again[key], plain[key]), key
    off = r64.reference_costs(dp, coef, vehicle, nn_window=window, terms=NO_TERMS, u_prev=(np.nan, 0.0), objective=NO_OBJECTIVE)
    for key in ("cost", "J", "V"):
        assert np.array_equal(off[key], plain[key]), key      # (a part that is off reads nothing: the NaN is not seen)


# ---- the composition --------------------------------------------------------------------------------------------------------
def _both_sides(name):
    index, settings = COMPOSED[name]
    case = c64.CASES[index]
    track, kind, n, N, window, grips, reduce, weights = case
    assert kind != "standstill" and n <= 49
    dp, coef = _problem(case)
    N = dp["U"].shape[0]
    kw = dp["kw"]
    terms, objective = dict(NO_TERMS, **settings.get("terms", {})), dict(NO_OBJECTIVE, **settings.get("objective", {}))
    u_prev = settings.get("u_prev")
    M, blend = settings.get("substeps", 1), settings.get("low_speed_blend")
    ratio, load = settings.get("coupling"), settings.get("load_transfer")
    px, py, psi = (coef[:, q].astype(np.float64) for q in (0, 1, 4))
    out = dict(n=n, w_bound=float(kw["w_bound"]), c32=[], V32=[], ref=[], ey=[], s=[], vx=[], b=[], settings=settings)
    for g in grips:
        vehicle = _params(g).coefficients()
        composed = Settings(M, blend, coupling=ratio, load_transfer=load, **terms, **objective)
        trace = {}
        c32, V32, X32 = ds.spec_costs(orc, dp, coef.astype(T), vehicle, nn_window=window, return_states=True, settings=composed,
                                      u_prev=u_prev, trace=trace)
        s32 = trace.get("s")
        six = gs.rollout_states(np.tile(dp["x0"], (N, 1)), dp["U"], vehicle, kw["dt"], settings=composed).astype(np.float64)
        ref = r64.reference_costs(dp, coef, vehicle, nn_window=window, substeps=M, low_speed_blend=blend, coupling=ratio,
                                  load_transfer=load, terms=terms, u_prev=u_prev, objective=objective)
        j, st = ref["j"], ref["states"]
        X, Y = X32[:, 1:, 0].astype(np.float64), X32[:, 1:, 1].astype(np.float64)
        ey32 = np.cos(psi[j]) * (Y - py[j]) - np.sin(psi[j]) * (X - px[j])
        lr = float(_params(g).lr)
        slip = lambda a: (a[:, 1:, 5] * lr - a[:, 1:, 4]) / (a[:, 1:, 3] + 1e-3)   # noqa: E731
        out["c32"].append(c32)
        out["V32"].append(V32)
        out["ref"].append(ref)
        out["ey"].append(float(np.abs(ey32 - ref["e_y"]).max()))
        out["s"].append(float(np.abs(s32.astype(np.float64) - ref["s"]).max()) if s32 is not None else 0.0)
        out["vx"].append(float(np.abs(six[:, 1:, 3] - st[:, 1:, 3]).max()))
        slip_on = terms["slip_weight"] != 0.0 or terms["slip_max"] is not None      # (what nothing reads is not measured)
        out["b"].append(float(np.abs(slip(six) - slip(st)).max()) if slip_on else 0.0)
    out["J32"], out["Vc32"] = es.combine(out["c32"], out["V32"], reduce, weights)
    out["J64"], out["Vc64"] = r64.combine64([r["cost"] for r in out["ref"]], [r["V"] for r in out["ref"]], reduce, weights)
    om = np.asarray(es.omegas(len(grips), weights), dtype=np.float64)
    out["fold"] = (lambda t: np.tensordot(om, t, axes=(0, 0))) if reduce == "mean" else (lambda t: t.max(axis=0))
    return out


def _excepted(s, bars):
    """The candidates that come within the bar of a hard limit on the float64 side, under any vehicle."""
    near = np.zeros(len(s["J64"]), dtype=bool)
    for r in s["ref"]:
        for name, slack in r["slack"].items():
            near |= (np.abs(slack) <= bars[name]).any(axis=1)
    return near


def _figures(s):
    both = (s["Vc32"] == 0) & (s["Vc64"] == 0)
    rel = np.abs(s["J32"].astype(np.float64) - s["J64"]) / np.maximum(np.abs(s["J64"]), 1.0)
    return dict(rel=float(rel[both].max()) if both.any() else 0.0, feasible=int(both.sum()), ey=max(s["ey"]), s=max(s["s"]),
                vx=max(s["vx"]), b=max(s["b"]), differ=int(np.count_nonzero((s["Vc32"] == 0) != (s["Vc64"] == 0))))


def _check(name, s):
    """test_dynamic_cost_float64._check with the hard limits' hinges in the violation's bound and test_dynamic_objective's
    exception for the candidates near a limit."""
    n, wb = s["n"], s["w_bound"]
    f = _figures(s)
    print("%s: feasible on both %d, rel %.3e, e_y drift %.3e m, s drift %.3e m, vx drift %.3e, slip drift %.3e, feasibility "
          "differs at %d" % (name, f["feasible"], f["rel"], f["ey"], f["s"], f["vx"], f["b"], f["differ"]))
    assert f["ey"] <= EY_DRIFT_M and f["s"] <= S_DRIFT_M and f["vx"] <= VX_DRIFT and f["b"] <= B_DRIFT, f
    assert f["rel"] <= RTOL, f
    bars = dict(rate_delta=RATE_BAR, rate_pedal=RATE_BAR, slip=B_DRIFT, ceiling=VX_DRIFT)
    excepted = _excepted(s, bars)
    assert np.count_nonzero(excepted) <= MIRROR_EXCEPTED_CAP * len(excepted), "%s: %d excepted" % (name, np.count_nonzero(excepted))
    J32, V32, J64, V64 = s["J32"].astype(np.float64), s["Vc32"].astype(np.float64), s["J64"], s["Vc64"]
    differ = (V32 == 0) != (V64 == 0)
    assert not np.any(differ & ~excepted), "%s: feasibility differs at %s" % (name, np.flatnonzero(differ & ~excepted)[:8])
    tol_k, vtol_k = [], []
    for c32, v32, r in zip(s["c32"], s["V32"], s["ref"]):
        hit = (v32 != 0) | (r["V"] != 0)
        bound = c64._violation_bound(r["V"], n, EY_DRIFT_M)
        for limit in r["slack"]:
            bound = bound + c64._violation_bound(r["V"], n, bars[limit])
        vtol = np.where(hit, bound, 0.0)
        assert np.all(np.abs(v32.astype(np.float64) - r["V"]) <= vtol), \
            "%s: violation off by %.3e (bound %.3e)" % (name, np.abs(v32 - r["V"]).max(), vtol.max())
        vtol_k.append(vtol)
        J = r["cost"] - wb * r["V"]
        tol_k.append(RTOL * np.maximum(np.abs(J), 1.0) + wb * vtol)
        assert np.all(np.abs(c32.astype(np.float64) - r["cost"]) <= tol_k[-1]), \
            "%s: a vehicle's cost off: worst %.3e of its tolerance" % (name, (np.abs(c32 - r["cost"]) / tol_k[-1]).max())
    tol = s["fold"](np.stack(tol_k))
    err = np.abs(J32 - J64)
    assert np.all(err <= tol), "%s: cost off at %s" % (name, np.argmax(err / tol))
    assert np.all(np.abs(V32 - V64) <= np.stack(vtol_k).max(axis=0)), name
    b32, b64 = orc.pick_best(s["J32"])[0], int(np.argmin(J64))
    assert b32 == b64 or J64[b32] - J64[b64] <= tol[b32] + tol[b64], \
        "%s: winner %d (float64 cost %.6e) against %d (%.6e)" % (name, b32, J64[b32], b64, J64[b64])
    return f


@pytest.mark.parametrize("name", list(COMPOSED))
def test_the_composed_restatement_against_the_float64_definition(name):
    f = _check(name, _both_sides(name))
    settings = COMPOSED[name][1]
    if "objective" in settings or "terms" in settings:
        assert f["feasible"] >= 8, f          # (the limits leave candidates feasible on both sides to compare)


def test_the_mix_of_settings():
    mixes = [m for _, m in COMPOSED.values()]
    assert len(mixes) == 8 and len({repr(sorted(m.items())) for m in mixes}) == 8

    def one_sided(m):
        return np.ndim(m.get("coupling")) == 1 and np.isinf(m["coupling"]).sum() == 1

    assert sum("load_transfer" in m for m in mixes) >= 2 and sum(one_sided(m) for m in mixes) >= 2
    assert sum(m.get("substeps", 1) > 1 and m.get("low_speed_blend") is not None for m in mixes) >= 2
    assert sum(len(c64.CASES[i][5]) == 3 for i, _ in COMPOSED.values()) >= 1


if __name__ == "__main__":
    worst = dict(rel=0.0, ey=0.0, s=0.0, vx=0.0, b=0.0)
    for name in COMPOSED:
        sides = _both_sides(name)
        f = _figures(sides)
        for key in worst:
            worst[key] = max(worst[key], f[key])
        bars = dict(rate_delta=RATE_BAR, rate_pedal=RATE_BAR, slip=B_DRIFT, ceiling=VX_DRIFT)
        print("%-40s feasible on both %4d of %4d  rel %.3e  e_y %.3e m  s %.3e m  vx %.3e  slip %.3e  differ %d  excepted %.4f"
              % (name, f["feasible"], len(sides["J64"]), f["rel"], f["ey"], f["s"], f["vx"], f["b"], f["differ"],
                 float(np.mean(_excepted(sides, bars)))))
    print("maxima: REL, EY_M, S_M, VX, B = %.3e, %.3e, %.3e, %.3e, %.3e" % (worst["rel"], worst["ey"], worst["s"], worst["vx"], worst["b"]))
