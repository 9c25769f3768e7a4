"""Every form of the sampled rounds at its horizon limits.  One round of `acmpc_optimize` / `acmpc_control_tick` in modes S
and T is one fused launch that exists in six forms; which one runs is host arithmetic on LDS budgets and workgroup counts
(tests/test_round_forms.py holds the numbers).  Here every form runs on both sides of every number, bit for bit against
 - the manual round loop (`sample_device` -> `solve_device`, the matrix kernels test_gpu_fuzz.py holds to the C oracle),
 - the oracle alone: candidates from `orc.sample_candidates`, costs from the C restatement, its argmin,
 - for ticks the two-call path on the tables the prologue made, and the oracle's re-roll of the winner.
No tolerances.  Each case first asserts, through `describe_rounds`, that it runs the form it is named for; the last test
asserts that the parameter lists cover every form of every mode."""
import numpy as np
import pytest

import acmpc_oracle as orc
import c_oracle
from test_support import RACING, engine_kwargs, make_problem

pytestmark = pytest.mark.gpu

S, T, TW = ("S", 0, None), ("T", 1, None), ("Tw", 1, (2, 5))   # (label, mode, nearest-waypoint window)
KERNELS = {0: "single", 1: "pair", 2: "quad", 3: "trio"}
# the forms of the table in DESIGN.md (section "Forms of a sampled round"), per mode
FORMS = {"S": {"quad", "pair", "single", "rerolled", "split"},
         "T": {"trio+frames", "trio", "single", "rerolled", "split"},
         "Tw": {"trio", "single", "rerolled", "split"}}


def form_of(d):
    """The row of the table a `describe_rounds` answer falls in."""
    if not d["fused_finalize"]:
        return "split"          # a rollout launch and a finalize launch
    if not d["traced"]:
        return "rerolled"       # one wave; the fused finalize re-draws and re-rolls the winner
    return KERNELS[d["kernel"]] + ("+frames" if d["frames_in_lds"] else "")


# ---- a. acmpc_optimize: (mode, steps n, form, non-finite centre planted)
OPTIMIZE = ([(S, n, form, n == 118) for n, form in ((117, "quad"), (118, "single"), (120, "single"), (121, "rerolled"),
                                                    (682, "rerolled"), (683, "split"))] +
            [(T, n, form, n == 107) for n, form in ((7, "trio"), (8, "trio+frames"), (106, "trio+frames"), (107, "trio"),
                                                    (108, "trio"), (109, "single"), (119, "single"), (120, "rerolled"),
                                                    (256, "rerolled"), (257, "rerolled"), (372, "rerolled"), (373, "split"))] +
            [(TW, n, form, False) for n, form in ((108, "trio"), (109, "single"), (119, "single"), (120, "rerolled"),
                                                  (372, "rerolled"), (373, "split"))])
# ---- b. ticks: (mode, steps n, form)
TICKS = ([(S, n, form) for n, form in ((63, "quad"), (64, "quad"), (117, "quad"), (118, "single"), (120, "single"),
                                       (121, "rerolled"), (128, "rerolled"))] +
         [(T, n, form) for n, form in ((104, "trio+frames"), (106, "trio+frames"), (107, "trio"), (108, "trio"),
                                       (109, "single"), (119, "single"), (120, "rerolled"), (128, "rerolled"))] +
         [(TW, n, form) for n, form in ((104, "trio"), (106, "trio"), (107, "trio"), (108, "trio"), (109, "single"),
                                        (119, "single"), (120, "rerolled"), (128, "rerolled"))])
# ---- c. workgroup counts at n = 20: (P, N, traced, chained)
BLOCKS = [(1, 16384, True, True), (1, 16448, True, False), (4, 16384, True, True), (4, 16385, False, False)]
# ---- d. switches: (mode, steps n, switches, form)
SWITCHED = [(S, 115, ("ACMPC_NO_QUAD_ROUNDS",), "pair"), (S, 116, ("ACMPC_NO_QUAD_ROUNDS",), "single"),
            (S, 117, ("ACMPC_NO_QUAD_ROUNDS",), "single"), (T, 106, ("ACMPC_NO_TRIO_ROUNDS",), "single"),
            (T, 106, ("ACMPC_NO_VERIFIED_SEARCH",), "trio")]
RAGGED = {"S": (S, [(("ACMPC_TICK_NO_FLAG",), "quad"), (("ACMPC_NO_QUAD_ROUNDS",), "pair"),
                    (("ACMPC_NO_QUAD_ROUNDS", "ACMPC_NO_CHAINED_ROUNDS"), "pair"), (("ACMPC_NO_PAIR_ROUNDS",), "single"),
                    (("ACMPC_NO_PAIR_ROUNDS", "ACMPC_NO_CHAINED_ROUNDS"), "single"), (("ACMPC_NO_CHAINED_ROUNDS",), "quad"),
                    (("ACMPC_NO_TRACED_FINALIZE",), "rerolled")]),
          "T": (T, [(("ACMPC_NO_TRIO_ROUNDS",), "single"), (("ACMPC_NO_TRIO_ROUNDS", "ACMPC_NO_CHAINED_ROUNDS"), "single"),
                    (("ACMPC_NO_CHAINED_ROUNDS",), "trio+frames"), (("ACMPC_NO_TRACED_FINALIZE",), "rerolled"),
                    (("ACMPC_NO_VERIFIED_SEARCH",), "trio")]),
          "Tw": (TW, [(("ACMPC_NO_TRIO_ROUNDS",), "single"), (("ACMPC_NO_CHAINED_ROUNDS",), "trio"),
                      (("ACMPC_NO_TRACED_FINALIZE",), "rerolled")])}


def _id(value):
    if isinstance(value, tuple) and len(value) == 3 and value[0] in FORMS:
        return value[0]
    if isinstance(value, tuple):
        return "+".join(str(v).replace("ACMPC_", "") for v in value)
    return str(value)


# ---------------------------------------------------------------------------------------------------------------------------
# a. acmpc_optimize against the manual round loop and the oracle
# ---------------------------------------------------------------------------------------------------------------------------
_PROBLEMS = {}


def _problems(H, P):
    """`silverstone` problems of H points, made once per horizon and shared (read only)."""
    have = _PROBLEMS.setdefault(H, [])
    while len(have) < P:
        have.append(make_problem(orc, "silverstone", H, 4, seed=500 + len(have)))
    return have[:P]


def _inputs(problems, mode):
    u_ref = np.stack([np.stack([p["table"][orc.ROW_V], p["table"][orc.ROW_KAPPA]], axis=1) for p in problems]).astype(np.float32)
    x0 = np.stack([p["x0"] if mode == 0 else p["pose0"] for p in problems])
    return x0, u_ref


def _manual_loop(eng, x0, centre, u_ref, N, rounds, sigma, seed):
    """sample_device -> solve_device per round, the incumbent fed back: the records and the winner's cost per round."""
    import torch
    from acmpc_amd import _capi
    P, n = u_ref.shape[0], u_ref.shape[1]
    dev = torch.device("cuda", 0)
    R = _capi.record_floats(n)
    d_x0, d_centre, d_ref = (torch.tensor(a, device=dev) for a in (x0, centre, u_ref))
    U = torch.empty(P, n, 2, N, device=dev)
    rec = torch.empty(P, R, device=dev)
    keys = torch.empty(P, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    costs = []
    for r in range(rounds):
        centre_ptr, stride = (d_centre.data_ptr(), 2 * n) if r == 0 else (rec.data_ptr() + 4 * _capi.REC_HEADER, R)
        eng.sample_device(centre_ptr, stride, d_ref.data_ptr(), P, N, n, 1, 0, (sigma[0] * 0.5**r, sigma[1] * 0.5**r), seed, r,
                          U.data_ptr(), s)
        eng.solve_device(d_x0.data_ptr(), U.data_ptr(), P, N, n, 1, 0, keys.data_ptr(), rec.data_ptr(), s)
        torch.cuda.synchronize()
        costs.append(rec[:, 0].cpu().numpy().copy())
    return rec.cpu().numpy(), costs


def _oracle_round(eng, prob, p, mode, window, x0, centre, u_ref, N, sigma, seed, got, label):
    """Round 0 of problem p with no kernel involved: every candidate drawn and costed by the oracle, its argmin the record."""
    cfg = prob["cfg"]
    U = orc.sample_candidates(centre, u_ref, N, 0, p, 0, seed, sigma, prob["u_lo"], prob["u_hi"])
    w = c_oracle.make_weights(cfg["step_cost"], cfg["r_term"], cfg["final_cost"], prob["u_lo"], prob["u_hi"], 1.0e6,
                              nn_window=window)
    cost, viol, states = c_oracle.rollout(mode, x0, eng.coefficients(p), U, 0, w, return_states=True)
    best = c_oracle.argmin(cost)
    assert np.isfinite(cost[best]), label
    assert got["cost"][p] == cost[best] and got["violation"][p] == viol[best], label
    assert got["n_feasible"][p] == np.count_nonzero(viol == 0), label
    np.testing.assert_array_equal(got["u"][p], U[best], err_msg=label)
    np.testing.assert_array_equal(got["x"][p], states[best], err_msg=label)
    return U


@pytest.mark.parametrize("which,n,form,planted", OPTIMIZE, ids=_id)
def test_optimize_at_the_horizon_limits(which, n, form, planted):
    """acmpc_optimize on both sides of every horizon at which its rounds change form: three rounds equal the manual round
    loop, and a one-round call equals what the oracle draws, costs and picks without any kernel.  `planted`: problem 0's
    centre holds a NaN and an inf control, so every candidate but the reference meets the sampler's clip with them -
    fmin(fmax(., lo), hi) takes a NaN to the lower bound and +inf to the upper, on the device as in the restatement, so no
    candidate's cost is non-finite and the winner's never is."""
    from acmpc_amd import Engine
    label, mode, window = which
    P, N, rounds, sigma, seed = 2, 130, 3, (3.0, 0.01), 42
    problems = _problems(n + 1, P)
    eng = Engine(**engine_kwargs(problems[0], mode, P, N, n, nn_window=window))
    assert form_of(eng.describe_rounds(P, N, n)) == form
    eng.set_paths(np.stack([p["table"] for p in problems]))
    x0, u_ref = _inputs(problems, mode)
    centre = u_ref.copy()
    if planted:
        centre[0, n // 2, 0] = np.nan
        centre[0, 0, 1] = np.inf
    out = eng.optimize(x0, centre, u_ref, N, rounds, sigma, shrink=0.5, seed=seed)
    want, costs = _manual_loop(eng, x0, centre, u_ref, N, rounds, sigma, seed)
    np.testing.assert_array_equal(out["records"], want)
    assert np.isfinite(out["records"]).all()
    for a, b in zip(costs, costs[1:]):
        assert (b <= a).all()
    first = eng.optimize(x0, centre, u_ref, N, 1, sigma, shrink=0.5, seed=seed)
    for p, prob in enumerate(problems):
        U = _oracle_round(eng, prob, p, mode, window, x0[p], centre[p], u_ref[p], N, sigma, seed, first,
                          "%s n %d problem %d" % (label, n, p))
        if planted and p == 0:
            lo, hi = prob["u_lo"].astype(np.float32), prob["u_hi"].astype(np.float32)
            others = np.arange(N) != 1
            assert (U[others, n // 2, 0] == lo[0]).all() and (U[others, 0, 1] == hi[1]).all() and np.isfinite(U).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# b. ticks up to the prologue's limit
# ---------------------------------------------------------------------------------------------------------------------------
def _tick_engine(mode, window, n, N, track="monza", v_max=28.0, v_min=8.0, problems=1):
    from acmpc_amd import Engine
    cfg = RACING[track]
    lim = orc.vehicle_limits(2.65, 1.94, 0.30, v_min, v_max)
    lo, hi = orc.input_box(lim)
    return Engine(mode=mode, max_problems=problems, max_candidates=N, max_steps=n, step_cost=cfg["step_cost"], r_term=cfg["r_term"],
                  final_cost=cfg["final_cost"], u_min=lo, u_max=hi, margin=lim.margin, wheelbase=lim.length, dt=0.05,
                  nn_window=window), (lo, hi)


def _tick(H, cons, N, rounds, offset, seed):
    from acmpc_amd import _capi
    t = _capi.Tick()
    t.struct_size = _capi.C.sizeof(_capi.Tick)
    t.horizon, t.localised, t.has_end_velocity = H, 0, 1
    t.n_candidates, t.rounds, t.centre_is_reference = N, rounds, 1
    t.qp_max_iter, t.qp_check_every = 4000, 10
    t.offset = offset
    t.v_min, t.v_max, t.a_min, t.a_max = cons["v_min"], cons["v_max"], cons["a_min"], cons["a_max"]
    t.ay_max, t.ki_min, t.end_velocity = cons["ay_max"], cons["ki_min"], cons["end_velocity"]
    t.sigma[0], t.sigma[1], t.shrink = 0.5, 1e-3, 0.5
    t.qp_eps_abs = t.qp_eps_rel = 1e-3
    t.seed = seed
    return t


def _path(H):
    """The path family of test_tick_equals_set_paths_plus_optimize_in_mode_t."""
    y = np.linspace(0, 2.45 * H, H)
    return np.stack([0.004 * y ** 2, y, np.linspace(10, 6, H)], axis=1)


def _check_tick(eng, out, mode, window, n, N, rounds, seed, centre, box, track="monza", label=""):
    """One tick's result against the two-call path on the tables its prologue made, the oracle's re-roll of the winner,
    and the record its unpacked plan must follow from."""
    assert out["info"][4] == 0 and out["info"][7] == 0, label
    rec = out["record"]
    x0, u_ref, coef = eng.tick_device_tables(n)
    eng.set_paths(out["table"])
    eng.set_coefficients(coef)   # the device's own rows (a host cos / sin may differ from them in a last float32 bit)
    start = u_ref if centre is None else centre
    best = eng.optimize(x0[None], start[None], u_ref[None], N, rounds, (0.5, 1e-3), shrink=0.5, seed=seed)
    np.testing.assert_array_equal(best["records"][0], rec, err_msg=label)
    cfg = RACING[track]
    lo, hi = box
    U = rec[4:4 + 2 * n].reshape(1, n, 2)
    if mode == 0:
        cost, viol, X = orc.rollout_spatial(x0, coef, U, cfg["step_cost"], cfg["r_term"], cfg["final_cost"], lo, hi, 1.0e6,
                                            dtype=np.float32, return_states=True)[:3]
    else:
        cost, viol, X = orc.rollout_temporal(x0, coef, U, cfg["step_cost"], cfg["r_term"], cfg["final_cost"], lo, hi, 1.0e6,
                                             0.05, dtype=np.float32, return_states=True, nn_window=window)[:3]
    assert rec[0] == cost[0] and rec[1] == viol[0], label
    np.testing.assert_array_equal(rec[4 + 2 * n:].reshape(n + 1, 3), X[0], err_msg=label)
    # dec.x = [x ; u] from the record's [u ; x] blocks, and the unpacked plan
    np.testing.assert_array_equal(out["decision"][:3 * (n + 1)], rec[4 + 2 * n:].astype(np.float64))
    np.testing.assert_array_equal(out["decision"][3 * (n + 1):], rec[4:4 + 2 * n].astype(np.float64))
    np.testing.assert_array_equal(out["projected_control"][0], rec[4:4 + 2 * n:2].astype(np.float64))
    if mode == 0:
        np.testing.assert_array_equal(out["cum_time"], rec[4 + 2 * n + 2::3][:n].astype(np.float64))
    else:
        np.testing.assert_array_equal(out["prediction"], rec[4 + 2 * n:].reshape(n + 1, 3)[:n, :2].astype(np.float64))
        np.testing.assert_allclose(out["cum_time"], 0.05 * np.arange(n), rtol=0, atol=1e-15)
        np.testing.assert_allclose(out["accelerations"], np.diff(out["projected_control"][0]) / 0.05, rtol=1e-12, atol=1e-12)


def _two_ticks(which, n, N, rounds, form):
    label, mode, window = which
    H = n + 1
    coords = _path(H)
    cons = dict(RACING["monza"]["speed_profile_constraints"], v_max=28.0)
    eng, box = _tick_engine(mode, window, n, N)
    d = eng.describe_rounds(1, N, n)
    assert form_of(d) == form and d["tick_accepted"]
    assert d["tick_frames"] == (form == "trio+frames")
    out = eng.control_tick(_tick(H, cons, N, rounds, 0.25, 77), coords, None)
    _check_tick(eng, out, mode, window, n, N, rounds, 77, None, box, label="%s n %d, first tick" % (label, n))
    if mode == 1:
        np.testing.assert_array_equal(eng.tick_device_tables(n)[0], np.array([0.25, 0.0, np.pi / 2], dtype=np.float32))
    # a second, warm-started tick on the same handle
    centre = out["decision"][3 * (n + 1):].reshape(n, 2).astype(np.float32)
    t2 = _tick(H, cons, N, rounds, 0.3, 78)
    t2.centre_is_reference = 0
    again = eng.control_tick(t2, coords, centre)
    _check_tick(eng, again, mode, window, n, N, rounds, 78, centre, box, label="%s n %d, second tick" % (label, n))
    eng.close()


@pytest.mark.parametrize("which,n,form", TICKS, ids=_id)
def test_tick_at_every_form_boundary(which, n, form):
    """Ticks of both modes on both sides of every horizon at which the rounds change form, up to the 128 steps the prologue
    takes (S: 63 | 64 steps also straddle the longest path that travels in the launch's arguments): a cold tick and a
    warm-started one, each held to set_paths + set_coefficients(device rows) + optimize and to the oracle's re-roll."""
    _two_ticks(which, n, 1000, 2, form)


def test_mode_t_tick_from_the_bound_map_at_107_steps():
    """The path cut out of the bound map (coords = None) at the first horizon whose frames no longer fit: three waves that
    scan every waypoint, no frames tabulated.  108 points do not divide the 500-point resampling: 4 x 108 are asked for,
    as the controller does."""
    from acmpc_amd import workloads
    n, N, rounds = 107, 1000, 2
    cons = dict(RACING["silverstone"]["speed_profile_constraints"], v_max=float(RACING["silverstone"]["unlocalised_max_speed"]))
    eng, box = _tick_engine(1, None, n, N, track="silverstone", v_max=cons["v_max"], v_min=cons["v_min"])
    d = eng.describe_rounds(1, N, n)
    assert form_of(d) == "trio" and d["tick_accepted"] and not d["tick_frames"] and d["frames_tabulated"]
    track = workloads.synthetic_track("silverstone")
    eng.bind_map(track["centre"], track["spacing"])
    t = _tick(n + 1, cons, N, rounds, 0.3, 31)
    t.map_index, t.centreline_points, t.lateral_offset = 1234, 4 * (n + 1), 0.3
    out = eng.control_tick(t, None, None)
    assert out["info"][6] == 1234
    want, first = eng.map_reference_path(n + 1, map_index=1234, lateral_offset=0.3, centreline_points=4 * (n + 1))
    assert first == 1234
    np.testing.assert_array_equal(out["coords"], want)
    _check_tick(eng, out, 1, None, n, N, rounds, 31, None, box, track="silverstone", label="bound map")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# c. workgroup-count limits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,N,traced,chained", BLOCKS)
@pytest.mark.parametrize("which", [S, T, TW], ids=_id)
def test_optimize_at_the_workgroup_count_limits(which, P, N, traced, chained):
    """256 | 257 workgroups per problem (chained or not) and 1024 | 1028 per launch (traced because of size, or not) at 20
    steps: the manual round loop's records, and the winner re-rolled by the oracle."""
    from acmpc_amd import Engine
    label, mode, window = which
    n, rounds, sigma, seed = 20, 3, (3.0, 0.01), 42
    problems = _problems(n + 1, P)
    eng = Engine(**engine_kwargs(problems[0], mode, P, N, n, nn_window=window))
    d = eng.describe_rounds(P, N, n)
    assert (d["fused_finalize"], d["traced"], d["chained"]) == (True, traced, chained)
    assert form_of(d) == ("rerolled" if not traced else {"S": "quad", "T": "trio+frames", "Tw": "trio"}[label])
    eng.set_paths(np.stack([p["table"] for p in problems]))
    x0, u_ref = _inputs(problems, mode)
    out = eng.optimize(x0, u_ref, u_ref, N, rounds, sigma, shrink=0.5, seed=seed)
    want, _ = _manual_loop(eng, x0, u_ref, u_ref, N, rounds, sigma, seed)
    np.testing.assert_array_equal(out["records"], want)
    for p, prob in enumerate(problems):
        cfg = prob["cfg"]
        w = c_oracle.make_weights(cfg["step_cost"], cfg["r_term"], cfg["final_cost"], prob["u_lo"], prob["u_hi"], 1.0e6,
                                  nn_window=window)
        cost, viol, states = c_oracle.rollout(mode, x0[p], eng.coefficients(p), out["u"][p][None], 0, w, return_states=True)
        assert out["cost"][p] == cost[0] and out["violation"][p] == viol[0] and np.isfinite(cost[0])
        np.testing.assert_array_equal(out["x"][p], states[0])
    eng.close()


@pytest.mark.parametrize("which", [S, T], ids=_id)
def test_tick_with_257_workgroups(which):
    """A tick whose rounds are traced but one workgroup too many to be chained: every round finalizes."""
    label, mode, window = which
    n, N = 20, 16448
    eng, _ = _tick_engine(mode, window, n, N)
    d = eng.describe_rounds(1, N, n)
    assert d["traced"] and not d["chained"]
    eng.close()
    _two_ticks(which, n, N, 2, "quad" if mode == 0 else "trio+frames")


# ---------------------------------------------------------------------------------------------------------------------------
# d. switch-forced forms away from H = 50
# ---------------------------------------------------------------------------------------------------------------------------
def _warm_ticks(which, n, N):
    """Four warm-started ticks on a fresh handle (which reads the switches when it is created), and what it ran."""
    label, mode, window = which
    H = n + 1
    cons = dict(RACING["monza"]["speed_profile_constraints"], v_max=28.0)
    y = np.linspace(0, 2.45 * H, H)
    eng, _ = _tick_engine(mode, window, n, N)
    d = eng.describe_rounds(1, N, n)
    outs, centre = [], None
    for j in range(4):
        coords = np.stack([0.004 * (1 + 0.1 * j) * y ** 2, y, np.linspace(10, 6, H)], axis=1)
        t = _tick(H, cons, N, 2, 0.1 * j, 5 + j)
        t.centre_is_reference = 1 if centre is None else 0
        out = eng.control_tick(t, coords, centre)
        assert out["info"][4] == 0 and out["info"][7] == 0
        centre = out["decision"][3 * (n + 1):].reshape(n, 2).astype(np.float32)
        outs.append(out)
    eng.close()
    return d, outs


def _same_ticks(reference, got, note):
    for want, have in zip(reference, got):
        for key in ("record", "table", "decision", "projected_control", "prediction", "cum_time", "coords"):
            np.testing.assert_array_equal(want[key], have[key], err_msg="%s with %s" % (key, note))
        np.testing.assert_array_equal(want["info"][:6], have["info"][:6])


@pytest.mark.parametrize("which,n,switches,form", SWITCHED, ids=_id)
def test_switch_forced_forms_at_the_horizon_limits(which, n, switches, form, monkeypatch):
    """Mode S without the four-wave form: two waves at 115 steps, and at 116 and 117 - where four waves fit and two do not -
    the fall through both to one wave.  Mode T at the last horizon with frames: one wave, and three waves that scan every
    waypoint.  Four warm-started ticks give the default form's numbers."""
    default, reference = _warm_ticks(which, n, 1000)
    assert form_of(default) == {"S": "quad", "T": "trio+frames"}[which[0]]
    for name in switches:
        monkeypatch.setenv(name, "1")
    forced, got = _warm_ticks(which, n, 1000)
    assert form_of(forced) == form
    _same_ticks(reference, got, switches)


@pytest.mark.parametrize("label", sorted(RAGGED))
def test_tick_forms_agree_on_a_ragged_shape(label, monkeypatch):
    """test_tick_forms_agree / test_mode_t_tick_forms_agree at H = 20 with 1000 candidates (a ragged last wave, sixteen
    workgroups): every switch set moves the form the way it says and gives the default's numbers."""
    which, switch_sets = RAGGED[label]
    n = 19
    default, reference = _warm_ticks(which, n, 1000)
    assert form_of(default) == {"S": "quad", "T": "trio+frames", "Tw": "trio"}[label] and default["chained"]
    for switches, form in switch_sets:
        for name in switches:
            monkeypatch.setenv(name, "1")
        forced, got = _warm_ticks(which, n, 1000)
        assert form_of(forced) == form, switches
        assert forced["chained"] == (form != "rerolled" and "ACMPC_NO_CHAINED_ROUNDS" not in switches), switches
        _same_ticks(reference, got, switches)
        for name in switches:
            monkeypatch.delenv(name)


# ---------------------------------------------------------------------------------------------------------------------------
def test_every_form_of_every_mode_is_in_the_parameter_lists(monkeypatch):
    """Over the cases above - asked of `describe_rounds` again, so whatever was selected to run - every (mode, form) pair of
    the table is exercised by acmpc_optimize, and every one a tick can take (all but the separate finalize launch, which
    starts beyond the prologue's 128 steps) by a tick; the two-wave form, which only a switch selects, by the switched ticks."""
    def ask(which, P, N, n):
        eng, _ = _tick_engine(which[1], which[2], n, N, problems=P)
        d = eng.describe_rounds(P, N, n)
        eng.close()
        return d

    optimize = {(which[0], form_of(ask(which, 2, 130, n))) for which, n, _, _ in OPTIMIZE}
    ticks = {(which[0], form_of(ask(which, 1, 1000, n))) for which, n, _ in TICKS}
    switched = set()
    for which, n, switches, _ in SWITCHED:
        for name in switches:
            monkeypatch.setenv(name, "1")
        switched.add((which[0], form_of(ask(which, 1, 1000, n))))
        for name in switches:
            monkeypatch.delenv(name)
    everything = {(label, form) for label, forms in FORMS.items() for form in forms}
    assert optimize | switched == everything, sorted(everything - optimize - switched)
    assert optimize == everything - {("S", "pair")}
    assert ticks == everything - {("S", "pair")} - {(label, "split") for label in FORMS}
    assert ("S", "pair") in switched and ("S", "single") in switched and ("T", "single") in switched and ("T", "trio") in switched
    # and the declared forms are the ones the cases assert before they run
    assert {(which[0], form) for which, _, form, _ in OPTIMIZE} == optimize
    assert {(which[0], form) for which, _, form in TICKS} == ticks
