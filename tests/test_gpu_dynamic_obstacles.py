"""Mode D's obstacles on the MI355X ("Mode D, obstacles"; csrc/acmpc_dynamic_obstacles.hip): every call
form of the handle with discs set, bit for bit against the float32 restatement (tests/dynamic_spec.py through
tests/dynamic_fuzz_cases.specification) - per-candidate costs, the key, the feasible count and the winner's
record - at the smallest shapes the kernels can go wrong at, and DynamicSamplingSolver overtaking a slower car in closed
loop with the float64 mirror as the plant."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_fuzz_cases as fz
import dynamic_spec as ds

pytestmark = pytest.mark.gpu

T = np.float32
INF = float("inf")
CLEARANCE = (40.0, 1.0)
ALL_TERMS = dict(rate_weight=(0.3, 0.02), rate_max=(1.5, 6.0), slip_weight=40.0, slip_max=0.08)
ALL_OBJECTIVE = dict(progress_weight=3.0, speed_ceiling=(1.05, 0.0))
NANS = ("none", "some", "all")


def _checks():
    import test_gpu_fuzz_dynamic_settings as tfs
    return tfs


def _case(n, N, P=1, seed=51000, **settings):
    """A case of tests/dynamic_fuzz_cases.py's kind with this file's shapes: everything off unless `settings` says so."""
    c = fz._longest("obstacles", None, "monza", 0, N, seed=seed)
    c.update(H=n + 1, P=P, kinds=[p % 4 for p in range(P)], index="n%d-N%d" % (n, N))
    c.update(settings)
    return c


def _discs(c, dps, K_obs, nans=None):
    """One problem's discs after another's: different ones per problem, `nans[p]` of NANS."""
    n = c["H"] - 1
    nans = nans if nans is not None else ["none"] * len(dps)
    return [ds.make_obstacles(d, n, K_obs, c["seed"] + 7 * p, nan=nans[p]) for p, d in enumerate(dps)]


def _specification(c, dps, coefs, discs, clearance, centre=None, ref=None):
    """tests/dynamic_fuzz_cases.specification with each problem's discs (None: a problem without any)."""
    return fz.specification(c, orc, dps, coefs, centre, ref, obstacles=discs, clearance=clearance)


def _set_discs(eng, discs):
    eng.set_obstacles(np.stack([d[0] for d in discs]), np.stack([d[1] for d in discs]))


def run_matrix(c, K_obs, nans=None, clearance=CLEARANCE, layouts=(0, 1)):
    from acmpc_amd import Engine
    n = c["H"] - 1
    dps = fz.problems(c, orc)
    discs = _discs(c, dps, K_obs, nans)
    U = np.stack([d["U"] for d in dps])
    x0 = np.stack([d["x0"] for d in dps])
    want = None
    for layout in layouts:
        label = "K_obs %d %s clearance %s | %s" % (K_obs, nans, clearance, fz.label(dict(c, layout=layout)))
        eng = Engine(**dict(dps[0]["kw"], max_problems=c["P"], max_candidates=c["N"], max_steps=n, nn_window=c["window"]))
        try:
            fz.apply(eng, c)
            eng.set_dynamics_clearance(*clearance)
            eng.set_paths(np.stack([d["table"] for d in dps]))
            _set_discs(eng, discs)
            if want is None:
                want = _specification(c, dps, [eng.coefficients(p) for p in range(c["P"])], discs, clearance)
            data = U if layout == 0 else np.ascontiguousarray(U.transpose(0, 2, 3, 1))
            _checks().check_solve(eng.solve(x0, data, layout=layout), U, want, n, label)
        finally:
            eng.close()
    return want


def run_sampled(c, K_obs, nans=None, clearance=CLEARANCE):
    import test_gpu_dynamic_sampled as tsm
    n, N = c["H"] - 1, c["N"]
    label = "K_obs %d %s clearance %s | %s" % (K_obs, nans, clearance, fz.label(c))
    rig = tsm.Rig(c["P"], N, n, K=1, window=c["window"], seed=c["seed"], with_ref=c["with_ref"], track=c["track"], kinds=c["kinds"])
    try:
        fz.apply(rig.eng, c)
        rig.eng.set_dynamics_clearance(*clearance)
        discs = _discs(c, rig.dps, K_obs, nans)
        _set_discs(rig.eng, discs)
        centre, ref = fz.centres(c, orc, rig.dps)
        rig.centre_h, rig.ref_h = centre, ref
        rig.upload()
        costs, keys = rig.fused(N, c["index_offset"], c["sigma"], c["sample_seed"], c["round"])
        records = rig.finalize_sampled(None, N, c["sigma"], c["sample_seed"], c["round"])
        want = _specification(c, rig.dps, [rig.eng.coefficients(p) for p in range(c["P"])], discs, clearance, centre, ref)
        _checks().check_sampled(costs.cpu().numpy(), keys.cpu().numpy(), records, want, n, label)
    finally:
        rig.close()


# ---- the control matrix: rollout and finalize -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 65, 257])
@pytest.mark.parametrize("K_obs", [1, 8])
@pytest.mark.parametrize("n", [2, 9])
def test_control_matrix_rollout_and_finalize(n, K_obs, N):
    """One candidate, a tail and two workgroups; three problems with discs of their own, the last one's all NaN; both layouts."""
    want = run_matrix(_case(n, N, P=3, seed=51000 + 10 * n + K_obs), K_obs, nans=["none", "some", "all"])
    if N > 1:
        assert any(np.any(V > 0) for _, V, _ in want[:2])


TIERS = {"plain": (None, None), "coupled": ((0.9, 1.1), None), "loaded": (None, (0.35, 0.9)), "both": ((INF, 0.9), (0.35, 0.9))}


@pytest.mark.parametrize("tier", list(TIERS))
def test_each_step_tier_with_every_part_on(tier):
    ratio, load = TIERS[tier]
    integration = dict(M=2, blend=(3.0, 5.0)) if tier == "both" else {}
    c = _case(9, 65, P=2, seed=52000, ratio=ratio, load=load, terms=ALL_TERMS, objective=ALL_OBJECTIVE, previous="finite",
              window=(2, 5), **integration)
    run_matrix(c, 3, nans=["some", "none"])


@pytest.mark.parametrize("tier", ["plain", "loaded"])
def test_the_hard_part_alone(tier):
    """Weight 0: the soft part is off, and with the rate and slip parts off too the finish skips E."""
    ratio, load = TIERS[tier]
    run_matrix(_case(9, 65, seed=52500, ratio=ratio, load=load, objective=dict(progress_weight=3.0, speed_ceiling=None)), 2,
               clearance=(0.0, 1.0), layouts=(1,))


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_ensemble_of_two_vehicles(reduce):
    c = _case(9, 65, P=2, seed=53000, K=2, vehicles=[0, 1], reduce=reduce, weights=[1.0, 2.0], ratio=(0.9, 1.1), load=(0.35, 0.9),
              terms=ALL_TERMS, objective=ALL_OBJECTIVE)
    run_matrix(c, 3, nans=["none", "some"])
    run_matrix(dict(c, ratio=None, load=None), 8, layouts=(0,))


def test_two_candidates_per_lane():
    """One launch at P N = 2^20 with n = 3: in full against the one-candidate-per-lane kernels (the two halves of the
    candidates, each launch below 2^20), and against the restatement on two problems' first and last candidates."""
    from acmpc_amd import Engine
    P, N, n, K_obs = 256, 4096, 3, 3
    c = _case(n, N, P=P, seed=54000, ratio=(0.9, 1.1), load=(0.35, 0.9), terms=ALL_TERMS, objective=ALL_OBJECTIVE)
    base = [ds.make_dynamic_problem(orc, "monza", n + 1, N, c["seed"] + q, **fz.KIND[q]) for q in range(4)]
    dps = [base[p % 4] for p in range(P)]
    discs = [ds.make_obstacles(base[p % 4], n, K_obs, c["seed"] + p % 8, nan=NANS[p % 3]) for p in range(P)]
    U = np.stack([d["U"] for d in dps])
    x0 = np.stack([d["x0"] for d in dps])
    eng = Engine(**dict(base[0]["kw"], max_problems=P, max_candidates=N, max_steps=n))
    try:
        fz.apply(eng, c)
        eng.set_dynamics_clearance(*CLEARANCE)
        eng.set_paths(np.stack([d["table"] for d in dps]))
        _set_discs(eng, discs)
        whole = eng.solve(x0, np.ascontiguousarray(U.transpose(0, 2, 3, 1)), layout=1)
        halves = [eng.solve(x0, np.ascontiguousarray(U[:, lo:lo + N // 2].transpose(0, 2, 3, 1)), layout=1) for lo in (0, N // 2)]
        both = np.concatenate([h["costs"] for h in halves], axis=1)
        assert np.array_equal(whole["costs"].view(np.uint32), both.view(np.uint32))
        assert np.array_equal(whole["n_feasible"], halves[0]["n_feasible"] + halves[1]["n_feasible"])
        picked = np.r_[0:40, N - 40:N]
        for p in (1, 254):
            sub = dict(c, N=len(picked), P=1)
            dp = dict(dps[p], U=U[p][picked])
            cost, V, _ = _specification(sub, [dp], [eng.coefficients(p)], [discs[p]], CLEARANCE)[0]
            _checks().same_bits(whole["costs"][p][picked], cost, "problem %d" % p)
            assert np.any(V > 0) or p % 3 == 2
    finally:
        eng.close()


# ---- the sampled forms ----------------------------------------------------------------------------------------------------------
SAMPLED = dict(form="sampled", round=2, with_ref=True, index_offset=0, sigma=(0.04, 0.35), sample_seed=777001)


@pytest.mark.parametrize("tier", ["plain", "both"])
def test_fused_sampled_rollout_with_the_redrawn_record(tier):
    ratio, load = TIERS[tier]
    c = _case(9, 257, P=2, seed=55000, ratio=ratio, load=load, terms=ALL_TERMS, objective=ALL_OBJECTIVE, previous="finite", **SAMPLED)
    run_sampled(c, 3, nans=["some", "none"])
    run_sampled(dict(c, index_offset=fz.BIG_OFFSET, with_ref=False, N=63), 8)


@pytest.mark.parametrize("update", ["argmin", "softmin"])
def test_optimize_against_the_restated_rounds(update):
    """acmpc_optimize over 2 rounds at N = 4 096.  argmin: every round restated - its candidates drawn round the round
    before's winner, the winner's record.  softmin: acmpc_optimize against the loop of device calls (sample, solve, softmin
    mean), each of whose rounds is restated from the centre the device handed it."""
    import torch
    from acmpc_amd import Engine, _capi
    P, N, n, rounds, shrink, seed, sigma = 2, 4096, 9, 2, 0.5, 99123, (0.04, 0.35)
    c = _case(n, N, P=P, seed=56000, ratio=(0.9, 1.1), objective=dict(progress_weight=3.0, speed_ceiling=None), form="sampled",
              index_offset=0, sample_seed=seed, reduce="mean")
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, 4, c["seed"] + p, **fz.KIND[k]) for p, k in enumerate(c["kinds"])]
    discs = _discs(c, dps, 3, ["none", "some"])
    centre, ref = fz.centres(dict(c, with_ref=True), orc, dps)
    x0 = np.stack([d["x0"] for d in dps])
    eng = Engine(**dict(dps[0]["kw"], max_problems=P, max_candidates=N, max_steps=n, centre_update=update, softmin_lambda=1.0))
    try:
        fz.apply(eng, c)
        eng.set_dynamics_clearance(*CLEARANCE)
        eng.set_paths(np.stack([d["table"] for d in dps]))
        _set_discs(eng, discs)
        coefs = [eng.coefficients(p) for p in range(P)]
        got = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]

        def restated(r, centre_r, ref_r):
            cr = dict(c, round=r, sigma=(sigma[0] * shrink**r, sigma[1] * shrink**r))
            return _specification(cr, dps, coefs, discs, CLEARANCE, centre_r, ref_r)

        if update == "argmin":
            centre_r = centre
            for r in range(rounds):
                want = restated(r, centre_r, ref)
                centre_r = np.stack([w["U"][w["best"]] for w in want])
            for p, w in enumerate(want):
                rec = _capi.split_record(got[p], n)
                assert rec["owner"] == 1.0 and rec["n_feasible"] == w["n_feasible"]
                for name, value in (("cost", w["cost"][w["best"]]), ("violation", w["violation"][w["best"]]),
                                    ("u", w["U"][w["best"]]), ("x", w["x"][w["best"]])):
                    _checks().same_bits(rec[name], value, "problem %d: the record's %s" % (p, name))
            return
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream().cuda_stream
        d_x0, d_ref = torch.tensor(x0, device=dev), torch.tensor(ref, device=dev)
        U = torch.empty(P, n, 2, N, device=dev)
        rec = torch.empty(P, _capi.record_floats(n), device=dev)
        keys = torch.empty(P, dtype=torch.int64, device=dev)
        cost = torch.empty(P, N, device=dev)
        wsum = torch.empty(P, dtype=torch.float64, device=dev)
        mean = torch.tensor(centre, device=dev)
        for r in range(rounds):
            ref_r = d_ref if r == 0 else rec[:, _capi.REC_HEADER:_capi.REC_HEADER + 2 * n].contiguous()
            centre_h, ref_h = mean.cpu().numpy().copy(), ref_r.cpu().numpy().reshape(P, n, 2).copy()
            eng.sample_device(mean.data_ptr(), 2 * n, ref_r.data_ptr(), P, N, n, 1, 0, (sigma[0] * shrink**r, sigma[1] * shrink**r),
                              seed, r, U.data_ptr(), s)
            eng.solve_device(d_x0.data_ptr(), U.data_ptr(), P, N, n, 1, cost.data_ptr(), keys.data_ptr(), rec.data_ptr(), s)
            eng.softmin_device(cost.data_ptr(), keys.data_ptr(), U.data_ptr(), P, N, n, 1, mean.data_ptr(), wsum.data_ptr(), s)
            torch.cuda.synchronize()
            _checks().check_sampled(cost.cpu().numpy(), keys.cpu().numpy(), rec.cpu().numpy(), restated(r, centre_h, ref_h), n,
                                    "softmin round %d" % r)
        assert np.array_equal(got.view(np.uint32), rec.cpu().numpy().view(np.uint32)), "acmpc_optimize against the loop of device calls"
    finally:
        eng.close()


# ---- clearing -------------------------------------------------------------------------------------------------------------------
def test_cleared_obstacles_leave_the_bits_of_a_handle_that_never_had_any():
    from acmpc_amd import Engine
    c = _case(9, 65, P=2, seed=57000, terms=ALL_TERMS, ratio=(0.9, 1.1))
    n = c["H"] - 1
    dps = fz.problems(c, orc)
    U = np.stack([d["U"] for d in dps])
    x0 = np.stack([d["x0"] for d in dps])
    out = []
    for with_discs in (False, True):
        eng = Engine(**dict(dps[0]["kw"], max_problems=c["P"], max_candidates=c["N"], max_steps=n))
        try:
            fz.apply(eng, c)
            eng.set_dynamics_clearance(*CLEARANCE)
            eng.set_paths(np.stack([d["table"] for d in dps]))
            if with_discs:
                _set_discs(eng, _discs(c, dps, 4))
                with_them = eng.solve(x0, U)
                eng.set_obstacles(None)
            out.append(eng.solve(x0, U))
        finally:
            eng.close()
    assert not np.array_equal(with_them["costs"].view(np.uint32), out[0]["costs"].view(np.uint32))
    for name in ("costs", "records", "best_idx", "n_feasible"):
        assert np.array_equal(np.asarray(out[0][name]).view(np.uint32), np.asarray(out[1][name]).view(np.uint32)), name


# ---- one small fuzz -------------------------------------------------------------------------------------------------------------
FUZZ_PER_CELL = 4            # x 5 families x 2 forms: 40 draws


@pytest.mark.parametrize("form", fz.FORMS)
@pytest.mark.parametrize("family", fz.FAMILIES)
def test_drawn_settings_with_drawn_discs(family, form):
    """tests/dynamic_fuzz_cases.py's draws of (tier, parts, call form) with K_obs, the NaN padding of each problem and the
    clearance setting drawn beside them."""
    for index in range(FUZZ_PER_CELL):
        c = fz.case(family, form, index)
        rng = np.random.default_rng([fz.SEED, 77, fz.FAMILIES.index(family), fz.FORMS.index(form), index])
        K_obs = int(rng.integers(1, 9))
        nans = [NANS[int(v)] for v in rng.integers(0, 3, c["P"])]
        clearance = [(0.0, 0.0), CLEARANCE, (0.0, 2.0), (5.0, 0.0)][int(rng.integers(0, 4))]
        if form == "matrix":
            run_matrix(c, K_obs, nans, clearance, layouts=(c["layout"],))
        else:
            run_sampled(c, K_obs, nans, clearance)      # (the rig's own vehicle is replaced by the case's: fz.apply)


# ---- closed loop ----------------------------------------------------------------------------------------------------------------
LOOP_TICKS = 80
OPPONENT_GAP = 25.0          # m ahead of the ego at the start, on the centre line
OPPONENT_SPEED = 0.6         # of the ego's start speed
OPPONENT_DISCS = (-1.2, 1.2)  # along its heading, from its centre
LOOP_R = 2.0                 # each disc's radius (1.0) plus the ego's (1.0)


def _overtake(with_obstacles):
    """80 ticks on the longest straight of the closed loop's circuit (tests/test_gpu_dynamic.py), progress rewarded, a
    slower car ahead on the centre line: (the plant's smallest centre distance to either disc, the ego's lead at the end)."""
    from acmpc_amd import DynamicBicycleParams, DynamicSamplingSolver
    from acmpc_amd.dynamic_model import predict_obstacles
    import test_gpu_dynamic as tgd
    centre, v_profile, heading, _ = tgd.loop_track()
    tangent = np.gradient(heading)
    span = 800                                                   # 400 m of centre line at 0.5 m
    bend = np.convolve(np.abs(np.r_[tangent, tangent[:span]]), np.ones(span), mode="valid")[:len(centre)]
    start = int(np.argmin(bend))
    plant = DynamicBicycleParams.reference()
    n = tgd.LOOP_H - 1
    config = dict(tgd.LOOP_CONFIG, n_candidates=4096, sampling_rounds=2, sampling_sigma=(0.03, 0.3), progress_cost=3.0,
                  clearance_cost=40.0, clearance_margin=1.0)
    solver = DynamicSamplingSolver(config, plant)
    v0 = float(v_profile[start])
    state = np.array([centre[start, 0], centre[start, 1], heading[start], v0, 0.0, 0.0])
    along = np.array([np.cos(heading[start]), np.sin(heading[start])])
    opponent = centre[start] + OPPONENT_GAP * along
    velocity = OPPONENT_SPEED * v0 * along
    offsets = np.array(OPPONENT_DISCS)[:, None] * along[None, :]
    radii = np.full(len(OPPONENT_DISCS), LOOP_R)
    closest = np.inf
    try:
        for _ in range(LOOP_TICKS):
            table, _ = tgd.loop_path(centre, v_profile, state)
            discs = predict_obstacles(opponent[None, :] + offsets, np.tile(velocity, (len(offsets), 1)), n, tgd.LOOP_DT)
            obj = solver.solve(state, table, obstacles=(discs, radii) if with_obstacles else None)
            assert obj.info.status == "solved"
            u = obj.x[3 * (n + 1):].reshape(n, 2)
            state = plant.predict_next_state(state, u[0], tgd.LOOP_DT)[0]
            state[3] = max(state[3], 0.0)
            opponent = opponent + velocity * tgd.LOOP_DT
            closest = min(closest, float(np.min(np.linalg.norm(state[None, :2] - (opponent[None, :] + offsets), axis=1))))
            assert abs(tgd.loop_frenet(centre, heading, state)[0]) < tgd.LOOP_CORRIDOR
    finally:
        solver.close()
    return closest, float(np.dot(state[:2] - opponent, along))


def test_closed_loop_overtakes_a_slower_car():
    closest, lead = _overtake(True)
    blind, blind_lead = _overtake(False)
    print("overtake loop: smallest centre distance %.3f m (R = %.1f m), lead at the end %.2f m; without obstacles %.3f m, lead %.2f m"
          % (closest, LOOP_R, lead, blind, blind_lead))
    assert closest >= LOOP_R, "entered the opponent's discs: %.3f m" % closest
    assert lead > 0.0, "did not get past: %.2f m" % lead
    assert blind < LOOP_R, "the loop without obstacles never met the opponent: %.3f m" % blind
