"""Mode D's actuator lag (acmpc_set_dynamics_actuator, acmpc_set_actuator_state) on the MI355X, from every call form.  Costs, keys,
feasible counts, records (u the command, x the lagged trajectory) and traces must be bit-identical to
tests/dynamic_actuator_spec.py; tau = (0, 0) and a constant command from its own position are held to the same handle with the
setting off; positions for another P are refused; DynamicSamplingSolver and the controller take `actuator_lag`.

Every case: tau = (0.12, 0.06), P = 2 on the dense problems of tests/test_dynamic_actuator.py (problem 0 from a standstill,
problem 1 at the path's speed) with different positions per problem, one case with the positions cleared.  Shapes: n = 3 and 20;
N = 70 (a wave's tail) and 257 (one candidate past a workgroup); N = 4099 at two candidates per lane (its last pair half empty).
A chosen few dozen combinations of layout, search, integration, tier, surface table, obstacles and ensemble - not the product."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_actuator_spec as das
import dynamic_sampled_spec as dsamp
import dynamic_softmin_spec as sms
import dynamic_spec as ds
import dynamic_surface_spec as dss
from dynamic_spec import Settings
import test_dynamic_actuator as tda
import test_gpu_dynamic as tgd
import test_gpu_dynamic_coupling as tgc
import test_gpu_dynamic_ensemble as tge
import test_gpu_dynamic_load_transfer as tgl
import test_gpu_dynamic_packed as tpk
import test_gpu_dynamic_softmin as tsf
import test_gpu_dynamic_terms as tgt

pytestmark = pytest.mark.gpu

T = np.float32
EINVAL, ESTATE = -1, -5
P = 2
TAU = tda.TAU
LOAD, AERO = tda.LOAD, tda.AERO
DEFAULT, FINE = tgc.DEFAULT, tgc.FINE
OFF, ALL_FOUR = tgc.OFF, tgc.ALL_FOUR
_vehicle, _u32 = tgc._vehicle, tgc._u32
_same_where_finite = tgl._same_where_finite
TIERS = {"none": (None, None, None), "loaded-coupled-downforce": ((0.9, 1.1), LOAD, AERO)}
GRIPS = (0.5, 0.8, 1.0)
WEIGHTS = (1.0, 2.0, 0.5)
SIGMA = (0.05, 0.3)


def _tables(n, seed, count=P):
    return np.stack([dss.random_table(n, seed + p) for p in range(count)])


def _set(eng, tier, setting=OFF, u_prev=None, integration=DEFAULT):
    ratio, load, aero = TIERS[tier]
    eng.set_dynamics_integration(*integration)
    eng.set_dynamics_coupling(ratio)
    eng.set_dynamics_load_transfer(load)
    eng.set_dynamics_downforce(aero)
    eng.set_dynamics_objective(**setting[0])
    eng.set_dynamics_terms(**setting[1])
    eng.set_previous_control(u_prev)


def _settings(tier, setting, integration, clearance=False):
    ratio, load, aero = TIERS[tier]
    extra = dict(clearance_weight=40.0, clearance_margin=1.0) if clearance else {}
    return Settings(*integration, **setting[0], **setting[1], coupling=ratio, load_transfer=load, downforce=aero, **extra)


def _vehicles(K):
    return [_vehicle()] if K == 1 else [_vehicle().with_grip(g) for g in GRIPS[:K]]


def _handle(dps, N, n, window, K, reduce="mean", **extra):
    eng = tge._engine(dps, P, N, n, window, **extra)
    if K == 1:
        eng.set_dynamics(_vehicle())
    else:
        eng.set_dynamics_ensemble(_vehicles(K), weights=WEIGHTS[:K], reduce=reduce)
    return eng


def _spec(dp, coef, K, reduce, **kw):
    blocks = [v.coefficients() for v in _vehicles(K)]
    if K == 1:
        return das.spec_costs(orc, dp, coef, blocks[0], **kw)
    return das.spec_ensemble(orc, dp, coef, blocks, reduce=reduce, weights=WEIGHTS[:K], **kw)


def _dress(eng, dps, n, seed, surface, K_obs, given):
    """The surface table, the obstacles and the actuator positions of a case on the handle: (mu, discs, a0), None where off."""
    mu = _tables(n, seed) if surface else None
    discs = [ds.make_obstacles(d, n, K_obs, 2800 + seed + p) for p, d in enumerate(dps)] if K_obs else None
    a0 = tda.positions(P, seed) if given else None
    eng.set_surface(mu)
    if discs is not None:
        eng.set_dynamics_clearance(40.0, 1.0)
        eng.set_obstacles(np.stack([d[0] for d in discs]), np.stack([d[1] for d in discs]))
    eng.set_dynamics_actuator(TAU)
    eng.set_actuator_state(a0)
    return mu, discs, a0


def _kw(p, window, s, prev, mu, discs, a0):
    return dict(nn_window=window, settings=s, u_prev=None if prev is None else prev[p], surface=None if mu is None else mu[p],
                obstacles=None if discs is None else discs[p], actuator=TAU, a0=None if a0 is None else a0[p])


# ---- 3: the control-matrix solve against the restatement ------------------------------------------------------------------------
# (n, N, layout, window, integration, tier, all four terms, surface table, obstacle discs, K, reduce, positions given)
SOLVES = [
    (3, 70, 0, None, DEFAULT, "none", False, False, 0, 1, "mean", True),
    (3, 257, 1, (2, 5), FINE, "loaded-coupled-downforce", True, True, 0, 1, "mean", True),
    (3, 70, 1, (2, 5), DEFAULT, "loaded-coupled-downforce", True, False, 2, 3, "max", False),
    (20, 70, 1, None, FINE, "none", True, True, 2, 1, "mean", True),
    (20, 257, 0, (2, 5), DEFAULT, "loaded-coupled-downforce", False, False, 2, 1, "mean", True),
    (20, 257, 1, None, DEFAULT, "none", False, False, 0, 1, "mean", False),
    (20, 70, 0, (2, 5), FINE, "loaded-coupled-downforce", True, True, 0, 1, "mean", True),
    (20, 257, 0, None, FINE, "none", False, True, 2, 1, "mean", False),
    (20, 70, 0, None, DEFAULT, "none", False, False, 0, 3, "mean", True),
    (20, 257, 1, (2, 5), FINE, "loaded-coupled-downforce", True, True, 2, 3, "max", True),
    (3, 257, 0, (2, 5), DEFAULT, "loaded-coupled-downforce", True, True, 0, 3, "mean", False),
    (20, 257, 1, None, FINE, "none", True, False, 0, 3, "max", True),
]


@pytest.mark.parametrize("n,N,layout,window,integration,tier,terms,surface,K_obs,K,reduce,given", SOLVES)
def test_costs_argmin_and_record_are_the_specification(n, N, layout, window, integration, tier, terms, surface, K_obs, K, reduce, given):
    from acmpc_amd import _capi
    dps = tda.problems(n, N)
    setting, prev = (ALL_FOUR, tgt._previous(P, 51)) if terms else (OFF, None)
    eng = _handle(dps, N, n, window, K, reduce)
    try:
        _set(eng, tier, setting, prev, integration)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        x0 = np.stack([d["x0"] for d in dps])
        mu, discs, a0 = _dress(eng, dps, n, 10 * n + N, surface, K_obs, given)
        out = eng.solve(x0, U_in, layout=layout)
        s = _settings(tier, setting, integration, clearance=K_obs > 0)
        for p in range(P):
            cost, V, X = _spec(dps[p], eng.coefficients(p), K, reduce, return_states=True, **_kw(p, window, s, prev, mu, discs, a0))
            tgd._same_bits(out["costs"][p], cost)
            rec = _capi.split_record(out["records"][p], n)
            best = tgd._check_record(rec, U_h[p], cost, V, X, n)       # (u: the command; x: the lagged trajectory)
            assert out["best_idx"][p] == best and out["n_feasible"][p] == np.count_nonzero(V == 0)
            tgd._same_bits(rec["cost"], out["costs"][p][best])          # the finalize's re-roll gives the rollout's own cost
        assert np.isnan(out["costs"][0][5]) and not np.isfinite(out["costs"][1][7])
        # the device really filters: the same handle with the setting off scores the candidates differently
        eng.set_dynamics_actuator(None)
        off = eng.solve(x0, U_in, layout=layout)["costs"]
        moved = np.count_nonzero(_u32(off[1]) != _u32(out["costs"][1]))
        assert moved > (0 if terms else N // 2)      # (under the rate limits most costs are w_bound V of the COMMAND'S hinges)
    finally:
        eng.close()


# ---- 3: two candidates per lane -------------------------------------------------------------------------------------------------
PACKED_N, PACKED_STEPS = 4099, 12


@pytest.mark.parametrize("K,layout,window,surface", [(1, 1, None, True), (2, 0, (2, 5), False)])
def test_packed_rollout_carries_two_pairs_of_positions_per_lane(K, layout, window, surface):
    n = PACKED_STEPS
    count = tpk._problems_for(PACKED_N, K)
    assert count * PACKED_N * K >= tpk.PACKED and (count - 1) * PACKED_N * K < tpk.PACKED
    base = [dss.make_dense_problem(orc, n + 1, PACKED_N, 2860 + q, vx0=v) for q, v in enumerate((None, 0.0, None, 14.0))]
    rng = np.random.default_rng(2860)
    U = np.stack([base[p % 4]["U"] for p in range(count)])
    U[..., 0] += rng.standard_normal(U.shape[:-1], dtype=T) * T(0.01)
    U[..., 0] = np.clip(U[..., 0], ds.U_MIN[0], ds.U_MAX[0])
    x0 = np.stack([base[p % 4]["x0"] for p in range(count)])
    tables = np.stack([base[p % 4]["table"] for p in range(count)])
    kinds_mu, kinds_a0 = _tables(n, 61, 4), tda.positions(4, 62)
    mu = np.stack([kinds_mu[p % 4] for p in range(count)]) if surface else None
    a0 = np.stack([kinds_a0[p % 4] for p in range(count)])
    planted = tpk._plant(U, PACKED_N, n)
    assert planted[0] == [PACKED_N - 1]                 # the NaN pedal in the last odd candidate
    vehicles = [_vehicle(), _vehicle().with_grip(0.6)][:K]
    label = "K %d layout %d window %s P %d" % (K, layout, window, count)
    eng = tge._engine([base[p % 4] for p in range(count)], count, PACKED_N, n, window)
    try:
        if K == 1:
            eng.set_dynamics(vehicles[0])
        else:
            eng.set_dynamics_ensemble(vehicles, weights=(1.0, 2.0), reduce="mean")
        _set(eng, "loaded-coupled-downforce", ALL_FOUR, None)
        eng.set_surface(mu)
        eng.set_dynamics_actuator(TAU)
        eng.set_actuator_state(a0)
        U_in = tpk._as_layout(U, layout)
        out = eng.solve(x0, U_in, layout=layout)
        coefs = [eng.coefficients(q) for q in range(4)]
        s = _settings("loaded-coupled-downforce", ALL_FOUR, DEFAULT)

        def spec(q, U_sub, states):
            return das.spec_ensemble(orc, base[q], coefs[q], [v.coefficients() for v in vehicles], reduce="mean",
                                     weights=(1.0, 2.0)[:K], nn_window=window, U=U_sub, return_states=states, settings=s,
                                     surface=kinds_mu[q] if surface else None, actuator=TAU, a0=kinds_a0[q])

        group = tpk.GROUP_ONE if K == 1 else tpk.GROUP_ENSEMBLE
        tpk._check_against_spec(out, base, coefs, U, PACKED_N, n, group, planted, spec, 17 + K, label)
        # packed against unpacked slices of the same handle, each slice with its own rows of the table and the positions
        chunk = (tpk.PACKED - 1) // (PACKED_N * K)
        assert 1 <= chunk < count
        for lo in range(0, count, chunk):
            hi = min(lo + chunk, count)
            eng.set_paths(tables[lo:hi])
            eng.set_surface(None if mu is None else mu[lo:hi])
            eng.set_actuator_state(a0[lo:hi])
            part = eng.solve(x0[lo:hi], U_in[lo:hi], layout=layout)
            tgd._same_bits(part["costs"], out["costs"][lo:hi])
            assert np.array_equal(part["best_idx"], out["best_idx"][lo:hi]), label
            assert np.array_equal(part["records"].view(np.uint32), out["records"][lo:hi].view(np.uint32)), label
    finally:
        eng.close()


# ---- 3: the sampled forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N,window,integration,tier,terms,surface,K_obs,K,reduce,given,offset", [
    (20, 257, (2, 5), DEFAULT, "none", False, False, 0, 1, "mean", True, 0),
    (20, 70, None, FINE, "loaded-coupled-downforce", True, True, 2, 1, "mean", True, tgc.BIG_OFFSET),
    (3, 257, None, DEFAULT, "loaded-coupled-downforce", True, True, 0, 3, "max", False, 0),
    (20, 257, (2, 5), FINE, "none", True, False, 2, 3, "mean", True, tgc.BIG_OFFSET)])
def test_fused_sampled_rollout_redrawn_finalize_and_a_softmin_round(n, N, window, integration, tier, terms, surface, K_obs, K,
                                                                     reduce, given, offset):
    import torch
    from acmpc_amd import _capi
    dps = tda.problems(n, N)
    setting, prev = (ALL_FOUR, tgt._previous(P, 52)) if terms else (OFF, None)
    lam, seed, rnd = 0.5, 77, 1
    eng = _handle(dps, N, n, window, K, reduce, softmin_lambda=lam)
    try:
        _set(eng, tier, setting, prev, integration)
        mu, discs, a0 = _dress(eng, dps, n, 20 * n + N, surface, K_obs, given)
        centre, ref = tsf._centres(dps, n, 6)
        x0 = np.stack([d["x0"] for d in dps])
        dev, s = torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
        d_x0, d_c, d_r = (torch.tensor(a, device=dev) for a in (x0, centre, ref))
        costs, keys = torch.empty(P, N, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
        rec = torch.empty(P, _capi.record_floats(n), device=dev)
        mean, wsum = torch.empty(P, n, 2, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
        eng.rollout_sampled_device(d_x0.data_ptr(), d_c.data_ptr(), 2 * n, d_r.data_ptr(), P, N, n, offset, SIGMA, seed, rnd,
                                   costs.data_ptr(), keys.data_ptr(), s)
        eng.finalize_sampled_device(0, d_x0.data_ptr(), d_c.data_ptr(), 2 * n, d_r.data_ptr(), P, N, n, SIGMA, seed, rnd,
                                    rec.data_ptr(), s)
        eng.softmin_sampled_device(costs.data_ptr(), keys.data_ptr(), d_c.data_ptr(), 2 * n, d_r.data_ptr(), P, N, n, offset, SIGMA,
                                   seed, rnd, mean.data_ptr(), wsum.data_ptr(), s)
        torch.cuda.synchronize()
        st = _settings(tier, setting, integration, clearance=K_obs > 0)
        for p in range(P):
            U = dsamp.candidates(orc, dps[p], centre[p], ref[p], N, offset, p, rnd, seed, SIGMA)
            cost, V, X = _spec(dps[p], eng.coefficients(p), K, reduce, U=U, return_states=True, **_kw(p, window, st, prev, mu, discs, a0))
            tgd._same_bits(costs[p].cpu().numpy(), cost)
            best = orc.pick_best(cost)[0]
            assert int(keys[p].item()) == dsamp.pack_key(cost[best], offset + best)
            r = _capi.split_record(rec[p].cpu().numpy(), n)
            assert r["owner"] == 1.0 and r["n_feasible"] == np.count_nonzero(V == 0)
            tgd._same_bits(r["cost"], cost[best])
            tgd._same_bits(r["violation"], V[best])
            tgd._same_bits(r["u"], U[best])                             # the re-drawn COMMAND
            tgd._same_bits(r["x"], X[best])                             # the lagged trajectory
            # one softmin round: the mean is a mean of commands, weighted by the lagged costs (the oracle's reduction, to the
            # tolerance tests/test_gpu_dynamic_softmin.py holds the kernel to)
            np.testing.assert_allclose(mean[p].cpu().numpy(), sms.softmin_mean(orc, cost, U, lam), rtol=2e-5, atol=1e-6)
    finally:
        eng.close()


@pytest.mark.parametrize("n,N,window,integration,tier,terms,surface,K,reduce,given", [
    (20, 257, (2, 5), FINE, "loaded-coupled-downforce", True, True, 1, "mean", True),
    (20, 70, None, DEFAULT, "none", False, False, 3, "mean", False)])
def test_optimize_of_two_rounds_is_its_restatement(n, N, window, integration, tier, terms, surface, K, reduce, given):
    from acmpc_amd import _capi
    dps = tda.problems(n, N)
    setting, prev = (ALL_FOUR, tgt._previous(P, 53)) if terms else (OFF, None)
    rounds, shrink, seed = 2, 0.5, 1234
    eng = _handle(dps, N, n, window, K, reduce)
    try:
        _set(eng, tier, setting, prev, integration)
        mu, discs, a0 = _dress(eng, dps, n, 30 * n + N, surface, 0, given)
        centre, _ = tsf._centres(dps, n, 7)
        x0 = np.stack([d["x0"] for d in dps])
        out = eng.optimize(x0, centre, None, N, rounds, SIGMA, shrink=shrink, seed=seed)
        st = _settings(tier, setting, integration)
        for p in range(P):
            c = centre[p]
            for r, sig in enumerate(sms.round_sigmas(SIGMA, shrink, rounds)):
                U = dsamp.candidates(orc, dps[p], c, None, N, 0, p, r, seed, sig)
                cost, V, X = _spec(dps[p], eng.coefficients(p), K, reduce, U=U, return_states=True,
                                   **_kw(p, window, st, prev, mu, discs, a0))
                c = U[orc.pick_best(cost)[0]]
            tgd._check_record(_capi.split_record(out["records"][p], n), U, cost, V, X, n)
    finally:
        eng.close()


# ---- 2: the identities, on the device -------------------------------------------------------------------------------------------
def _all_forms(eng, dps, N, n):
    """solve in both layouts, the fused sampled rollout (costs and keys) and acmpc_optimize (its re-drawn records) of one handle."""
    import torch
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    centre, ref = tsf._centres(dps, n, 5)
    a, b = eng.solve(x0, U), eng.solve(x0, np.ascontiguousarray(U.transpose(0, 2, 3, 1)), layout=1)
    opt = eng.optimize(x0, centre, ref, N, 2, SIGMA, shrink=0.5, seed=31)["records"]
    dev, s = torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
    d_x0, d_c = torch.tensor(x0, device=dev), torch.tensor(centre, device=dev)
    costs, keys = torch.empty(P, N, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
    eng.rollout_sampled_device(d_x0.data_ptr(), d_c.data_ptr(), 2 * n, 0, P, N, n, tgc.BIG_OFFSET, SIGMA, 77, 1, costs.data_ptr(),
                               keys.data_ptr(), s)
    torch.cuda.synchronize()
    return [a["costs"], a["records"], b["costs"], b["records"], opt, costs.cpu().numpy(), keys.cpu().numpy()]


def _same_values(got, want, label):
    """`==` wherever the handle without the setting has a number, a NaN where it has one (the sign of a zero does not count)."""
    for q, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        if w.dtype != T:
            assert np.array_equal(g, w), (label, q)
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan], w[~nan]), (label, q)


@pytest.mark.parametrize("tier,K,reduce,integration,terms,surface,K_obs", [
    ("none", 1, "mean", DEFAULT, False, False, 0), ("loaded-coupled-downforce", 1, "mean", FINE, True, True, 2),
    ("none", 3, "max", FINE, True, True, 0), ("loaded-coupled-downforce", 3, "mean", DEFAULT, False, False, 2)])
def test_zero_time_constants_and_a_held_command_are_the_handle_without_the_setting(tier, K, reduce, integration, terms, surface, K_obs):
    n, N = 20, 257
    dps = tda.problems(n, N)
    setting, prev = (ALL_FOUR, tgt._previous(P, 54)) if terms else (OFF, None)
    held = np.array([0.04, 0.3], dtype=T)
    constant = [dict(d, U=np.tile(held, (N, n, 1))) for d in dps]
    eng = _handle(dps, N, n, (2, 5), K, reduce, softmin_lambda=0.5)
    try:
        _set(eng, tier, setting, prev, integration)
        mu, discs, a0 = _dress(eng, dps, n, 40, surface, K_obs, True)
        eng.set_dynamics_actuator(None)
        off = _all_forms(eng, dps, N, n)
        off_constant = eng.solve(np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in constant]))
        # (a): tau = (0, 0), from given positions and from cleared ones
        eng.set_dynamics_actuator((0.0, 0.0))
        _same_values(_all_forms(eng, dps, N, n), off, "tau 0, positions given")
        eng.set_actuator_state(None)
        _same_values(_all_forms(eng, dps, N, n), off, "tau 0, positions cleared")
        # (b): any tau, every plan holding the command the actuators are at
        eng.set_dynamics_actuator((0.5, 0.01))
        eng.set_actuator_state(np.tile(held, (P, 1)))
        got = eng.solve(np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in constant]))
        _same_values([got["costs"], got["records"]], [off_constant["costs"], off_constant["records"]], "held command")
        # the plain handle (no tier promoted), wherever that one's values are finite
        if not surface and tier == "none":
            plain = _handle(dps, N, n, (2, 5), K, reduce, softmin_lambda=0.5)
            try:
                _set(plain, tier, setting, prev, integration)
                if discs is not None:
                    plain.set_dynamics_clearance(40.0, 1.0)
                    plain.set_obstacles(np.stack([d[0] for d in discs]), np.stack([d[1] for d in discs]))
                want = _all_forms(plain, dps, N, n)
            finally:
                plain.close()
            eng.set_dynamics_actuator((0.0, 0.0))
            eng.set_actuator_state(a0)
            for q, (g, w) in enumerate(zip(_all_forms(eng, dps, N, n), want)):
                _same_where_finite(g, w, ("plain", q))
        # and the lag does something as soon as the command moves
        eng.set_dynamics_actuator(TAU)
        eng.set_actuator_state(a0)
        moved = _all_forms(eng, dps, N, n)
        assert not np.array_equal(_u32(moved[0]), _u32(off[0])) and not np.array_equal(_u32(moved[5]), _u32(off[5]))
    finally:
        eng.close()


# ---- 4: the plan trace ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,integration,tier,surface,K_obs,given", [(None, DEFAULT, "none", False, 0, True),
                                                                         ((2, 5), FINE, "loaded-coupled-downforce", True, 2, True),
                                                                         ((2, 5), FINE, "none", True, 0, False)])
def test_trace_plans_is_the_specification(window, integration, tier, surface, K_obs, given):
    from acmpc_amd import _capi
    n, N, K = 20, 70, 3
    dps = tda.problems(n, N)
    prev = tgt._previous(P, 55)
    eng = _handle(dps, N, n, window, K)
    try:
        _set(eng, tier, ALL_FOUR, prev, integration)
        mu, discs, a0 = _dress(eng, dps, n, 50, surface, K_obs, given)
        U = np.stack([d["U"][20:22] for d in dps])                       # M = 2 plans per problem
        x0 = np.stack([d["x0"] for d in dps])
        got = eng.trace_plans(x0, U)
        assert _capi.TRACE_TERM_FLOATS == 22 and got["terms"].shape == (P, 2, K, n, 22)
        s = _settings(tier, ALL_FOUR, integration, clearance=K_obs > 0)
        per = [das.trace_plans(dp, eng.coefficients(p), U[p], [v.coefficients() for v in _vehicles(K)], s, window, prev[p],
                               None if discs is None else discs[p], surface=None if mu is None else mu[p], actuator=TAU,
                               a0=None if a0 is None else a0[p]) for p, dp in enumerate(dps)]
        want = {name: np.stack([t[name] for t in per]) for name in ("states", "totals", "terms")}
        for name in ("states", "terms"):
            assert np.array_equal(ds.bits(got[name]), ds.bits(want[name])), name
        assert np.array_equal(ds.bits(np.stack([got["cost"], got["violation"]], axis=-1)), ds.bits(want["totals"]))
        assert np.array_equal(ds.bits(ds.replay(got["terms"])), ds.bits(got["terms"][..., ds.V_SLOT]))      # slots 5 .. 19 -> 20
        # slots 4 to 6 and 8 to 9 are on the command: the box's hinges from U alone, the rates' those of the handle without the lag
        lo, hi = (np.asarray(dps[0]["kw"][k], dtype=T) for k in ("u_min", "u_max"))
        for ch in range(2):
            box = U[..., ch] - np.fmin(np.fmax(U[..., ch], lo[ch]), hi[ch])
            assert np.array_equal(ds.bits(got["terms"][..., ds.BOX + ch]), ds.bits(np.broadcast_to(box[:, :, None], (P, 2, K, n))))
        eng.set_dynamics_actuator(None)
        off = eng.trace_plans(x0, U)
        assert np.array_equal(ds.bits(off["terms"][..., ds.RATE:ds.RATE + 2]), ds.bits(got["terms"][..., ds.RATE:ds.RATE + 2]))
        assert not np.array_equal(ds.bits(off["states"][..., 1:, :]), ds.bits(got["states"][..., 1:, :]))
        # and the totals are the rollout's costs of the same plans under vehicle 0 ... (an ensemble's solve combines the K)
    finally:
        eng.close()


# ---- 6: a steering step through a lagging rack, on the device -------------------------------------------------------------------
def test_a_steering_step_reaches_less_yaw_through_a_lagging_rack():
    dp, coef, U, a0 = tda.steering_step_problem()
    n = tda.STEER_STEPS
    eng = tgd._engine([dp], 1, 4, n)
    try:
        yaws = []
        for tau in ((tda.STEER_TAU, 0.0), (0.0, 0.0)):
            eng.set_dynamics_actuator(tau)
            eng.set_actuator_state(a0)
            got = eng.trace_plans(dp["x0"][None], U)
            trace = {}
            das.spec_costs(orc, dp, eng.coefficients(0), _vehicle().coefficients(), U=U, actuator=tau, a0=a0, trace=trace)
            assert np.array_equal(ds.bits(got["states"][0, 0, 0]), ds.bits(trace["states"][0]))
            yaws.append(float(got["states"][0, 0, 0, -1, 2]))
        assert 0.0 < yaws[0] < yaws[1]
        (lag64, _), (now64, _) = tda._steering_yaws()
        assert abs(yaws[0] - lag64) < 1e-4 and abs(yaws[1] - now64) < 1e-4
    finally:
        eng.close()


# ---- 5: positions for another P -------------------------------------------------------------------------------------------------
def test_positions_for_another_P_are_refused_and_the_handle_stays_usable():
    from acmpc_amd import EngineError
    n, N = 20, 70
    dps = tda.problems(n, N)
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    centre, ref = tsf._centres(dps, n, 5)
    a0 = tda.positions(P, 63)
    eng = tgd._engine(dps, P, N, n, (2, 5))
    try:
        eng.set_dynamics_actuator(TAU)
        eng.set_actuator_state(a0)
        want = eng.solve(x0, U)
        eng.set_actuator_state(a0[:1])
        for call in (lambda: eng.solve(x0, U), lambda: eng.optimize(x0, centre, ref, N, 2, SIGMA, shrink=0.5, seed=31),
                     lambda: eng.trace_plans(x0, U[:, :2])):
            with pytest.raises(EngineError) as e:
                call()
            assert e.value.code == ESTATE and "acmpc_set_actuator_state" in str(e.value)
        with pytest.raises(EngineError) as e:
            eng.set_dynamics_actuator((0.1, float("nan")))
        assert e.value.code == EINVAL
        eng.set_actuator_state(a0)
        again = eng.solve(x0, U)
        assert np.array_equal(_u32(again["costs"]), _u32(want["costs"])) and np.array_equal(_u32(again["records"]), _u32(want["records"]))
        # off again: the bits of a handle that never had the setting, the positions still set
        eng.set_dynamics_actuator(None)
        never = tgd._engine(dps, P, N, n, (2, 5))
        try:
            assert np.array_equal(_u32(eng.solve(x0, U)["costs"]), _u32(never.solve(x0, U)["costs"]))
        finally:
            never.close()
    finally:
        eng.close()


# ---- 7: the solver and the controller -------------------------------------------------------------------------------------------
SOLVER = dict(horizon=13, n_candidates=2048, sampling_rounds=2, sampling_sigma=(0.02, 0.3), sampling_seed=11, progress_cost=3.0,
              r_term=(0.0, 10.0), tyre_coupling=(1.0, 1.0), plan_states=True, actuator_lag=(0.1, 0.05))


def test_dynamic_sampling_solver_takes_an_actuator_lag_and_keeps_its_own_estimate():
    from acmpc_amd import dynamic_model as dm
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    n = SOLVER["horizon"] - 1
    dp = tda.problems(n, 70)[1]
    table, state = dp["table"], dp["x0"].astype(np.float64)
    solver, plain = DynamicSamplingSolver(SOLVER), DynamicSamplingSolver({k: v for k, v in SOLVER.items() if k != "actuator_lag"})
    try:
        sent = []
        first = solver.solve(state, table)
        assert first.info.status == "solved" and solver.actuator_state is None      # nothing measured, nothing sent yet
        sent.append(first.x[3 * (n + 1):].reshape(n, 2)[0])
        second = solver.solve(state, table)
        assert second.info.status == "solved"
        # the estimate the second solve started from: the response to the control the first one returned
        assert np.array_equal(solver.actuator_state, dm.actuator_response(np.array(sent), None, SOLVER["actuator_lag"], 0.05)[1][-1])
        sent.append(second.x[3 * (n + 1):].reshape(n, 2)[0])
        third = solver.solve(state, table)
        assert third.info.status == "solved"
        want = dm.actuator_response(np.array(sent), None, SOLVER["actuator_lag"], 0.05)[1][-1]
        assert np.array_equal(solver.actuator_state, want)
        # trace() carries the lag and the positions: the float64 mirror from the same positions gives the same trajectory
        traced = solver.trace()
        plan = third.x[3 * (n + 1):].reshape(n, 2)
        mirror = dm.trace(_vehicle(), state, plan, table[:, :n], dt=0.05, coupling=(1.0, 1.0), actuator=(SOLVER["actuator_lag"], want))
        assert np.max(np.abs(traced["states"][0] - mirror["states"])) < 1e-3
        assert np.array_equal(third.states, traced["states"][0].astype(np.float64))
        # a measured position takes the estimate's place
        solver.solve(state, table, actuator_state=(0.05, 0.2))
        assert np.array_equal(solver.actuator_state, np.array([0.05, 0.2]))
        # and the setting changes the plan's trajectory
        other = plain.solve(state, table)
        assert other.info.status == "solved" and not np.array_equal(other.states, first.states)
    finally:
        solver.close()
        plain.close()


def test_the_controller_in_mode_d_runs_get_control_with_the_key():
    """Four ticks along test_gpu_dynamic's circuit with `actuator_lag` in the control config: get_control's plan is the plan of a
    DynamicSamplingSolver of the same config called directly (both keep their own estimate of the positions), bit for bit."""
    import test_gpu_dynamic_controller as tgk
    from acmpc_amd import DynamicBicycleParams, DynamicSamplingSolver, workloads
    from acmpc_amd.mpc import build_mpc
    lag = (0.1, 0.05)
    plant = DynamicBicycleParams.reference()
    cfg = dict(tgd.LOOP_CONFIG, actuator_lag=lag)
    mpc = build_mpc(dict(cfg, rollout_mode="D", speed_profile_constraints=dict(tgk.CONSTRAINTS)), workloads.PlaceholderVehicle())
    direct = DynamicSamplingSolver(dict(cfg, plan_states=True), plant)
    try:
        centre, v_profile, heading, state = tgk._start()
        n = tgd.LOOP_H - 1
        for tick in range(4):
            mpc.get_control(tgk._window(centre, state), motion=state[3:])
            assert mpc.infeasibility_counter == 0, tick
            obj = direct.solve(np.array([0.0, 0.0, np.pi / 2, *state[3:]]), mpc.reference_path.table)
            u = obj.x[3 * (n + 1):].reshape(n, 2)
            np.testing.assert_array_equal(mpc.projected_control[1], u[:, 0])
            np.testing.assert_array_equal(mpc.projected_pedal, u[:, 1])
            np.testing.assert_array_equal(mpc.plan_states, obj.states)
            steering, pedal, _ = tgk._command(mpc)
            state = plant.predict_next_state(state, (steering, pedal), tgd.LOOP_DT)[0]
            state[3] = max(state[3], 0.0)
        inner = mpc._control_solver.dynamic_solver
        assert inner.actuator_state is not None and np.array_equal(inner.actuator_state, direct.actuator_state)
    finally:
        direct.close()
        mpc._control_solver.dynamic_solver.close()
