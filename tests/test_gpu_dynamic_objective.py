"""Mode D's objective (acmpc_set_dynamics_objective) on the MI355X, from every call form.  Costs, keys, feasible counts and
records must be bit-identical to tests/dynamic_spec.py - alone on the small shapes, and through the forms already
held to it (the one-candidate-per-lane kernels, the control matrix) on the large ones - with costs that are negative; a
handle whose objective is off must give the bits of a handle that never heard of the call; and DynamicSamplingSolver with a
progress reward under a ceiling from the speed profile covers more of the loop of test_gpu_dynamic than the same solver
tracking that profile, inside the corridor, the slip limit and the ceiling."""
import dataclasses

import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_ensemble_spec as es
import dynamic_sampled_spec as dss
import dynamic_spec as ds
from dynamic_spec import Settings
import test_gpu_dynamic as tgd
import test_gpu_dynamic_ensemble as tge
import test_gpu_dynamic_packed as tpk
import test_gpu_dynamic_sampled as tsm
import test_gpu_dynamic_softmin as tsf
import test_gpu_dynamic_terms as tgt
from acmpc_oracle import fma32

pytestmark = pytest.mark.gpu

T = np.float32
DEFAULT, FINE = tgt.DEFAULT, tgt.FINE
BIG_OFFSET = tsm.BIG_OFFSET
NO_TERMS = dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=None)
# progress: 400 per metre outweighs every stage cost of a candidate that moves - most costs are negative; ceiling: the
# path's own speed plus 0.3 m/s, which the candidates with a pedal above the mild ones break; both: a ceiling 5 % above
SETTINGS = {
    "progress": (dict(progress_weight=400.0, speed_ceiling=None), NO_TERMS),
    "ceiling": (dict(progress_weight=0.0, speed_ceiling=(1.0, 0.3)), NO_TERMS),
    "both": (dict(progress_weight=3.0, speed_ceiling=(1.05, 0.0)), NO_TERMS),
    "both+terms": (dict(progress_weight=3.0, speed_ceiling=(1.05, 0.0)), tgt.BOTH),
}
BOTH = SETTINGS["both+terms"]
NEGATIVE = dict(progress_weight=400.0, speed_ceiling=None)
# an ensemble of three grips under MEAN (test_gpu_dynamic_sampled's K = 3 holds the reference's literal block, whose costs are
# huge or non-finite: no set of negative costs)
GRIPS3 = dict(vehicles=(0, 1, 2), weights=(1.0, 2.0, 0.5), reduce="mean")


def _vehicle():
    from acmpc_amd import DynamicBicycleParams
    return DynamicBicycleParams.reference()


def _set(eng, objective, terms, u_prev=None):
    eng.set_dynamics_objective(**objective)
    eng.set_dynamics_terms(**terms)
    eng.set_previous_control(u_prev)


# ---- one candidate per lane ---------------------------------------------------------------------------------------------
# P = 2, N = 300 (one full 256-lane workgroup and a tail), n = 12.  Layout 0 starts its problems at a standstill and at the
# path's speed, layout 1 above the ceiling (1.3 x the path's speed) and at the path's speed.  A NaN pedal, an inf steering.
@pytest.mark.parametrize("integration", [DEFAULT, FINE], ids=["euler", "M3-blend"])
@pytest.mark.parametrize("layout,window", [(0, None), (1, (2, 5)), (1, None), (0, (2, 5))])
def test_costs_argmin_and_record_are_the_specification(layout, window, integration):
    from acmpc_amd import _capi
    P, N, n = 2, 300, 12
    first = ds.make_dynamic_problem(orc, "monza", n + 1, N, 1700)
    over = 1.3 * float(first["table"][orc.ROW_V][0])
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 1700 + p, vx0=v) for p, v in enumerate(((0.0, over)[layout], None))]
    dps[0]["U"][5, n // 2, 1] = np.nan
    dps[1]["U"][7, 0, 0] = np.inf
    u_prev = tgt._previous(P, 11)
    eng = tgd._engine(dps, P, N, n, window)
    try:
        eng.set_dynamics_integration(*integration)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        x0 = np.stack([d["x0"] for d in dps])
        negative = {}
        for name, (objective, terms) in SETTINGS.items():
            _set(eng, objective, terms, u_prev)
            out = eng.solve(x0, U_in, layout=layout)
            for p in range(P):
                trace = {}
                cost, V, X = ds.spec_costs(orc, dps[p], eng.coefficients(p), _vehicle().coefficients(), nn_window=window,
                                           return_states=True, settings=Settings(*integration, **objective, **terms),
                                           u_prev=u_prev[p], trace=trace)
                label = "%s, problem %d" % (name, p)
                tgd._same_bits(out["costs"][p], cost)
                rec = _capi.split_record(out["records"][p], n)
                best = tgd._check_record(rec, U_h[p], cost, V, X, n)
                assert out["best_idx"][p] == best, label
                assert out["n_feasible"][p] == np.count_nonzero(V == 0), label
                tgd._same_bits(rec["cost"], out["costs"][p][best])      # the finalize's re-roll gives the rollout's own cost
                negative[name, p] = float(np.mean(cost < 0))
                if name == "ceiling" and layout == 1 and p == 0:        # above the cap at step 0: every candidate
                    assert np.all(trace["over"][np.isfinite(cost), 0] > 0) and out["n_feasible"][p] == 0, label
            assert np.isnan(out["costs"][0][5]) and not np.isfinite(out["costs"][1][7])
        # most costs of the problem at the path's speed are negative under the large weight, and its winner's is
        assert negative["progress", 1] > 0.5 and negative["ceiling", 1] == 0.0, negative
        _set(eng, *SETTINGS["progress"], u_prev)
        assert eng.solve(x0, U_in, layout=layout)["records"][1][0] < 0
    finally:
        eng.close()


def test_candidates_past_the_paths_end():
    """A start beside the last waypoint but one, along the path at 45 m/s (27 m in 12 steps, the waypoints 12.5 m apart),
    exhaustive search: j stays at n - 1 and s keeps growing linearly, beyond the last waypoint's arc length."""
    from acmpc_amd import _capi
    P, N, n = 1, 130, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 1710, vx0=45.0)]
    dps[0]["x0"][:3] = dps[0]["table"][:3, n - 2]
    objective = dict(progress_weight=3.0, speed_ceiling=(1.05, 0.0))
    eng = tgd._engine(dps, P, N, n, None)
    try:
        eng.set_dynamics_objective(**objective)
        out = eng.solve(np.stack([d["x0"] for d in dps]), dps[0]["U"][None])
        trace = {}
        cost, V, X = ds.spec_costs(orc, dps[0], eng.coefficients(0), _vehicle().coefficients(), return_states=True,
                                   settings=Settings(*DEFAULT, **objective, **NO_TERMS), trace=trace)
        coef = eng.coefficients(0)
        length = float(np.sum(np.hypot(np.diff(coef[:, 0].astype(np.float64)), np.diff(coef[:, 1].astype(np.float64)))))
        past = (trace["j"][:, -1] == n - 1) & (trace["s"] > length + 5.0)
        assert past.sum() > N // 2, (past.sum(), length, float(np.nanmax(trace["s"])))
        tgd._same_bits(out["costs"][0], cost)
        tgd._check_record(_capi.split_record(out["records"][0], n), dps[0]["U"], cost, V, X, n)
    finally:
        eng.close()


# ---- ensembles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integration", [DEFAULT, FINE], ids=["euler", "M3-blend"])
@pytest.mark.parametrize("reduce,layout,window", [("mean", 0, None), ("max", 1, (2, 5))])
def test_ensemble_is_the_specification(reduce, layout, window, integration):
    """K = 3: two grips and a longer car; every vehicle carries both parts with its own end state."""
    from acmpc_amd import _capi
    P, N, n = 2, 300, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 1720 + p, vx0=v) for p, v in enumerate((0.0, None))]
    dps[0]["U"][5, n // 2, 1] = np.nan
    vehicles = [_vehicle(), dataclasses.replace(_vehicle(), lf=1.9, lr=1.1).with_grip(0.6), _vehicle().with_grip(1.3)]
    blocks = [v.coefficients() for v in vehicles]
    weights = (1.0, 2.0, 0.5) if reduce == "mean" else None
    u_prev = tgt._previous(P, 13)
    eng = tge._engine(dps, P, N, n, window)
    try:
        _set(eng, *BOTH, u_prev)                  # before the vehicles: the setting does not depend on them
        eng.set_dynamics_ensemble(vehicles, weights=weights, reduce=reduce)
        eng.set_dynamics_integration(*integration)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        out = eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)
        for p in range(P):
            J, V, X = es.spec_ensemble(orc, dps[p], eng.coefficients(p), blocks, reduce=reduce, weights=weights, nn_window=window,
                                       return_states=True, settings=Settings(*integration, **BOTH[0], **BOTH[1]), u_prev=u_prev[p])
            tgd._same_bits(out["costs"][p], J)
            best = tgd._check_record(_capi.split_record(out["records"][p], n), U_h[p], J, V, X, n)
            assert out["best_idx"][p] == best
            alone = ds.spec_costs(orc, dps[p], eng.coefficients(p), blocks[1], nn_window=window, settings=Settings(*integration,
                                  **BOTH[0], **BOTH[1]), u_prev=u_prev[p])[0]
            assert not np.array_equal(alone.view(np.uint32), J.view(np.uint32))
    finally:
        eng.close()


def test_ensemble_of_one_is_the_single_vehicle():
    P, N, n = 2, 300, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 1740 + p, vx0=v) for p, v in enumerate((1.0, None))]
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    eng = tge._engine(dps, P, N, n, (2, 5))
    try:
        _set(eng, *BOTH, tgt._previous(P, 14))
        eng.set_dynamics(_vehicle())
        single = eng.solve(x0, U)
        eng.set_dynamics_ensemble([_vehicle()], reduce="mean")
        one = eng.solve(x0, U)
        assert np.array_equal(one["costs"].view(np.uint32), single["costs"].view(np.uint32))
        assert np.array_equal(one["records"].view(np.uint32), single["records"].view(np.uint32))
        eng.set_dynamics_objective()
        assert not np.array_equal(eng.solve(x0, U)["costs"].view(np.uint32), single["costs"].view(np.uint32))
    finally:
        eng.close()


# ---- the sampled forms and acmpc_optimize -----------------------------------------------------------------------------------
def _rig(P, N, n, K, window, seed, integration, setting=BOTH, **kw):
    rig = tsm.Rig(P, N, n, K=K, window=window, seed=seed, **kw)
    rig.u_prev = tgt._previous(P, seed)
    rig.eng.set_dynamics_integration(*integration)
    _set(rig.eng, *setting, rig.u_prev)
    return rig


@pytest.mark.parametrize("P,N,n,K,window,with_ref,rnd,offset,integration", [
    (3, 1537, 30, 1, (2, 5), True, 2, 0, DEFAULT),
    (1, 1000, 49, 1, None, False, 1, BIG_OFFSET, FINE),
    (3, 300, 49, 3, (2, 5), True, 0, BIG_OFFSET, DEFAULT),
    (1, 131, 8, 4, None, True, 1, 0, FINE),
])
def test_fused_rollout_equals_sample_then_rollout(P, N, n, K, window, with_ref, rnd, offset, integration):
    """acmpc_rollout_sampled_device and the re-drawing finalize against their matrix forms: the sampled kernels hand the last
    step's nearest waypoint to the finish through the terms' state, the matrix kernels hold it themselves."""
    rig = _rig(P, N, n, K, window, 1800 + n, integration, with_ref=with_ref, kinds=[(1, 0, 3)[p % 3] for p in range(P)])
    try:
        sigma, seed = (0.04, 0.35), 0xC0FFEE1234
        U, costs, keys = tsm._compare_rollouts(rig, N, offset, sigma, seed, rnd)
        tsm._compare_records(rig, U, keys, N, offset, sigma, seed, rnd)
    finally:
        rig.close()


@pytest.mark.parametrize("K", [1, 3])
def test_fused_rollout_and_optimize_equal_the_specification(K):
    """96 x 12 against the restatements alone: the fused rollout's costs, key and count, the re-drawn record, and
    acmpc_optimize's argmin rounds."""
    from acmpc_amd import _capi
    P, N, n, sigma, seed, rnd, window = 2, 96, 12, (0.05, 0.3), 99, 3, (2, 5)
    rig = _rig(P, N, n, K, window, 1840, FINE, with_ref=True, kinds=[1, 0])
    try:
        for offset in (0, BIG_OFFSET):
            costs, keys = rig.fused(N, offset, sigma, seed, rnd)
            rec = rig.finalize_sampled(None, N, sigma, seed, rnd)
            for p in range(P):
                want = dss.rollout_sampled(orc, rig.dps[p], rig.eng.coefficients(p), rig.blocks(), rig.centre_h[p], rig.ref_h[p],
                                           N, offset, p, rnd, seed, sigma, reduce=rig.reduce, weights=rig.weights,
                                           nn_window=window, return_states=True, settings=Settings(*FINE, **BOTH[0], **BOTH[1]),
                                           u_prev=rig.u_prev[p])
                tsm._same_bits(costs[p].cpu().numpy(), want["cost"], "costs, problem %d" % p)
                assert int(keys[p].item()) == want["key"]
                r, best = _capi.split_record(rec[p], n), want["best"]
                assert r["owner"] == 1.0 and r["n_feasible"] == want["n_feasible"]
                for name, value in (("cost", want["cost"][best]), ("violation", want["violation"][best]),
                                    ("u", want["U"][best]), ("x", want["x"][best])):
                    tsm._same_bits(r[name], value)
        rounds, shrink = 2, 0.5
        got = rig.eng.optimize(rig.x0_h, rig.centre_h, None, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        for p in range(P):
            centre = rig.centre_h[p]
            for r in range(rounds):
                sig = (sigma[0] * shrink**r, sigma[1] * shrink**r)
                U = dss.candidates(orc, rig.dps[p], centre, None, N, 0, p, r, seed, sig)
                cost, V, X = dss.costs(orc, rig.dps[p], rig.eng.coefficients(p), rig.blocks(), U, rig.reduce, rig.weights, window,
                                       return_states=True, settings=Settings(*FINE, **BOTH[0], **BOTH[1]), u_prev=rig.u_prev[p])
                centre = U[orc.pick_best(cost)[0]]
            tgd._check_record(_capi.split_record(got[p], n), U, cost, V, X, n)
    finally:
        rig.close()


@pytest.mark.parametrize("K", [1, 3])
def test_softmin_mean_over_negative_costs_is_the_matrix_form(K):
    """Every cost of the fused rollout negative (problems at their path's speed, 400 per metre, a steering spread of 3 mrad
    that keeps every candidate in the corridor): the mean of
    acmpc_softmin_sampled_device is that of acmpc_sample_device + acmpc_softmin_device on the same costs and keys, bit for
    bit, its weights exp(-(cost - min) / lambda) with a negative min: the winner's is 1, none above."""
    P, N, n, sigma, seed, rnd = 2, 1025, 30, (0.003, 0.3), 77, 1
    rig = _rig(P, N, n, K, (2, 5), 1850, DEFAULT, setting=(NEGATIVE, NO_TERMS), with_ref=True, kinds=[0, 3],
               **(GRIPS3 if K == 3 else {}))
    try:
        for offset in (0, tsf.BIG_OFFSET):
            costs, keys = rig.fused(N, offset, sigma, seed, rnd)
            c = costs.cpu().numpy()
            assert np.all(c < 0) and np.all(np.isfinite(c))
            from acmpc_amd import _capi
            for p in range(P):
                k = int(keys[p].item())
                assert _capi.key_cost(k) == float(c[p].min()) and _capi.key_index(k) - offset == int(np.argmin(c[p]))
            got, want = tsf._both_forms(rig.torch, rig.eng, rig.dev, rig.s, costs, keys, rig.centre, rig.ref, P, N, n, offset,
                                        sigma, seed, rnd)
            assert np.array_equal(tsf._u32(got[0]), tsf._u32(want[0])), "mean, offset %d" % offset
            assert np.array_equal(tsf._u64(got[1]), tsf._u64(want[1])), "weight sum, offset %d" % offset
            wsum = got[1].cpu().numpy()
            assert np.all(wsum >= 1.0) and np.all(wsum <= N) and np.all(np.isfinite(got[0].cpu().numpy()))
    finally:
        rig.close()


@pytest.mark.parametrize("update", ["argmin", "softmin"])
@pytest.mark.parametrize("vehicles", [None, (0, 1, 2)], ids=["K1", "K3"])
def test_optimize_with_and_without_the_matrix_and_the_sharded_optimizer(vehicles, update):
    """Rounds 2, both centre updates, winners with negative costs: the default rounds (no control matrix) against
    ACMPC_DYNAMIC_MATRIX_ROUNDS=1, bit for bit, and ShardedOptimizer at world size 1 against both."""
    import torch
    from acmpc_amd.sharding import ShardedOptimizer
    P, N, n, rounds, sigma, shrink, seed = 2, 1025, 30, 2, (0.05, 0.3), 0.5, 1234
    eng, dps = tsf._dynamic_engine(P, N, n, seed=1860, vehicles=vehicles, window=(2, 5), centre_update=update,
                                   softmin_lambda=0.5)
    try:
        centre, ref = tsf._centres(dps, n, 3)
        x0 = np.stack([d["x0"] for d in dps])
        plain = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        eng.set_dynamics_objective(progress_weight=400.0, speed_ceiling=(1.5, 0.0))   # (a ceiling no plan of 1.5 s reaches)
        default = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        assert not np.array_equal(plain.view(np.uint32), default.view(np.uint32))   # (the objective reaches these rounds)
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", "1")
        matrix = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", None)
        tsm._same_bits(default, matrix, "the rounds without a matrix against the rounds through it")
        assert np.all(default[:, 3] == 1.0) and np.all(default[:, 0] < 0) and np.all(default[:, 1] == 0)
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream().cuda_stream
        opt = ShardedOptimizer(eng, P, N, n, 0, dev, centre_update=update)
        rec = opt.solve(torch.tensor(x0, device=dev), torch.tensor(centre, device=dev), torch.tensor(ref, device=dev), rounds,
                        sigma, shrink=shrink, seed=seed, stream=s)
        torch.cuda.synchronize()
        tsm._same_bits(rec.cpu().numpy(), matrix, "ShardedOptimizer at world size 1")
    finally:
        eng.close()


@pytest.mark.parametrize("K", [1, 3])
def test_four_ranks_at_large_odd_offsets_end_with_the_unsharded_record(K):
    """test_gpu_dynamic_sampled's four emulated ranks, the launch's first candidate at a large odd global index: every
    rank's handle carries the same objective; the reduced keys are negative."""
    import torch
    from acmpc_amd import _capi
    from acmpc_amd.sharding import shard_range
    P, N, n, sigma, seed, rnd, base = 3, 1030, 30, (0.05, 0.3), 4242, 1, BIG_OFFSET
    setting = (dict(progress_weight=400.0, speed_ceiling=(1.5, 0.0)), NO_TERMS)
    rig = _rig(P, N, n, K, (2, 5), 1880, DEFAULT, setting=setting, with_ref=True, kinds=[0, 3, 2], **(GRIPS3 if K == 3 else {}))
    try:
        U, costs, keys = tsm._compare_rollouts(rig, N, base, sigma, seed, rnd)
        whole = tsm._compare_records(rig, U, keys, N, base, sigma, seed, rnd)
        slices = [shard_range(N, r, 4) for r in range(4)]
        shard_keys, shard_costs = [], []
        for off, count in slices:
            c, k = rig.fused(count, base + off, sigma, seed, rnd)
            shard_keys.append(k.cpu().numpy())
            shard_costs.append(c.cpu().numpy())
        tsm._same_bits(np.concatenate(shard_costs, axis=1), costs.cpu().numpy())
        reduced_h = np.minimum.reduce(shard_keys)                 # the all-reduce(MIN) of signed keys, on the host
        assert np.array_equal(reduced_h, keys.cpu().numpy()) and np.all(reduced_h < 0)
        reduced = torch.tensor(reduced_h, device=rig.dev)
        recs = []
        for off, count in slices:
            rig.fused(count, base + off, sigma, seed, rnd, want_costs=False, want_keys=False)
            recs.append(rig.finalize_sampled(reduced, count, sigma, seed, rnd))
        for p in range(P):
            assert base <= _capi.key_index(int(reduced_h[p])) < base + N
            assert whole[p][0] < 0 and _capi.key_cost(int(reduced_h[p])) == float(whole[p][0])
            for rec in recs:
                assert rec[p][3] == 1.0
                tsm._same_bits(np.delete(rec[p], 2), np.delete(whole[p], 2), "problem %d" % p)
            assert sum(float(rec[p][2]) for rec in recs) == float(whole[p][2])
    finally:
        rig.close()


# ---- two candidates per lane ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,layout,window,integration", [(1, 1, (2, 5), DEFAULT), (2, 0, None, FINE)])
def test_packed_rollout(K, layout, window, integration):
    """The smallest launch with P N K >= 2^20 at n = 4 with an odd N: the f32x2 step loop with all four parts.  In full
    against the one-candidate-per-lane kernels - two shards of candidates by index_offset, each below 2^20 - and against the
    specification on test_gpu_dynamic_packed's subset."""
    import torch
    from acmpc_amd import _capi
    N, n = 4099, 4
    P = tpk._problems_for(N, K)
    half = (N + 1) // 2
    assert P * N * K >= tpk.PACKED and P * half * K < tpk.PACKED
    label = "K %d layout %d window %s P %d" % (K, layout, window, P)
    base, U, x0, tables = tpk._make(P, N, n, seed=1900 + K)
    x0[2::4, 3] = 4.0
    planted = tpk._plant(U, N, n)
    by_kind = tgt._previous(4, 16)
    u_prev = by_kind[np.arange(P) % 4]
    vehicles = [_vehicle()] if K == 1 else [_vehicle(), dataclasses.replace(_vehicle(), lf=1.9, lr=1.1).with_grip(0.6)]
    eng = tge._engine([base[p % 4] for p in range(P)], P, N, n, window)
    try:
        eng.set_dynamics_integration(*integration)
        _set(eng, *BOTH, u_prev)
        if K == 1:
            eng.set_dynamics(vehicles[0])
        else:
            eng.set_dynamics_ensemble(vehicles, reduce="mean")
        U_in = tpk._as_layout(U, layout)
        whole = eng.solve(x0, U_in, layout=layout)
        coefs = [eng.coefficients(q) for q in range(4)]
        blocks = [v.coefficients() for v in vehicles]

        def spec(q, U_sub, states):
            dp = dict(base[q], x0=x0[q])
            if K == 1:
                return ds.spec_costs(orc, dp, coefs[q], blocks[0], nn_window=window, U=U_sub, return_states=states,
                                     settings=Settings(*integration, **BOTH[0], **BOTH[1]), u_prev=by_kind[q])
            return es.spec_ensemble(orc, dp, coefs[q], blocks, reduce="mean", nn_window=window, U=U_sub, return_states=states,
                                    settings=Settings(*integration, **BOTH[0], **BOTH[1]), u_prev=by_kind[q])

        tpk._check_against_spec(whole, base, coefs, U, N, n, tpk.GROUP_ONE if K == 1 else tpk.GROUP_ENSEMBLE, planted, spec,
                                37 + K, label)
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream().cuda_stream
        rf = _capi.record_floats(n)
        d_x0 = torch.tensor(x0, device=dev)
        parts = []
        for lo, hi in ((0, half), (half, N)):
            d_U = torch.tensor(tpk._as_layout(U[:, lo:hi], layout), device=dev)
            parts.append((lo, hi - lo, d_U, torch.empty(P, hi - lo, device=dev), torch.empty(P, dtype=torch.int64, device=dev)))
        for lo, count, d_U, cs, ks in parts:
            eng.rollout_device(d_x0.data_ptr(), d_U.data_ptr(), P, count, n, layout, lo, cs.data_ptr(), ks.data_ptr(), s)
        torch.cuda.synchronize()
        tgd._same_bits(np.concatenate([parts[0][3].cpu().numpy(), parts[1][3].cpu().numpy()], axis=1), whole["costs"])
        combined = torch.minimum(parts[0][4], parts[1][4])
        assert [_capi.key_index(int(k)) for k in combined.cpu().numpy()] == list(whole["best_idx"]), label
        records = []
        for lo, count, d_U, cs, ks in parts:
            r = torch.empty(P, rf, device=dev)
            eng.rollout_device(d_x0.data_ptr(), d_U.data_ptr(), P, count, n, layout, lo, cs.data_ptr(), 0, s)
            eng.finalize_device(combined.data_ptr(), d_x0.data_ptr(), d_U.data_ptr(), P, count, n, layout, lo, r.data_ptr(), s)
            records.append(r)
        torch.cuda.synchronize()
        r0, r1 = (r.cpu().numpy() for r in records)
        for p in range(P):
            owner, other = (r0[p], r1[p]) if r0[p][3] == 1.0 else (r1[p], r0[p])
            assert owner[3] == 1.0 and other[3] == 0.0, "%s: problem %d" % (label, p)
            assert owner[2] + other[2] == whole["records"][p][2], "%s: problem %d" % (label, p)
            assert np.array_equal(np.delete(owner, 2).view(np.uint32), np.delete(whole["records"][p], 2).view(np.uint32)), \
                "%s: problem %d" % (label, p)
    finally:
        eng.close()


# ---- handle hygiene ---------------------------------------------------------------------------------------------------------
def test_objective_off_is_a_handle_that_never_made_the_call():
    """(0, NULL); set then switched off; set then refused: costs, records and acmpc_optimize's records of a handle that never
    called - alone and beside rate and slip terms, whose kernels are then the ones that ran before.  And the setting survives
    acmpc_set_dynamics, _ensemble, _integration and _terms."""
    P, N, n = 2, 700, 30
    dps = tgd._problems(P, N, n, seed=1910)
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    centre = np.tile(np.stack([np.zeros(n), np.full(n, 0.2)], axis=1).astype(T), (P, 1, 1))
    objective = dict(progress_weight=3.0, speed_ceiling=(1.05, 0.0))

    def run(prepare):
        eng = tgd._engine(dps, P, N, n, (2, 5))
        try:
            prepare(eng)
            out = eng.solve(x0, U)
            opt = eng.optimize(x0, centre, None, N, 2, (0.05, 0.3), shrink=0.5, seed=77)
            return out["costs"], out["records"], opt["records"]
        finally:
            eng.close()

    def differs(eng, want):
        return not np.array_equal(eng.solve(x0, U)["costs"].view(np.uint32), want.view(np.uint32))

    def explicit_off(eng):
        assert eng._lib.acmpc_set_dynamics_objective(eng._ctx, 0.0, None) == 0

    def there_and_back(eng):
        eng.set_dynamics_objective(**objective)
        assert differs(eng, never[0])
        eng.set_dynamics_objective()

    def refused(eng):
        c = np.array([-1.0, 0.0])
        assert eng._lib.acmpc_set_dynamics_objective(eng._ctx, 1.0, c.ctypes.data) == -1
        assert eng._lib.acmpc_set_dynamics_objective(eng._ctx, -1.0, None) == -1

    never = run(lambda eng: None)
    for prepare in (explicit_off, there_and_back, refused):
        for got, want in zip(run(prepare), never):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), prepare.__name__

    # beside the terms: off again is the handle with the terms alone
    def terms_only(eng):
        eng.set_dynamics_terms(**tgt.BOTH)

    def terms_and_back(eng):
        eng.set_dynamics_terms(**tgt.BOTH)
        eng.set_dynamics_objective(**objective)
        assert differs(eng, termed[0])
        eng.set_dynamics_objective(0.0, None)

    termed = run(terms_only)
    for got, want in zip(run(terms_and_back), termed):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

    # the setting survives a change of vehicle(s), of the integration setting and of the terms
    def survives(eng):
        eng.set_dynamics_objective(**objective)
        eng.set_dynamics_integration(*FINE)
        eng.set_dynamics_ensemble([_vehicle(), _vehicle().with_grip(0.6)])
        eng.set_dynamics(_vehicle())
        eng.set_dynamics_terms(**tgt.BOTH)
        eng.set_dynamics_terms()
        eng.set_dynamics_integration(1, None)

    want = run(lambda eng: eng.set_dynamics_objective(**objective))
    assert not np.array_equal(want[0].view(np.uint32), never[0].view(np.uint32))
    for got, w in zip(run(survives), want):
        assert np.array_equal(got.view(np.uint32), w.view(np.uint32))
    for p in range(P):   # (and that is the specification's)
        cost = ds.spec_costs(orc, dps[p], orc.coefficients_temporal(dps[p]["table"], dps[p]["kw"]["margin"]).astype(T),
                             _vehicle().coefficients(), nn_window=(2, 5), settings=Settings(*DEFAULT, **objective, **NO_TERMS))[0]
        tgd._same_bits(want[0][p], cost)


# ---- closed loop ------------------------------------------------------------------------------------------------------------
# The loop of test_gpu_dynamic_terms (200 ticks, 4 096 candidates, through the tightest corner), twice: A tracks the speed
# profile (its config with the terms), B is told to make progress instead.  B's keys:
#   r_term = (0, 10)        the speed error is no longer a cost
#   speed_ceiling = 1.1     the profile allows 8 m/s^2 of lateral acceleration (6.8 at its 34 m/s cap) and the tyres give about
#                           11.4: sqrt(11.4 / 8) = 1.19 would be the limit with nothing in hand; 1.1 is 9.7 m/s^2, 85 % of
#                           the tyres, the rest for braking into the corner and for the plant not being the plan
#   progress_cost = 0.1     small against w_bound = 1e4, so that the hinge and not the reward decides at the ceiling: going eps
#                           over it for the 20 steps that remain gains 0.1 eps and costs 2e5 eps^2 - only eps < 5e-7 m/s would
#                           pay, an eighth of an ulp of 37 m/s; and large enough that the reward, not the other terms' noise
#                           between candidates, decides the pedal.  The restated loop on the CPU (this config, the restatements
#                           in place of the kernels, the same plant) covers 330.0 m at 0.05 - the whole run to reach the
#                           ceiling -, 363.0 m at 0.1, 365.0 m at 0.2 and at 1.0, against A's 338.0 m; at 0.2 the winner of 4
#                           of the 200 ticks has a V of 1e-7 beside feasible candidates (w_bound V = 1e-3, lost in the noise
#                           between candidates), at 0.1 none
#   slip_limit = 0.1        TERMS_KEYS' own
LOOP_CEILING = 1.1
LOOP_B = dict(tgt.TERMS_CONFIG, **tgt.TERMS_KEYS, r_term=(0.0, 10.0), progress_cost=0.1, speed_ceiling=LOOP_CEILING)


def _step0_excess(solver, state, u0):
    """float32 vx - cap after the first control step of the plan, in the kernel's arithmetic: the restatement's step on the
    handle's own rows, the windowed search from waypoint 0, cap = fma(cs, v_ref_j, co)."""
    coef = solver.engine.coefficients(0)
    c = ds.constants(_vehicle().coefficients(), dt=tgd.LOOP_DT)
    x0 = np.asarray(state, dtype=T)
    ox, oy = coef[0, 0], coef[0, 1]
    st = [np.array([x0[0] - ox], dtype=T), np.array([x0[1] - oy], dtype=T)] + [np.array([x0[q]], dtype=T) for q in range(2, 6)]
    st = ds.dynamic_step(st, np.array([u0[0]], dtype=T), np.array([u0[1]], dtype=T), c)
    back, ahead = tgt.TERMS_CONFIG["nn_window"]
    m = np.arange(min(back + ahead + 1, len(coef)))
    wx, wy = coef[m, 0] - ox, coef[m, 1] - oy
    key = fma32(st[1], T(-2.0) * wy, fma32(st[0], T(-2.0) * wx, fma32(wy, wy, wx * wx)))
    j = int(np.argmin(np.where(np.isnan(key), T(np.inf), key)))
    cap = fma32(T(LOOP_CEILING), coef[j, 6], T(0.0))
    return float(np.asarray(st[3] - cap, dtype=T)[0])


def _run_loop(config, check_ceiling):
    """tgt.run_terms_loop's loop; per tick (e_y, |vy| / vx, centre-line index, n_feasible, violation, step-0 excess)."""
    from acmpc_amd import DynamicSamplingSolver
    plant = _vehicle()
    solver = DynamicSamplingSolver(dict(config), plant)
    centre, v_profile, heading, start = tgd.loop_track()
    state = np.array([centre[start, 0], centre[start, 1], heading[start], v_profile[start] - 4.0, 0.0, 0.0])
    n = tgd.LOOP_H - 1
    log = []
    try:
        for _ in range(tgt.TERMS_TICKS):
            table, _ = tgd.loop_path(centre, v_profile, state)
            obj = solver.solve(state, table)
            assert obj.info.status == "solved"
            u = obj.x[3 * (n + 1):].reshape(n, 2)
            excess = _step0_excess(solver, state, u[0]) if check_ceiling else 0.0
            state = plant.predict_next_state(state, u[0], tgd.LOOP_DT)[0]
            state[3] = max(state[3], 0.0)
            ey, i = tgd.loop_frenet(centre, heading, state)
            log.append((ey, abs(state[4]) / max(state[3], 1.0), i, obj.n_feasible, obj.violation, excess, state[3]))
    finally:
        solver.close()
    log = np.array(log)
    steps = np.diff(np.concatenate([[start], log[:, 2]])) % len(centre)       # centre-line samples passed per tick, 0.5 m each
    return log, 0.5 * float(np.sum(np.where(steps > len(centre) // 2, steps - len(centre), steps)))


def test_closed_loop_makes_more_progress_under_its_ceiling():
    log_a, dist_a = _run_loop(dict(tgt.TERMS_CONFIG, **tgt.TERMS_KEYS), False)
    log_b, dist_b = _run_loop(LOOP_B, True)
    print("closed loop, %d ticks: %.1f m of centre line tracking the profile, %.1f m with %r" % (
        tgt.TERMS_TICKS, dist_a, dist_b, {k: LOOP_B[k] for k in ("r_term", "progress_cost", "speed_ceiling", "slip_limit")}))
    ey, slip = log_b[:, 0], log_b[:, 1]
    print("B: max |e_y| %.3f m, mean %.3f m, sideslip %.4f, top speed %.2f m/s (A: %.2f), ticks with a feasible candidate %d"
          % (np.abs(ey).max(), np.abs(ey).mean(), slip.max(), log_b[:, 6].max(), log_a[:, 6].max(),
             np.count_nonzero(log_b[:, 3] > 0)))
    assert np.abs(ey).max() < tgd.LOOP_CORRIDOR, "left the corridor: |e_y| %.2f m" % np.abs(ey).max()
    assert slip.max() < tgd.LOOP_SLIP, "sideslip |vy| / vx %.4f" % slip.max()
    checked = 0
    for tick in range(tgt.TERMS_TICKS):
        if log_b[tick, 3] > 0:
            assert log_b[tick, 4] == 0.0, "tick %d: a winner with V %.3g among %d feasible candidates" % (
                tick, log_b[tick, 4], log_b[tick, 3])
            assert max(T(log_b[tick, 5]), T(0.0)) == 0.0, "tick %d: %.3g m/s over the ceiling after step 0" % (tick, log_b[tick, 5])
            checked += 1
    assert checked > tgt.TERMS_TICKS // 2
    assert dist_b > dist_a
