"""Mode D's integration setting (acmpc_set_dynamics_integration) on the MI355X: M Euler sub-steps per control step and the
low-speed blend, from every call form.  Costs, keys, feasible counts and records must be bit-identical to
tests/dynamic_spec.py - alone on the small shapes, and through the forms already held to it (the
one-candidate-per-lane kernels, the control matrix) on the large ones; the default setting must give the bits of a handle
that never heard of the call; and DynamicSamplingSolver with the setting drives a finely integrated plant round a 15 m
circle from a standstill."""
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

pytestmark = pytest.mark.gpu

BLEND = (3.0, 5.0)
SETTINGS = [(m, b) for b in (None, BLEND) for m in (1, 2, 5, 16)]
FINE = (4, BLEND)             # the setting the documents recommend
BIG_OFFSET = tsm.BIG_OFFSET


def _id(setting):
    return "M%d-%s" % (setting[0], "blend" if setting[1] else "plain")


def _vehicle():
    from acmpc_amd import DynamicBicycleParams
    return DynamicBicycleParams.reference()


# ---- one candidate per lane ---------------------------------------------------------------------------------------------
# P = 3, N = 300 (the second workgroup's tail), n = 2 and 49.  The three problems start at a standstill (below the blend
# interval), inside it and above it; with the windowed search, below it, inside it and at the path's speed.
START_SPEEDS = {None: (0.0, 4.0, 9.0), (2, 5): (2.0, 4.5, None)}
# (layout, window): both layouts and both searches for every setting; the other two pairings for one of them.  The NumPy
# specification costs about 4 ms per sub-step whatever N is - 12 s for the three problems at n = 49, M = 16 - so those two
# settings run one pairing each (the exhaustive search without the blend, the windowed one with it).
PAIRINGS = [(0, None), (1, (2, 5))]
ONE_PER_LANE = [(n, s, lay, w) for n in (2, 49) for s in SETTINGS for i, (lay, w) in enumerate(PAIRINGS)
                if not (n == 49 and s[0] == 16 and i != (s[1] is not None))] + \
               [(n, (5, BLEND), lay, w) for n in (2, 49) for lay, w in ((1, None), (0, (2, 5)))]


def _lane_problems(N, n, window):
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 200 + p, vx0=v) for p, v in enumerate(START_SPEEDS[window])]
    dps[0]["U"][5, n // 2, 1] = np.nan      # a NaN pedal ranks last
    dps[1]["U"][7, 0, 0] = np.inf           # an inf steering angle
    return dps


@pytest.mark.parametrize("n,setting,layout,window", ONE_PER_LANE,
                         ids=["n%d-%s-layout%d-%s" % (n, _id(s), lay, "window" if w else "all") for n, s, lay, w in ONE_PER_LANE])
def test_costs_argmin_and_record_are_the_specification(n, setting, layout, window):
    from acmpc_amd import _capi
    P, N = 3, 300
    dps = _lane_problems(N, n, window)
    eng = tgd._engine(dps, P, N, n, window)
    try:
        eng.set_dynamics_integration(*setting)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        out = eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)
        for p in range(P):
            cost, V, X = ds.spec_costs(orc, dps[p], eng.coefficients(p), _vehicle().coefficients(), nn_window=window,
                                       return_states=True, settings=Settings(*setting))
            tgd._same_bits(out["costs"][p], cost)
            best = tgd._check_record(_capi.split_record(out["records"][p], n), U_h[p], cost, V, X, n)
            assert out["best_idx"][p] == best
            assert out["n_feasible"][p] == np.count_nonzero(V == 0)
        assert np.isnan(out["costs"][0][5]) and not np.isfinite(out["costs"][1][7])
    finally:
        eng.close()


# ---- the default setting --------------------------------------------------------------------------------------------------
def test_default_setting_is_a_handle_that_never_made_the_call():
    """(1, 0, 0), and (4, 3, 5) then back to (1, 0, 0): the bits of a handle that never called - costs, records, and
    acmpc_optimize's records.  A refused call keeps the setting it found."""
    P, N, n = 2, 700, 30
    dps = tgd._problems(P, N, n, seed=310)
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    centre = np.tile(np.stack([np.zeros(n), np.full(n, 0.2)], axis=1).astype(np.float32), (P, 1, 1))

    def run(prepare):
        eng = tgd._engine(dps, P, N, n, (2, 5))
        try:
            prepare(eng)
            out = eng.solve(x0, U)
            opt = eng.optimize(x0, centre, None, N, 2, (0.05, 0.3), shrink=0.5, seed=77)
            return out["costs"], out["records"], opt["records"]
        finally:
            eng.close()

    def there_and_back(eng):
        eng.set_dynamics_integration(*FINE)
        assert not np.array_equal(eng.solve(x0, U)["costs"].view(np.uint32), never[0].view(np.uint32))
        eng.set_dynamics_integration(1, None)

    def refused(eng):
        assert eng._lib.acmpc_set_dynamics_integration(eng._ctx, 17, 3.0, 5.0) == -1
        assert eng._lib.acmpc_set_dynamics_integration(eng._ctx, 4, 5.0, 3.0) == -1

    never = run(lambda eng: None)
    for prepare in (lambda eng: eng.set_dynamics_integration(1, None), there_and_back, refused):
        for got, want in zip(run(prepare), never):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for p in range(P):   # (and that handle is dynamic_spec's, as ever)
        tgd._same_bits(never[0][p], ds.spec_costs(orc, dps[p], orc.coefficients_temporal(
            dps[p]["table"], dps[p]["kw"]["margin"]).astype(np.float32), _vehicle().coefficients(), nn_window=(2, 5))[0])


# ---- ensembles -------------------------------------------------------------------------------------------------------------
GRIPS = (1.0, 0.6, 1.3)


@pytest.mark.parametrize("setting", [FINE, (2, None)], ids=_id)
@pytest.mark.parametrize("reduce,layout,window", [("mean", 0, None), ("max", 1, (2, 5))])
def test_ensemble_is_the_specification(reduce, layout, window, setting):
    """K = 3 grips: every member is blended with its own lf, lr (here the same) and stepped with its own tyres."""
    from acmpc_amd import _capi
    P, N, n = 2, 130, 20
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 400 + p, vx0=v) for p, v in enumerate((0.0, 6.0))]
    dps[0]["U"][5, n // 2, 1] = np.nan
    vehicles = [_vehicle().with_grip(g) for g in GRIPS]
    weights = (1.0, 2.0, 0.5) if reduce == "mean" else None
    eng = tge._engine(dps, P, N, n, window)
    try:
        eng.set_dynamics_integration(*setting)      # before the vehicles: the setting does not depend on them
        eng.set_dynamics_ensemble(vehicles, weights=weights, reduce=reduce)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        out = eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)
        for p in range(P):
            J, V, X = es.spec_ensemble(orc, dps[p], eng.coefficients(p), [v.coefficients() for v in vehicles], reduce=reduce,
                                       weights=weights, nn_window=window, return_states=True, settings=Settings(*setting))
            tgd._same_bits(out["costs"][p], J)
            best = tgd._check_record(_capi.split_record(out["records"][p], n), U_h[p], J, V, X, n)
            assert out["best_idx"][p] == best
    finally:
        eng.close()


def test_ensemble_of_one_is_the_single_vehicle_and_members_use_their_own_wheelbase():
    import dataclasses
    P, N, n = 2, 130, 20
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 420 + p, vx0=v) for p, v in enumerate((1.0, 4.0))]
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    eng = tge._engine(dps, P, N, n, (2, 5))
    try:
        eng.set_dynamics_integration(*FINE)
        eng.set_dynamics(_vehicle())
        single = eng.solve(x0, U)
        eng.set_dynamics_ensemble([_vehicle()], reduce="mean")
        one = eng.solve(x0, U)
        assert np.array_equal(one["costs"].view(np.uint32), single["costs"].view(np.uint32))
        assert np.array_equal(one["records"].view(np.uint32), single["records"].view(np.uint32))
        # two members with different lf, lr: each blended towards ITS kinematic bicycle
        long_car = dataclasses.replace(_vehicle(), lf=1.9, lr=1.1)
        eng.set_dynamics_ensemble([_vehicle(), long_car], reduce="max")
        out = eng.solve(x0, U)
        for p in range(P):
            J = es.spec_ensemble(orc, dps[p], eng.coefficients(p), [_vehicle().coefficients(), long_car.coefficients()],
                                 reduce="max", nn_window=(2, 5), settings=Settings(*FINE))[0]
            tgd._same_bits(out["costs"][p], J)
    finally:
        eng.close()


# ---- the sampled forms and acmpc_optimize -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P,N,n,K,window,with_ref,rnd,offset,setting", [
    (3, 1537, 30, 1, (2, 5), True, 2, 0, FINE),
    (1, 1000, 49, 1, None, False, 1, BIG_OFFSET, (16, None)),
    (3, 300, 49, 3, (2, 5), True, 0, BIG_OFFSET, FINE),
    (1, 131, 8, 4, None, True, 1, 0, (2, BLEND)),
])
def test_fused_rollout_equals_sample_then_rollout(P, N, n, K, window, with_ref, rnd, offset, setting):
    rig = tsm.Rig(P, N, n, K=K, window=window, seed=500 + n, with_ref=with_ref, kinds=[(1, 0, 3)[p % 3] for p in range(P)])
    try:
        rig.eng.set_dynamics_integration(*setting)
        sigma, seed = (0.04, 0.35), 0xC0FFEE1234
        U, costs, keys = tsm._compare_rollouts(rig, N, offset, sigma, seed, rnd)
        tsm._compare_records(rig, U, keys, N, offset, sigma, seed, rnd)
    finally:
        rig.close()


@pytest.mark.parametrize("K", [1, 3])
def test_fused_rollout_and_optimize_equal_the_specification(K):
    """One small shape against the restatements alone: the fused rollout's costs, key and count, the re-drawn record, and
    acmpc_optimize's argmin rounds (candidates of dynamic_sampled_spec round the previous winner)."""
    from acmpc_amd import _capi
    P, N, n, sigma, seed, rnd, window = 2, 96, 12, (0.05, 0.3), 99, 3, (2, 5)
    rig = tsm.Rig(P, N, n, K=K, window=window, seed=540, with_ref=True, kinds=[1, 0])
    try:
        rig.eng.set_dynamics_integration(*FINE)
        for offset in (0, BIG_OFFSET):
            costs, keys = rig.fused(N, offset, sigma, seed, rnd)
            rec = rig.finalize_sampled(None, N, sigma, seed, rnd)
            for p in range(P):
                want = dss.rollout_sampled(orc, rig.dps[p], rig.eng.coefficients(p), rig.blocks(), rig.centre_h[p],
                                           rig.ref_h[p], N, offset, p, rnd, seed, sigma, reduce=rig.reduce,
                                           weights=rig.weights, nn_window=window, return_states=True, settings=Settings(*FINE))
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
                cost, V, X = dss.costs(orc, rig.dps[p], rig.eng.coefficients(p), rig.blocks(), U, rig.reduce,
                                       rig.weights, window, return_states=True, settings=Settings(*FINE))
                centre = U[orc.pick_best(cost)[0]]
            tgd._check_record(_capi.split_record(got[p], n), U, cost, V, X, n)
    finally:
        rig.close()


@pytest.mark.parametrize("update", ["argmin", "softmin"])
@pytest.mark.parametrize("vehicles", [None, (0, 1, 2)], ids=["K1", "K3"])
def test_optimize_with_and_without_the_matrix_and_the_sharded_optimizer(vehicles, update):
    """Rounds 2, both centre updates: the default rounds (no control matrix) against the matrix rounds, bit for bit, and
    ShardedOptimizer at world size 1 against both."""
    import torch
    from acmpc_amd.sharding import ShardedOptimizer
    P, N, n, rounds, sigma, shrink, seed = 2, 1025, 30, 2, (0.05, 0.3), 0.5, 1234
    eng, dps = tsf._dynamic_engine(P, N, n, seed=560, vehicles=vehicles, window=(2, 5), centre_update=update,
                                   softmin_lambda=0.5)
    try:
        eng.set_dynamics_integration(*FINE)
        centre, ref = tsf._centres(dps, n, 3)
        x0 = np.stack([d["x0"] for d in dps])
        x0[0, 3] = 0.5                                # one problem from (nearly) a standstill
        default = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", "1")
        matrix = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", None)
        tsm._same_bits(default, matrix, "the rounds without a matrix against the rounds through it")
        assert np.all(default[:, 3] == 1.0) and np.all(np.isfinite(default[:, 0]))
        eng.set_dynamics_integration(1, None)
        plain = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        assert not np.array_equal(plain.view(np.uint32), default.view(np.uint32))   # (the setting reaches these rounds)
        eng.set_dynamics_integration(*FINE)
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
    """test_gpu_dynamic_sampled's four emulated ranks, the launch's first candidate at a large odd global index."""
    import torch
    from acmpc_amd import _capi
    from acmpc_amd.sharding import shard_range
    P, N, n, sigma, seed, rnd, base = 3, 1030, 30, (0.05, 0.3), 4242, 1, BIG_OFFSET
    rig = tsm.Rig(P, N, n, K=K, window=(2, 5), seed=580, with_ref=True, kinds=[1, 0, 3])
    try:
        rig.eng.set_dynamics_integration(*FINE)
        U, costs, keys = tsm._compare_rollouts(rig, N, base, sigma, seed, rnd)
        whole = tsm._compare_records(rig, U, keys, N, base, sigma, seed, rnd)
        slices = [shard_range(N, r, 4) for r in range(4)]
        shard_keys, shard_costs = [], []
        for off, count in slices:
            c, k = rig.fused(count, base + off, sigma, seed, rnd)
            shard_keys.append(k.cpu().numpy())
            shard_costs.append(c.cpu().numpy())
        tsm._same_bits(np.concatenate(shard_costs, axis=1), costs.cpu().numpy())
        reduced_h = np.minimum.reduce(shard_keys)                 # the all-reduce(MIN), on the host
        assert np.array_equal(reduced_h, keys.cpu().numpy())
        reduced = torch.tensor(reduced_h, device=rig.dev)
        recs = []
        for off, count in slices:   # each rank: its own rollout (partial counts in the handle), then the finalize on the keys
            rig.fused(count, base + off, sigma, seed, rnd, want_costs=False, want_keys=False)
            recs.append(rig.finalize_sampled(reduced, count, sigma, seed, rnd))
        for p in range(P):
            assert base <= _capi.key_index(int(reduced_h[p])) < base + N
            for rec in recs:
                assert rec[p][3] == 1.0
                tsm._same_bits(np.delete(rec[p], 2), np.delete(whole[p], 2), "problem %d" % p)
            assert sum(float(rec[p][2]) for rec in recs) == float(whole[p][2])
    finally:
        rig.close()


# ---- two candidates per lane ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,layout,window", [(1, 1, (2, 5)), (2, 0, None)])
def test_packed_rollout(K, layout, window):
    """P N K >= 2^20 at n = 4 with an odd N: the f32x2 step loop of the FINE kernels.  In full against the
    one-candidate-per-lane kernels - two shards of candidates by index_offset, each below 2^20 - and against the
    specification on each problem's first and last candidates, the workgroup boundaries, the planted non-finite controls
    and a seeded draw (test_gpu_dynamic_packed's subset)."""
    import torch
    from acmpc_amd import _capi
    N, n = 4099, 4
    P = tpk._problems_for(N, K)
    half = (N + 1) // 2
    assert P * N * K >= tpk.PACKED and P * half * K < tpk.PACKED
    label = "K %d layout %d window %s P %d" % (K, layout, window, P)
    base, U, x0, tables = tpk._make(P, N, n, seed=600 + K)
    x0[1::4, 3] = 0.0          # (kind 1 is the standstill already; kinds 2 and 3 inside and below the blend interval)
    x0[2::4, 3] = 4.0
    x0[3::4, 3] = 2.0
    planted = tpk._plant(U, N, n)
    vehicles = [_vehicle()] if K == 1 else [_vehicle(), _vehicle().with_grip(0.6)]
    eng = tge._engine([base[p % 4] for p in range(P)], P, N, n, window)
    try:
        eng.set_dynamics_integration(*FINE)
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
                                     settings=Settings(*FINE))
            return es.spec_ensemble(orc, dp, coefs[q], blocks, reduce="mean", nn_window=window, U=U_sub, return_states=states,
                                    settings=Settings(*FINE))

        tpk._check_against_spec(whole, base, coefs, U, N, n, tpk.GROUP_ONE if K == 1 else tpk.GROUP_ENSEMBLE, planted, spec,
                                17 + K, label)
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
        for lo, count, d_U, cs, ks in parts:   # each shard: its rollout (partials in the handle), then the finalize on the keys
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


# ---- random shapes ----------------------------------------------------------------------------------------------------------
HORIZONS = [3, 4, 9, 17, 33, 50, 65, 100, 130, 257, 513]
CANDIDATES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 700]
SUBSTEPS = list(range(1, 17))
WINDOWS = [None, (2, 5), (1, 2), (3, 12), (20, 43)]
FUZZ_CASES = 10
FUZZ_BUDGET_S = 0.9           # of the NumPy specification per case (test_gpu_fuzz_dynamic's estimate, the step M times)
LONGEST = dict(H=513, M=2, N=17, P=1, window=(2, 5), blend=BLEND, layout=1, K=1, speeds=[0.0])


def _spec_seconds(c):
    n = c["H"] - 1
    W = n if c["window"] is None else min(c["window"][0] + c["window"][1] + 1, n)
    return c["P"] * c["K"] * (3.3e-3 * n * c["M"] + 8.0e-8 * c["N"] * n * W)


def _fuzz_case(rng):
    """n <= 512, M <= 16, N <= 700, P <= 5.  A case above the budget gives up problems, then vehicles, then sub-steps (the
    specification's time hardly depends on N), then candidates - never its horizon, window, blend or layout."""
    c = dict(H=int(rng.choice(HORIZONS)), M=int(rng.choice(SUBSTEPS)), N=int(rng.choice(CANDIDATES)), P=int(rng.integers(1, 6)),
             window=WINDOWS[int(rng.integers(0, len(WINDOWS)))],
             blend=[None, BLEND, (0.0, 8.0), (5.0, 5.5)][int(rng.integers(0, 4))], layout=int(rng.integers(0, 2)),
             K=int(rng.choice([1, 1, 2, 3])), speeds=[[0.0, 1.0, 3.0, 4.0, 5.2, 7.0, None][int(i)] for i in rng.integers(0, 7, 5)])
    while _spec_seconds(c) > FUZZ_BUDGET_S:
        if c["P"] > 1:
            c["P"] -= 1
        elif c["K"] > 1:
            c["K"] -= 1
        elif c["M"] > 1:
            c["M"] -= 1
        elif c["N"] > 1:
            c["N"] = max(v for v in CANDIDATES if v < c["N"])
        else:
            break
    return c


def test_random_shapes_against_the_specification():
    from acmpc_amd import _capi
    rng = np.random.default_rng(20261018)
    todo = [LONGEST] + [_fuzz_case(rng) for _ in range(FUZZ_CASES)]
    assert any(c["M"] > 8 for c in todo) and any(c["K"] > 1 for c in todo) and any(c["blend"] for c in todo)
    for index, c in enumerate(todo):
        label = "case %d: %r" % (index, c)
        P, N, n = c["P"], c["N"], c["H"] - 1
        dps = [ds.make_dynamic_problem(orc, "monza", c["H"], N, 21000 + 10 * index + p, vx0=c["speeds"][p]) for p in range(P)]
        if N > 8 and index % 3 == 1:
            dps[0]["U"][5, n // 2, 0] = np.nan
            dps[0]["U"][7, 0, 1] = np.inf
        vehicles = [_vehicle().with_grip(g) for g in GRIPS[:c["K"]]]
        eng = tge._engine(dps, P, N, n, c["window"])
        try:
            eng.set_dynamics_integration(c["M"], c["blend"])
            if c["K"] == 1:
                eng.set_dynamics(vehicles[0])
            else:
                eng.set_dynamics_ensemble(vehicles, reduce="mean")
            U = np.stack([d["U"] for d in dps])
            data = U if c["layout"] == 0 else np.ascontiguousarray(U.transpose(0, 2, 3, 1))
            out = eng.solve(np.stack([d["x0"] for d in dps]), data, layout=c["layout"])
            for p in range(P):
                cost, V, X = dss.costs(orc, dps[p], eng.coefficients(p), [v.coefficients() for v in vehicles], dps[p]["U"],
                                       nn_window=c["window"], return_states=True, settings=Settings(c["M"], c["blend"]))
                nan = np.isnan(cost)
                assert np.array_equal(np.isnan(out["costs"][p]), nan), label
                assert np.array_equal(out["costs"][p][~nan].view(np.uint32), cost[~nan].view(np.uint32)), label
                assert out["best_idx"][p] == orc.pick_best(cost)[0], label
                assert out["n_feasible"][p] == np.count_nonzero(V == 0), label
                tgd._check_record(_capi.split_record(out["records"][p], n), U[p], cost, V, X, n)
        finally:
            eng.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------------
# DynamicSamplingSolver drives the float64 mirror integrated with 16 sub-steps and the blend (the plant) round a circle of
# radius 15 m, counter-clockwise, for 200 ticks of 0.05 s FROM A STANDSTILL, tangent to the circle.  Each tick it is fed the
# window of the circle ahead of the car: 50 waypoints 0.4 m apart (the horizon's travel at the profile's 6 m/s is 14.7 m).
CIRCLE_R = 15.0
CIRCLE_V = 6.0
CIRCLE_WIDTH = 7.56           # with margin 0 the corridor of test_gpu_dynamic's loop: 3.78 m either side
CIRCLE_H = 50
CIRCLE_SPACING = 0.4
CIRCLE_TICKS = 200
CIRCLE_DT = 0.05
CIRCLE_SETTLE_S = 4.0         # the launch: 0 -> 6 m/s
CIRCLE_CONFIG = dict(tgd.LOOP_CONFIG, horizon=CIRCLE_H, margin=0.0, sampling_sigma=(0.05, 0.3), rollout_dt=CIRCLE_DT)
PLANT_SETTING = dict(substeps=16, low_speed_blend=BLEND)


def circle_table(state):
    """The [7, n] table of the 50 waypoints ahead of the car on the circle (world frame), v = 6 m/s."""
    theta0 = np.arctan2(state[1], state[0])
    theta = theta0 + CIRCLE_SPACING / CIRCLE_R * np.arange(CIRCLE_H)
    xy = CIRCLE_R * np.column_stack([np.cos(theta), np.sin(theta)])
    table = orc.construct_waypoints(np.column_stack([xy, np.full(CIRCLE_H, CIRCLE_WIDTH)]))
    table[orc.ROW_V] = CIRCLE_V
    return table


def run_circle(config):
    """The loop under `config`; per tick (e_y, vx - v_ref, yaw rate, steering command)."""
    from acmpc_amd import DynamicSamplingSolver
    plant = _vehicle()
    solver = DynamicSamplingSolver(dict(config), plant)
    n = CIRCLE_H - 1
    state = np.array([CIRCLE_R, 0.0, np.pi / 2, 0.0, 0.0, 0.0])
    log = []
    try:
        for _ in range(CIRCLE_TICKS):
            obj = solver.solve(state, circle_table(state))
            assert obj.info.status == "solved"
            u = obj.x[3 * (n + 1):].reshape(n, 2)
            state = plant.rollout(state, u[:1], CIRCLE_DT, **PLANT_SETTING)[-1]
            log.append((CIRCLE_R - np.hypot(state[0], state[1]), state[3] - CIRCLE_V, state[5], u[0, 0]))
    finally:
        solver.close()
    return np.array(log)


def circle_figures(log):
    settled = int(CIRCLE_SETTLE_S / CIRCLE_DT)
    ey, dv = log[:, 0], log[:, 1]
    return dict(max_ey=float(np.abs(ey).max()), mean_ey=float(np.abs(ey).mean()),
                speed_error_after_settling=float(np.abs(dv[settled:]).max()),
                steering_sign_changes=int(np.count_nonzero(np.diff(np.sign(np.diff(log[:, 3]))) != 0)))


def test_closed_loop_round_a_15_m_circle_from_a_standstill():
    """test_gpu_dynamic's bars: |e_y| inside the 3.78 m corridor throughout and 0.25 m on average, the speed within
    0.5 m/s of the profile once the launch (4 s) is over."""
    fig = circle_figures(run_circle(dict(CIRCLE_CONFIG, rollout_substeps=4, low_speed_blend=BLEND)))
    print("closed loop, 4 sub-steps and the blend:", fig)
    assert fig["max_ey"] < CIRCLE_WIDTH / 2, "left the corridor: |e_y| %.2f m" % fig["max_ey"]
    assert fig["mean_ey"] < tgd.LOOP_MEAN_EY, "does not hold the centre line: mean |e_y| %.2f m" % fig["mean_ey"]
    assert fig["speed_error_after_settling"] < tgd.LOOP_SPEED_BAND, \
        "speed off the profile by %.2f m/s after %.0f s" % (fig["speed_error_after_settling"], CIRCLE_SETTLE_S)
