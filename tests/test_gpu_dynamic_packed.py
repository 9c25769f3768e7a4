"""Mode D's two-candidates-per-lane rollouts on the MI355X: launches with P N K >= 2^20, which take
rollout_dynamic_kernel<LAYOUT, 2> (one vehicle) and rollout_dynamic_ensemble_kernel<LAYOUT, 2> (K > 1) - the f32x2 step,
the two-row settle and the pair tail of an odd N.  tools/bench_dynamic.py times these kernels and compares their costs
with nothing; this file is that comparison.

The float32 restatement is too slow for 2^20 candidates, and candidates are independent, so every case runs two checks:
 (i)  packed against unpacked: the same problems and controls scored again in slices of problems whose P' N K is below
      2^20 - the one-candidate-per-lane kernels that test_gpu_dynamic / test_gpu_dynamic_ensemble hold to the
      specification in full.  Every cost, best index and the whole record (n_feasible in it) must have the same bits.
 (ii) packed against the specification, bit for bit, on a subset of candidates of EVERY problem: the first and last
      four, two either side of every workgroup boundary, the planted non-finite candidates and their neighbours, a
      seeded draw; and the full record of the winner of four problems (one per kind).
Each test asserts the threshold it relies on."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_ensemble_spec as es
import dynamic_spec as ds
import test_gpu_dynamic as tgd
import test_gpu_dynamic_ensemble as tge

pytestmark = pytest.mark.gpu

PACKED = 1 << 20          # dynamic_candidates_per_lane(P, N, K) == 2 from here (csrc/acmpc_dynamic.hip)
GROUP_ONE = 512           # candidates per workgroup of the packed single-vehicle rollout: 256 lanes x 2
GROUP_ENSEMBLE = 128      # and of the packed ensemble rollout: 64 lanes x 2, K waves
DRAW = 192                # seeded random candidates per problem on top of the edges


def _problems_for(N, K):
    return -(-PACKED // (N * K))


def _make(P, N, n, seed):
    """P problems of test_gpu_dynamic's four kinds (problem p is kind p % 4: the kinds' tables and starts are shared, the
    controls are not): (the four base problems, U [P, N, n, 2], x0 [P, 6], tables)."""
    base = tgd._problems(4, N, n, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    U = np.stack([base[p % 4]["U"] for p in range(P)])
    U[..., 0] += rng.standard_normal(U.shape[:-1], dtype=np.float32) * np.float32(0.01)
    U[..., 0] = np.clip(U[..., 0], ds.U_MIN[0], ds.U_MAX[0])
    x0 = np.stack([base[p % 4]["x0"] for p in range(P)])
    tables = np.stack([base[p % 4]["table"] for p in range(P)])
    return base, U, x0, tables


def _plant(U, N, n):
    """Non-finite controls where the pair handling could go wrong.  An odd N: a NaN pedal (problem 0) and an inf steering
    (problem 5) in the LAST candidate - element 0 of the last pair, whose element 1 repeats it and must not be reported.
    Any N: a NaN pedal (problem 2) and an inf pedal (problem 7) in element 1 of an interior pair; element 0 is its
    neighbour.  Returns {problem: [candidates]}."""
    planted = {}
    P = U.shape[0]
    if N % 2 == 1:
        U[0, N - 1, n // 2, 1] = np.nan
        planted[0] = [N - 1]
        if P > 5:
            U[5, N - 1, 0, 0] = np.inf
            planted[5] = [N - 1]
    inner = (N // 2) | 1
    U[2, inner, n - 1, 1] = np.nan
    planted[2] = [inner]
    if P > 7:
        U[7, inner, 0, 1] = -np.inf
        planted[7] = [inner]
    return planted


def _subset(N, group, planted, rng):
    idx = set(range(min(4, N))) | set(range(max(N - 4, 0), N))
    for b in range(group, N, group):
        idx |= {b - 2, b - 1, b, b + 1}
    for c in planted:
        idx |= {c - 1, c, c + 1}
    idx |= set(int(c) for c in rng.integers(0, N, DRAW))
    return np.array(sorted(c for c in idx if 0 <= c < N), dtype=np.int64)


def _as_layout(U, layout):
    return U if layout == 0 else np.ascontiguousarray(np.moveaxis(U, -3, -1))   # [.., N, n, 2] -> [.., n, 2, N]


def _check_against_unpacked(eng, out, x0, U_in, tables, N, K, label):
    """Check (i): slices of problems below the threshold, on the same handle."""
    P = x0.shape[0]
    chunk = (PACKED - 1) // (N * K)
    assert 1 <= chunk < P and chunk * N * K < PACKED, label
    layout = 0 if U_in.shape[-1] == 2 else 1
    for lo in range(0, P, chunk):
        hi = min(lo + chunk, P)
        eng.set_paths(tables[lo:hi])
        part = eng.solve(x0[lo:hi], U_in[lo:hi], layout=layout)
        tgd._same_bits(part["costs"], out["costs"][lo:hi])
        assert np.array_equal(part["best_idx"], out["best_idx"][lo:hi]), label
        assert np.array_equal(part["n_feasible"], out["n_feasible"][lo:hi]), label
        assert np.array_equal(part["records"].view(np.uint32), out["records"][lo:hi].view(np.uint32)), label
    eng.set_paths(tables)


def _check_against_spec(out, base, coefs, U, N, n, group, planted, spec, seed, label):
    """Check (ii): `spec(q, U_subset, states)` is the specification of kind q's problem on controls U_subset."""
    from acmpc_amd import _capi
    P = U.shape[0]
    rng = np.random.default_rng(seed)
    picks = [_subset(N, group, planted.get(p, ()), rng) for p in range(P)]
    for q in range(4):
        members = [p for p in range(P) if p % 4 == q]
        cost = spec(q, np.concatenate([U[p][picks[p]] for p in members]), False)[0]
        at = 0
        for p in members:
            got = out["costs"][p][picks[p]]
            want = cost[at:at + len(picks[p])]
            at += len(picks[p])
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), \
                "%s: problem %d, candidates %s" % (label, p, picks[p][np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8]])
    for p in range(P):   # the argmin over the launch's own costs, NaN last
        best = orc.pick_best(out["costs"][p])[0]
        assert out["best_idx"][p] == best, "%s: problem %d" % (label, p)
        assert out["n_feasible"][p] <= N - len(planted.get(p, ())), label
        for c in planted.get(p, ()):
            assert not np.isfinite(out["costs"][p][c]) and best != c, "%s: problem %d candidate %d" % (label, p, c)
    for p in range(min(P, 4)):   # the winner's whole record, one problem of each kind
        best = int(out["best_idx"][p])
        cost, V, X = spec(p % 4, U[p][best:best + 1], True)
        rec = _capi.split_record(out["records"][p], n)
        assert rec["owner"] == 1.0, label
        tgd._same_bits(rec["cost"], cost[0])
        tgd._same_bits(rec["violation"], V[0])
        tgd._same_bits(rec["u"], U[p][best])
        tgd._same_bits(rec["x"], X[0])


# ---- one vehicle ---------------------------------------------------------------------------------------------------
# N: 4099 odd with three candidates in the last workgroup (a pair and half a pair), 2561 = 5 x 512 + 1 one real candidate
# in the last workgroup, 4096 a full last workgroup; 32769 and 16385 (64 and 32 x 512 + 1) keep P small at the long horizons
ONE_VEHICLE = [(4099, 20, 0, None), (4099, 20, 1, (2, 5)), (2561, 20, 1, None), (2561, 20, 0, (2, 5)),
               (4096, 20, 0, (2, 5)), (4096, 20, 1, None), (4099, 2, 0, (2, 5)), (4099, 2, 1, None),
               (32769, 72, 1, (2, 5)), (16385, 65, 0, None)]


@pytest.mark.parametrize("N,n,layout,nn_window", ONE_VEHICLE)
def test_one_vehicle_packed_rollout(N, n, layout, nn_window):
    from acmpc_amd import DynamicBicycleParams
    P = _problems_for(N, 1)
    assert P * N * 1 >= 1 << 20
    label = "N %d n %d layout %d window %s P %d" % (N, n, layout, nn_window, P)
    base, U, x0, tables = _make(P, N, n, seed=300 + n)
    planted = _plant(U, N, n)
    vehicle = DynamicBicycleParams.reference().coefficients()
    eng = tgd._engine([base[p % 4] for p in range(P)], P, N, n, nn_window)
    try:
        U_in = _as_layout(U, layout)
        out = eng.solve(x0, U_in, layout=layout)
        coefs = [eng.coefficients(q) for q in range(4)]

        def spec(q, U_sub, states):
            return ds.spec_costs(orc, base[q], coefs[q], vehicle, nn_window=nn_window, U=U_sub, return_states=states)

        _check_against_spec(out, base, coefs, U, N, n, GROUP_ONE, planted, spec, 7 + N, label)
        _check_against_unpacked(eng, out, x0, U_in, tables, N, 1, label)
    finally:
        eng.close()


def test_optimize_with_packed_rounds():
    """acmpc_optimize with P N >= 2^20 (an odd N) == the loop of sample_device + solve_device calls, and its last round's
    winners are the specification's on what the product's sampler drew."""
    import torch
    from acmpc_amd import DynamicBicycleParams, _capi
    N, n, rounds, sigma, shrink, seed, window = 4097, 20, 2, (0.05, 0.3), 0.5, 4321, (2, 5)
    P = _problems_for(N, 1)
    assert P * N * 1 >= 1 << 20
    base, _, x0, tables = _make(P, 8, n, seed=520)
    eng = tgd._engine([base[p % 4] for p in range(P)], P, N, n, window)
    try:
        centre = np.tile(np.stack([np.zeros(n), np.full(n, 0.2)], axis=1).astype(np.float32), (P, 1, 1))
        out = eng.optimize(x0, centre, None, N, rounds, sigma, shrink=shrink, seed=seed)
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream().cuda_stream
        R = _capi.record_floats(n)
        d_x0, d_centre = torch.tensor(x0, device=dev), torch.tensor(centre, device=dev)
        U = torch.empty(P, n, 2, N, device=dev)
        rec = torch.empty(P, R, device=dev)
        keys = torch.empty(P, dtype=torch.int64, device=dev)
        for r in range(rounds):
            ptr, stride = (d_centre.data_ptr(), 2 * n) if r == 0 else (rec.data_ptr() + 4 * _capi.REC_HEADER, R)
            eng.sample_device(ptr, stride, 0, P, N, n, 1, 0, (sigma[0] * shrink**r, sigma[1] * shrink**r), seed, r,
                              U.data_ptr(), s)
            eng.solve_device(d_x0.data_ptr(), U.data_ptr(), P, N, n, 1, 0, keys.data_ptr(), rec.data_ptr(), s)
            torch.cuda.synchronize()
        manual = rec.cpu().numpy()
        assert np.array_equal(out["records"].view(np.uint32), manual.view(np.uint32))
        vehicle = DynamicBicycleParams.reference().coefficients()
        best = [_capi.key_index(int(k)) for k in keys.cpu().numpy()]
        for p in range(4):   # one problem of each kind in full: the last round's winner is the specification's argmin
            u = np.ascontiguousarray(U[p].cpu().numpy().transpose(2, 0, 1))
            cost, V, X = ds.spec_costs(orc, base[p], eng.coefficients(p), vehicle, nn_window=window, U=u, return_states=True)
            assert best[p] == orc.pick_best(cost)[0]
            got = _capi.split_record(out["records"][p], n)
            assert got["owner"] == 1.0 and got["n_feasible"] == np.count_nonzero(V == 0)
            for name, want in (("cost", cost[best[p]]), ("violation", V[best[p]]), ("u", u[best[p]]), ("x", X[best[p]])):
                tgd._same_bits(got[name], want)
    finally:
        eng.close()


# ---- ensembles -------------------------------------------------------------------------------------------------------
# K = 3: an odd number of waves, tge's (default, the reference's literal block, grip 1.1) with weights; K = 8: a 512-lane
# workgroup, every vehicle of tge._vehicles() (the literal one among them: huge or non-finite costs under that vehicle)
WEIGHTS = {3: (1.0, 2.0, 0.5), 8: (1.0, 2.0, 0.5, 1.0, 3.0, 1.0, 1.5, 0.25)}
VEHICLES = {3: (0, 3, 2), 8: tuple(range(8))}
ENSEMBLES = [(3, "mean", 0, None), (3, "max", 1, (2, 5)), (3, "mean", 1, (2, 5)), (3, "max", 0, None),
             (8, "mean", 0, (2, 5)), (8, "max", 1, None), (8, "mean", 1, None), (8, "max", 0, (2, 5))]


@pytest.mark.parametrize("K,reduce,layout,nn_window", ENSEMBLES)
def test_ensemble_packed_rollout(K, reduce, layout, nn_window):
    N, n = 4097, 12                    # odd, and 32 x 128 + 1: one real candidate in the last workgroup
    P = _problems_for(N, K)
    assert P * N * K >= 1 << 20
    label = "K %d %s layout %d window %s P %d" % (K, reduce, layout, nn_window, P)
    weights = WEIGHTS[K] if reduce == "mean" else None
    base, U, x0, tables = _make(P, N, n, seed=700 + K)
    planted = _plant(U, N, n)
    blocks = [tge._vehicles()[i].coefficients() for i in VEHICLES[K]]
    eng = tge._engine([base[p % 4] for p in range(P)], P, N, n, nn_window)
    try:
        tge._set(eng, VEHICLES[K], weights, reduce)
        U_in = _as_layout(U, layout)
        out = eng.solve(x0, U_in, layout=layout)
        coefs = [eng.coefficients(q) for q in range(4)]

        def spec(q, U_sub, states):
            return es.spec_ensemble(orc, base[q], coefs[q], blocks, reduce=reduce, weights=weights, nn_window=nn_window,
                                    U=U_sub, return_states=states)

        _check_against_spec(out, base, coefs, U, N, n, GROUP_ENSEMBLE, planted, spec, 11 + K, label)
        _check_against_unpacked(eng, out, x0, U_in, tables, N, K, label)
    finally:
        eng.close()


# ---- shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,layout", [(1, 1), (3, 0)])
def test_two_packed_shards(K, layout):
    """Two rollout_device shards by index_offset, each of them a packed launch; keys MIN-combined as the all-reduce leaves
    them, finalize_device on each shard: one owner record and one blank one per problem, equal to the unsharded solve -
    which checks (i) and (ii) hold to the unpacked kernels and to the specification."""
    import torch
    from acmpc_amd import DynamicBicycleParams, _capi
    shard, n, window = 4097, 10, (2, 5)
    N = 2 * shard
    P = _problems_for(shard, K)
    assert P * shard * K >= 1 << 20
    label = "K %d layout %d P %d" % (K, layout, P)
    base, U, x0, tables = _make(P, N, n, seed=900 + K)
    planted = _plant(U, N, n)
    eng = tge._engine([base[p % 4] for p in range(P)], P, N, n, window)
    try:
        if K == 1:
            eng.set_dynamics(DynamicBicycleParams.reference())
        else:
            tge._set(eng, VEHICLES[K], WEIGHTS[K], "mean")
        U_in = _as_layout(U, layout)
        whole = eng.solve(x0, U_in, layout=layout)
        coefs = [eng.coefficients(q) for q in range(4)]
        blocks = [tge._vehicles()[i].coefficients() for i in (VEHICLES[K] if K > 1 else (0,))]

        def spec(q, U_sub, states):
            if K == 1:
                return ds.spec_costs(orc, base[q], coefs[q], blocks[0], nn_window=window, U=U_sub, return_states=states)
            return es.spec_ensemble(orc, base[q], coefs[q], blocks, reduce="mean", weights=WEIGHTS[K], nn_window=window,
                                    U=U_sub, return_states=states)

        _check_against_spec(whole, base, coefs, U, N, n, GROUP_ONE if K == 1 else GROUP_ENSEMBLE, planted, spec, 13 + K, label)
        _check_against_unpacked(eng, whole, x0, U_in, tables, N, K, label)
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream().cuda_stream
        rf = _capi.record_floats(n)
        d_x0 = torch.tensor(x0, device=dev)
        parts = []
        for lo in (0, shard):
            d_U = torch.tensor(_as_layout(U[:, lo:lo + shard], layout), device=dev)
            parts.append((lo, d_U, torch.empty(P, shard, device=dev), torch.empty(P, dtype=torch.int64, device=dev)))
        for lo, d_U, cs, ks in parts:
            eng.rollout_device(d_x0.data_ptr(), d_U.data_ptr(), P, shard, n, layout, lo, cs.data_ptr(), ks.data_ptr(), s)
        torch.cuda.synchronize()
        combined = torch.minimum(parts[0][3], parts[1][3])
        records = []
        for lo, d_U, cs, ks in parts:   # each rank: its rollout (partials in the handle), then the finalize on the keys
            r = torch.empty(P, rf, device=dev)
            eng.rollout_device(d_x0.data_ptr(), d_U.data_ptr(), P, shard, n, layout, lo, cs.data_ptr(), 0, s)
            eng.finalize_device(combined.data_ptr(), d_x0.data_ptr(), d_U.data_ptr(), P, shard, n, layout, lo, r.data_ptr(), s)
            records.append(r)
        torch.cuda.synchronize()
        tgd._same_bits(np.concatenate([parts[0][2].cpu().numpy(), parts[1][2].cpu().numpy()], axis=1), whole["costs"])
        assert [_capi.key_index(int(k)) for k in combined.cpu().numpy()] == list(whole["best_idx"]), label
        r0, r1 = (r.cpu().numpy() for r in records)
        for p in range(P):
            owner, other = (r0[p], r1[p]) if r0[p][3] == 1.0 else (r1[p], r0[p])
            assert owner[3] == 1.0 and other[3] == 0.0 and not np.any(np.delete(other, 2)), "%s: problem %d" % (label, p)
            assert (r0[p][3] == 1.0) == (whole["best_idx"][p] < shard), "%s: problem %d" % (label, p)
            assert owner[2] + other[2] == whole["records"][p][2], "%s: problem %d" % (label, p)
            assert np.array_equal(np.delete(owner, 2).view(np.uint32), np.delete(whole["records"][p], 2).view(np.uint32)), \
                "%s: problem %d" % (label, p)
        for p, cands in planted.items():
            for c in cands:
                assert not np.isfinite(whole["costs"][p][c]), label
    finally:
        eng.close()
