"""Mode D's softmin (MPPI) recentring on the MI355X.  acmpc_softmin_sampled_device re-draws the candidates it averages and
must give, bit for bit, what acmpc_sample_device into a matrix + acmpc_softmin_device of it give; acmpc_optimize with
centre_update = 1 on a mode D handle, its matrix form and the loop built from device calls must give the same records;
shards of a launch combine to the unsharded mean; and the closed loop of tests/test_gpu_dynamic.py holds its bars with
the softmin update."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_spec as ds
from test_support import engine_kwargs, make_problem

pytestmark = pytest.mark.gpu

BIG_OFFSET = (1 << 31) + 12345     # global candidates 0 and 1 lie outside the slice; not a multiple of 8
SIGMA = (0.05, 0.3)
LAMBDA = 0.5


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _u64(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


def _dynamic_engine(P, N, n, seed=0, vehicles=None, window=None, **extra):
    """A mode D handle on P problems with its vehicle (or an ensemble under MEAN) and its tables set; and the problems."""
    import test_gpu_dynamic_ensemble as tge
    from acmpc_amd import Engine
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, 4, seed + p) for p in range(P)]
    eng = Engine(**dict(dps[0]["kw"], max_problems=P, max_candidates=N, max_steps=n, nn_window=window, **extra))
    fleet = tge._vehicles()
    if vehicles is None:
        eng.set_dynamics(fleet[0])
    else:
        eng.set_dynamics_ensemble([fleet[i] for i in vehicles], weights=None, reduce="mean")
    eng.set_paths(np.stack([d["table"] for d in dps]))
    return eng, dps


def _centres(dps, n, seed):
    """centre / u_ref [P, n, 2] round the paths' steering reference."""
    rng = np.random.default_rng(900 + seed)
    L = float(dps[0]["kw"]["wheelbase"])
    P = len(dps)
    centre, ref = np.empty((P, n, 2), dtype=np.float32), np.empty((P, n, 2), dtype=np.float32)
    for p, d in enumerate(dps):
        d_ref = np.arctan(L * d["table"][orc.ROW_KAPPA])[:n]
        centre[p, :, 0] = d_ref + rng.normal(0.0, 0.01, n)
        centre[p, :, 1] = rng.uniform(-0.1, 0.4)
        ref[p, :, 0] = d_ref
        ref[p, :, 1] = 0.15
    return centre, ref


def _synthetic_costs(P, N, seed):
    """Seeded costs [P, N] with NaN and +inf planted in the first, a middle and the last chunk of 1 024, the LAST problem's
    all non-finite; and the key of each problem's minimum at `index_offset` 0 (the index plays no part in the weights)."""
    from acmpc_amd import _capi
    rng = np.random.default_rng(seed)
    costs = rng.uniform(0.5, 6.0, (P, N)).astype(np.float32)
    chunks = (N + 1023) // 1024
    for chunk in sorted({0, chunks // 2, chunks - 1}):
        lo, hi = chunk * 1024, min(N, chunk * 1024 + 1024)
        if hi - lo >= 4:
            costs[:, lo + (hi - lo) // 3] = np.nan
            costs[:, hi - 1] = np.inf
            costs[0, lo] = np.inf
    if N >= 3:
        costs[0, N // 2] = np.nan
    costs[P - 1] = np.where(np.arange(N) % 2 == 0, np.nan, np.inf).astype(np.float32)
    keys = np.empty(P, dtype=np.int64)
    for p in range(P):
        best = orc.pick_best(costs[p])[0]
        keys[p] = _capi.pack_key(float(costs[p][best]), best)
    return costs, keys


def _both_forms(torch, eng, dev, s, costs, keys, centre, ref, P, N, n, offset, sigma, seed, rnd):
    """((mean, weight_sum) of acmpc_softmin_sampled_device, the same of acmpc_sample_device + acmpc_softmin_device)."""
    ref_ptr = ref.data_ptr() if ref is not None else 0
    out = []
    for sampled in (True, False):
        mean = torch.full((P, n, 2), -7.0, device=dev)
        wsum = torch.full((P,), -7.0, dtype=torch.float64, device=dev)
        if sampled:
            eng.softmin_sampled_device(costs.data_ptr(), keys.data_ptr(), centre.data_ptr(), 2 * n, ref_ptr, P, N, n, offset,
                                       sigma, seed, rnd, mean.data_ptr(), wsum.data_ptr(), s)
        else:
            U = torch.empty(P, n, 2, N, device=dev)
            eng.sample_device(centre.data_ptr(), 2 * n, ref_ptr, P, N, n, 1, offset, sigma, seed, rnd, U.data_ptr(), s)
            eng.softmin_device(costs.data_ptr(), keys.data_ptr(), U.data_ptr(), P, N, n, 1, mean.data_ptr(),
                               wsum.data_ptr(), s)
        torch.cuda.synchronize()
        out.append((mean, wsum))
    return out


# ---- 1. the kernel against the matrix form ----------------------------------------------------------------------------------
KERNEL_N = (1, 63, 64, 65, 1024, 1025, 3000)


@pytest.mark.parametrize("n", [2, 7, 49, 129, 512])
def test_sampled_softmin_is_the_matrix_softmin_bit_for_bit(n):
    """N: a lone candidate, the wave edges, a full chunk, a chunk of one, ragged chunks; n: fewer steps than knots up to the
    mode's longest horizon.  Synthetic costs (no rollout), NaN / +inf planted, one problem without a finite cost, a NaN in
    the centre; with and without u_ref; at index_offset 0 and beyond 2^31."""
    import torch
    P = 3
    eng, dps = _dynamic_engine(P, max(KERNEL_N), n, seed=10, softmin_lambda=LAMBDA)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    centre_h, ref_h = _centres(dps, n, n)
    centre_h[1, n // 2, 0] = np.nan   # (clipped to the box's lower bound by every candidate that reads it)
    centre, ref = torch.tensor(centre_h, device=dev), torch.tensor(ref_h, device=dev)
    try:
        for N in KERNEL_N:
            costs_h, keys_h = _synthetic_costs(P, N, seed=31 * n + N)
            costs, keys = torch.tensor(costs_h, device=dev), torch.tensor(keys_h, device=dev)
            for with_ref in (False, True):
                for offset in (0, BIG_OFFSET):
                    got, want = _both_forms(torch, eng, dev, s, costs, keys, centre, ref if with_ref else None, P, N, n,
                                            offset, SIGMA, 0x1234567890AB, 2)
                    what = "N=%d n=%d u_ref=%s offset=%d" % (N, n, with_ref, offset)
                    assert np.array_equal(_u32(got[0]), _u32(want[0])), "mean: " + what
                    assert np.array_equal(_u64(got[1]), _u64(want[1])), "weight sum: " + what
                    wsum = got[1].cpu().numpy()
                    assert wsum[P - 1] == 0.0 and np.all(wsum[:P - 1] > 0.0), what   # the uniform fallback, exactly 0
                    assert np.all(np.isfinite(got[0].cpu().numpy())), what
    finally:
        eng.close()


def test_sampled_softmin_on_a_mode_s_handle():
    """The sampler is the same in every mode: a mode S handle, (v, kappa) controls in its own box."""
    import torch
    P, H, N = 3, 50, 1500
    n = H - 1
    problems = [make_problem(orc, "monza", H, 4, seed=400 + p) for p in range(P)]
    from acmpc_amd import Engine
    eng = Engine(**engine_kwargs(problems[0], 0, P, N, n, softmin_lambda=LAMBDA))
    eng.set_paths(np.stack([p["table"] for p in problems]))
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    u_ref = np.stack([np.stack([p["table"][orc.ROW_V], p["table"][orc.ROW_KAPPA]], axis=1) for p in problems]).astype(np.float32)
    centre = (u_ref + np.array([-1.0, 0.002], dtype=np.float32)).astype(np.float32)
    costs_h, keys_h = _synthetic_costs(P, N, seed=5)
    costs, keys = torch.tensor(costs_h, device=dev), torch.tensor(keys_h, device=dev)
    try:
        for offset in (0, BIG_OFFSET):
            got, want = _both_forms(torch, eng, dev, s, costs, keys, torch.tensor(centre, device=dev),
                                    torch.tensor(u_ref, device=dev), P, N, n, offset, (3.0, 0.01), 99, 1)
            assert np.array_equal(_u32(got[0]), _u32(want[0])) and np.array_equal(_u64(got[1]), _u64(want[1])), offset
    finally:
        eng.close()


# ---- 2. acmpc_optimize, mode D, softmin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("vehicles", [None, (0, 1, 2)], ids=["K1", "K3-mean"])
def test_optimize_softmin_equals_its_matrix_form_and_the_manual_round_loop(vehicles):
    """Round 0 samples round the caller's centre with the caller's u_ref as candidate 1; every later round round the softmin
    mean of the round before, the previous winner as candidate 1.  Three launches per round without a matrix (the default),
    the matrix form and the loop of device calls: the same records bit for bit; the winner's cost never rises; round 0's
    mean against the oracle's weighted reduction."""
    import torch
    from acmpc_amd import _capi
    P, N, n, rounds, shrink, seed, lam = 2, 2065, 30, 3, 0.5, 4321, 1.0
    eng, dps = _dynamic_engine(P, N, n, seed=60, vehicles=vehicles, window=(2, 5), centre_update="softmin",
                               softmin_lambda=lam)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    centre_h, ref_h = _centres(dps, n, 1)
    x0_h = np.stack([d["x0"] for d in dps])
    try:
        default = eng.optimize(x0_h, centre_h, ref_h, N, rounds, SIGMA, shrink=shrink, seed=seed)["records"]
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", "1")
        matrix = eng.optimize(x0_h, centre_h, ref_h, N, rounds, SIGMA, shrink=shrink, seed=seed)["records"]
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", None)
        again = eng.optimize(x0_h, centre_h, ref_h, N, rounds, SIGMA, shrink=shrink, seed=seed)["records"]
        assert np.all(default[:, _capi.REC_OWNER] == 1.0) and np.all(np.isfinite(default[:, 0]))
        assert np.array_equal(default.view(np.uint32), matrix.view(np.uint32)), "three launches per round against the matrix"
        assert np.array_equal(again.view(np.uint32), default.view(np.uint32))

        # the manual loop (tests/test_gpu_sharded.py test_softmin_centre_update_equals_the_manual_round_loop)
        R = _capi.record_floats(n)
        d_x0, d_ref = torch.tensor(x0_h, device=dev), torch.tensor(ref_h, device=dev)
        U = torch.empty(P, n, 2, N, device=dev)
        rec = torch.empty(P, R, device=dev)
        keys = torch.empty(P, dtype=torch.int64, device=dev)
        cost = torch.empty(P, N, device=dev)
        wsum = torch.empty(P, dtype=torch.float64, device=dev)
        mean = torch.tensor(centre_h, device=dev)
        best = []
        for r in range(rounds):
            ref = d_ref if r == 0 else rec[:, _capi.REC_HEADER:_capi.REC_HEADER + 2 * n].contiguous()
            eng.sample_device(mean.data_ptr(), 2 * n, ref.data_ptr(), P, N, n, 1, 0,
                              (SIGMA[0] * shrink**r, SIGMA[1] * shrink**r), seed, r, U.data_ptr(), s)
            eng.solve_device(d_x0.data_ptr(), U.data_ptr(), P, N, n, 1, cost.data_ptr(), keys.data_ptr(), rec.data_ptr(), s)
            eng.softmin_device(cost.data_ptr(), keys.data_ptr(), U.data_ptr(), P, N, n, 1, mean.data_ptr(), wsum.data_ptr(), s)
            torch.cuda.synchronize()
            best.append(rec[:, 0].cpu().numpy().copy())
            if r == 0:
                Uh, ch = U.cpu().numpy(), cost.cpu().numpy()
                for p in range(P):
                    want = orc.softmin_mean(ch[p], np.moveaxis(Uh[p], -1, 0), lam)
                    np.testing.assert_allclose(mean[p].cpu().numpy(), want, rtol=2e-5, atol=1e-6)
                    w = orc.softmin_weights(ch[p], lam).astype(np.float64)
                    np.testing.assert_allclose(wsum[p].item(), w.sum(), rtol=1e-5)
        assert np.array_equal(default.view(np.uint32), _u32(rec)), "acmpc_optimize against the loop of device calls"
        for a, b in zip(best, best[1:]):
            assert (b <= a).all()
    finally:
        eng.close()


# ---- 3. shards ----------------------------------------------------------------------------------------------------------------
def test_four_shards_combine_to_the_unsharded_mean():
    """Four emulated ranks on one card, uneven slices at large offsets: each slice's sampled softmin equals the matrix softmin
    of that slice bit for bit, and the payloads combined in rank order equal the unsharded launch's mean to float32
    rounding (the bars of test_softmin_over_shards_equals_the_unsharded_mean)."""
    import torch
    from acmpc_amd.sharding import combine_softmin, softmin_payload
    P, N, n, seed, rnd = 2, 3000, 30, 77, 1
    base = 3_000_000_013
    cuts = [0, 700, 1724, 1725, N]     # 700, a full chunk, one candidate, 1 275
    eng, dps = _dynamic_engine(P, N, n, seed=70, softmin_lambda=LAMBDA)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    centre_h, ref_h = _centres(dps, n, 2)
    centre, ref = torch.tensor(centre_h, device=dev), torch.tensor(ref_h, device=dev)
    x0 = torch.tensor(np.stack([d["x0"] for d in dps]), device=dev)

    def rollout(offset, count):
        costs = torch.empty(P, count, device=dev)
        keys = torch.empty(P, dtype=torch.int64, device=dev)
        eng.rollout_sampled_device(x0.data_ptr(), centre.data_ptr(), 2 * n, ref.data_ptr(), P, count, n, offset, SIGMA, seed,
                                   rnd, costs.data_ptr(), keys.data_ptr(), s)
        torch.cuda.synchronize()
        return costs, keys

    try:
        costs_full, keys_full = rollout(base, N)
        mean_full = torch.empty(P, n, 2, device=dev)
        wsum_full = torch.empty(P, dtype=torch.float64, device=dev)
        eng.softmin_sampled_device(costs_full.data_ptr(), keys_full.data_ptr(), centre.data_ptr(), 2 * n, ref.data_ptr(), P, N,
                                   n, base, SIGMA, seed, rnd, mean_full.data_ptr(), wsum_full.data_ptr(), s)
        torch.cuda.synchronize()
        slices = [(base + lo, hi - lo) + rollout(base + lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
        gkeys = torch.stack([sl[3] for sl in slices]).min(dim=0).values.contiguous()   # what all-reduce(MIN) leaves
        assert torch.equal(gkeys, keys_full)
        payloads = []
        for offset, count, costs, _ in slices:
            got, want = _both_forms(torch, eng, dev, s, costs, gkeys, centre, ref, P, count, n, offset, SIGMA, seed, rnd)
            assert np.array_equal(_u32(got[0]), _u32(want[0])) and np.array_equal(_u64(got[1]), _u64(want[1])), (offset, count)
            payloads.append(softmin_payload(got[0], got[1], count))
        mean, wsum = combine_softmin(payloads, n)
        torch.cuda.synchronize()
        np.testing.assert_allclose(mean.cpu().numpy(), mean_full.cpu().numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(wsum.cpu().numpy(), wsum_full.cpu().numpy(), rtol=1e-12)
        assert np.all(wsum.cpu().numpy() > 0.0)
    finally:
        eng.close()


@pytest.mark.parametrize("vehicles", [None, (0, 1, 2)], ids=["K1", "K3-mean"])
def test_sharded_optimizer_softmin_at_world_size_one_is_optimize(vehicles):
    import torch
    from acmpc_amd.sharding import ShardedOptimizer
    P, N, n, rounds, shrink, seed = 2, 2065, 30, 3, 0.5, 99
    eng, dps = _dynamic_engine(P, N, n, seed=80, vehicles=vehicles, window=(2, 5), centre_update="softmin",
                               softmin_lambda=1.0)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    centre_h, ref_h = _centres(dps, n, 3)
    x0_h = np.stack([d["x0"] for d in dps])
    try:
        for ref in (ref_h, None):
            want = eng.optimize(x0_h, centre_h, ref, N, rounds, SIGMA, shrink=shrink, seed=seed)["records"]
            opt = ShardedOptimizer(eng, P, N, n, 0, dev, centre_update="softmin")
            assert opt.U is None                                  # no control matrix on a mode D engine
            rec = opt.solve(torch.tensor(x0_h, device=dev), torch.tensor(centre_h, device=dev),
                            torch.tensor(ref, device=dev) if ref is not None else None, rounds, SIGMA, shrink=shrink,
                            seed=seed, stream=s)
            torch.cuda.synchronize()
            assert np.array_equal(_u32(rec), want.view(np.uint32)), "u_ref given" if ref is not None else "no u_ref"
    finally:
        eng.close()


def test_sharded_optimizer_softmin_on_a_mode_s_engine_is_optimize():
    """Modes S and T sample into U and take the matrix softmin: at world size 1 the records of acmpc_optimize."""
    import torch
    from acmpc_amd import Engine
    from acmpc_amd.sharding import ShardedOptimizer
    P, H, N, rounds = 2, 50, 2048, 3
    n = H - 1
    problems = [make_problem(orc, "silverstone", H, 4, seed=520 + p) for p in range(P)]
    eng = Engine(**engine_kwargs(problems[0], 0, P, N, n, centre_update="softmin"))
    eng.set_paths(np.stack([p["table"] for p in problems]))
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    u_ref = np.stack([np.stack([p["table"][orc.ROW_V], p["table"][orc.ROW_KAPPA]], axis=1) for p in problems]).astype(np.float32)
    x0 = np.stack([p["x0"] for p in problems])
    try:
        want = eng.optimize(x0, u_ref, u_ref, N, rounds, (3.0, 0.01), shrink=0.5, seed=43)["records"]
        opt = ShardedOptimizer(eng, P, N, n, 0, dev, centre_update="softmin")
        d_ref = torch.tensor(u_ref, device=dev)
        rec = opt.solve(torch.tensor(x0, device=dev), d_ref, d_ref, rounds, (3.0, 0.01), shrink=0.5, seed=43, stream=s)
        torch.cuda.synchronize()
        assert np.array_equal(_u32(rec), want.view(np.uint32))
    finally:
        eng.close()


# ---- 4. closed loop -------------------------------------------------------------------------------------------------------------
def test_dynamic_sampling_solver_closed_loop_with_the_softmin_update():
    """tests/test_gpu_dynamic.py's loop and bars with sampling_update = "softmin", lambda = 1 (measured on the MI355X:
    DESIGN.md section 6)."""
    from acmpc_amd import DynamicBicycleParams, DynamicSamplingSolver
    from test_gpu_dynamic import LOOP_CONFIG, LOOP_H, check_loop, run_loop
    plant = DynamicBicycleParams.reference()
    solver = DynamicSamplingSolver(dict(LOOP_CONFIG, sampling_update="softmin", softmin_lambda=1.0), plant)
    n = LOOP_H - 1

    def solve(state, table):
        obj = solver.solve(state, table)
        u = obj.x[3 * (n + 1):].reshape(n, 2)
        assert np.all(np.abs(u[:, 0]) <= 0.3) and np.all(np.abs(u[:, 1]) <= 1.0)
        return obj

    try:
        log = run_loop(solve, plant)
        ey, slip, dv, idx = log.T
        print("softmin loop: max |e_y| %.3f m, mean |e_y| %.3f m, sideslip %.4f, speed error %.3f m/s, travelled %d m"
              % (np.abs(ey).max(), np.abs(ey).mean(), slip.max(), np.abs(dv[40:]).max(), ((idx[-1] - idx[0]) % 11586) // 2))
        check_loop(log)
    finally:
        solver.close()
