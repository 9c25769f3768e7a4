"""Mode D's sampled call forms on the MI355X.  acmpc_rollout_sampled_device draws its candidates inside the rollout kernel;
acmpc_finalize_sampled_device / acmpc_solve_sampled_device re-draw the winner from the index in its key; acmpc_optimize and
ShardedOptimizer are built from the two.  Each must give, bit for bit (non-finite values included), what the control
matrix gives: acmpc_sample_device into a matrix, acmpc_rollout_device of it, acmpc_finalize_device on it - and, on a small
shape, what tests/dynamic_sampled_spec.py gives alone."""
import os

import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_sampled_spec as dss
import dynamic_spec as ds
import test_gpu_dynamic_ensemble as tge

pytestmark = pytest.mark.gpu

BIG_OFFSET = 3_000_000_013     # not a multiple of 8: amplitudes cycle from 6/8, candidates 0 and 1 lie outside the shard
ENSEMBLES = {1: ((0,), None, "mean"), 4: ((0, 1, 2, 4), (1.0, 2.0, 0.5, 1.5), "mean"), 3: ((0, 3, 2), None, "max"),
             2: ((0, 1), None, "mean")}
KIND = [dict(), dict(vx0=0.0), dict(yaw_turns=-1), dict(origin=(3000.0, 2700.0))]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same_bits(got, want, message=""):
    assert np.array_equal(_bits(got), _bits(want)), message


class Rig:
    """A mode D engine on P problems with its device buffers: centre / u_ref [P, n, 2], x0 [P, 6]."""

    def __init__(self, P, N, n, K=1, window=None, seed=0, with_ref=True, track="monza", kinds=None, vehicles=None,
                 weights=None, reduce=None):
        import torch
        from acmpc_amd import Engine
        self.torch = torch
        self.P, self.N, self.n, self.K, self.window = P, N, n, K, window
        kinds = kinds if kinds is not None else [p % 4 for p in range(P)]
        # (the problems' own candidate matrices are not used: 4 candidates keep their construction cheap)
        self.dps = [ds.make_dynamic_problem(orc, track, n + 1, 4, seed + p, **KIND[kind]) for p, kind in enumerate(kinds)]
        idx, w, red = ENSEMBLES[K] if vehicles is None else (vehicles, weights, reduce)
        self.vehicle_index, self.weights, self.reduce = tuple(idx), w, red
        eng = Engine(**dict(self.dps[0]["kw"], max_problems=P, max_candidates=N, max_steps=n, nn_window=window))
        try:
            fleet = tge._vehicles()
            if len(idx) == 1:
                eng.set_dynamics(fleet[idx[0]])
            else:
                eng.set_dynamics_ensemble([fleet[i] for i in idx], weights=w, reduce=red)
            eng.set_paths(np.stack([d["table"] for d in self.dps]))
        except Exception:
            eng.close()
            raise
        self.eng = eng
        self.dev = torch.device("cuda", 0)
        self.s = torch.cuda.current_stream().cuda_stream
        rng = np.random.default_rng(777 + seed)
        L = float(self.dps[0]["kw"]["wheelbase"])
        centre = np.empty((P, n, 2), dtype=np.float32)
        ref = np.empty((P, n, 2), dtype=np.float32)
        for p, d in enumerate(self.dps):
            d_ref = np.arctan(L * d["table"][orc.ROW_KAPPA])[:n]
            centre[p, :, 0] = d_ref + rng.normal(0.0, 0.01, n)
            centre[p, :, 1] = rng.uniform(-0.1, 0.4)
            ref[p, :, 0] = d_ref
            ref[p, :, 1] = 0.15
        self.centre_h, self.ref_h = centre, (ref if with_ref else None)
        self.x0_h = np.stack([d["x0"] for d in self.dps])
        self.upload()

    def upload(self):
        t = self.torch
        self.centre = t.tensor(self.centre_h, device=self.dev)
        self.ref = t.tensor(self.ref_h, device=self.dev) if self.ref_h is not None else None
        self.x0 = t.tensor(self.x0_h, device=self.dev)

    @property
    def ref_ptr(self):
        return self.ref.data_ptr() if self.ref is not None else 0

    def blocks(self):
        return [tge._vehicles()[i].coefficients() for i in self.vehicle_index]

    def matrix(self, N, offset, sigma, seed, rnd):
        """acmpc_sample_device into a step-major matrix, acmpc_rollout_device of it: (U, costs, keys)"""
        t, e = self.torch, self.eng
        U = t.empty(self.P, self.n, 2, N, device=self.dev)
        costs = t.empty(self.P, N, device=self.dev)
        keys = t.empty(self.P, dtype=t.int64, device=self.dev)
        e.sample_device(self.centre.data_ptr(), 2 * self.n, self.ref_ptr, self.P, N, self.n, 1, offset, sigma, seed, rnd,
                        U.data_ptr(), self.s)
        e.rollout_device(self.x0.data_ptr(), U.data_ptr(), self.P, N, self.n, 1, offset, costs.data_ptr(), keys.data_ptr(),
                         self.s)
        t.cuda.synchronize()
        return U, costs, keys

    def fused(self, N, offset, sigma, seed, rnd, want_costs=True, want_keys=True):
        """acmpc_rollout_sampled_device: (costs, keys)"""
        t, e = self.torch, self.eng
        costs = t.empty(self.P, N, device=self.dev) if want_costs else None
        keys = t.empty(self.P, dtype=t.int64, device=self.dev) if want_keys else None
        e.rollout_sampled_device(self.x0.data_ptr(), self.centre.data_ptr(), 2 * self.n, self.ref_ptr, self.P, N, self.n,
                                 offset, sigma, seed, rnd, costs.data_ptr() if want_costs else 0,
                                 keys.data_ptr() if want_keys else 0, self.s)
        t.cuda.synchronize()
        return costs, keys

    def finalize_sampled(self, keys, N, sigma, seed, rnd):
        from acmpc_amd import _capi
        t = self.torch
        rec = t.empty(self.P, _capi.record_floats(self.n), device=self.dev)
        self.eng.finalize_sampled_device(keys.data_ptr() if keys is not None else 0, self.x0.data_ptr(),
                                         self.centre.data_ptr(), 2 * self.n, self.ref_ptr, self.P, N, self.n, sigma, seed, rnd,
                                         rec.data_ptr(), self.s)
        t.cuda.synchronize()
        return rec.cpu().numpy()

    def finalize_matrix(self, keys, U, N, offset):
        from acmpc_amd import _capi
        t = self.torch
        rec = t.empty(self.P, _capi.record_floats(self.n), device=self.dev)
        self.eng.finalize_device(keys.data_ptr(), self.x0.data_ptr(), U.data_ptr(), self.P, N, self.n, 1, offset,
                                 rec.data_ptr(), self.s)
        t.cuda.synchronize()
        return rec.cpu().numpy()

    def close(self):
        self.eng.close()


def _compare_rollouts(rig, N, offset, sigma, seed, rnd, label=""):
    """item 1: the fused rollout against sample + rollout through the matrix.  Returns what both computed."""
    U, costs_m, keys_m = rig.matrix(N, offset, sigma, seed, rnd)
    costs_f, keys_f = rig.fused(N, offset, sigma, seed, rnd)
    _same_bits(costs_f.cpu().numpy(), costs_m.cpu().numpy(), label + ": costs")
    assert np.array_equal(keys_f.cpu().numpy(), keys_m.cpu().numpy()), label + ": keys"
    _, keys_only = rig.fused(N, offset, sigma, seed, rnd, want_costs=False)   # d_costs NULL: the same keys
    assert np.array_equal(keys_only.cpu().numpy(), keys_m.cpu().numpy()), label + ": keys without costs"
    return U, costs_m, keys_m


def _compare_records(rig, U, keys, N, offset, sigma, seed, rnd, label=""):
    """the re-drawing finalize (on the handle's partial keys of a fused rollout of this shard, and on the keys handed in)
    against acmpc_finalize_device on the sampled matrix (whose shard owns the winner: a full record too)."""
    rig.fused(N, offset, sigma, seed, rnd, want_costs=False, want_keys=False)
    rec_partial = rig.finalize_sampled(None, N, sigma, seed, rnd)
    rec_keys = rig.finalize_sampled(keys, N, sigma, seed, rnd)
    rig.matrix(N, offset, sigma, seed, rnd)     # (the handle's partial counts are this shard's either way)
    rec_matrix = rig.finalize_matrix(keys, U, N, offset)
    _same_bits(rec_partial, rec_matrix, label + ": record from the partial keys")
    _same_bits(rec_keys, rec_matrix, label + ": record from the reduced keys")
    assert np.all(rec_matrix[:, 3] == 1.0), label
    return rec_matrix


# ---- 1. the fused rollout = sample + rollout ---------------------------------------------------------------------------
# (P, N, n, K, window, with_ref, round, offset): P in {1, 3}; N not a multiple of 256, N odd; n in {8, 30, 49, 200}; with and
# without u_ref; round != 0; the large offset; windowed and exhaustive; K = 1, 4 (MEAN), 3 (MAX); P N K >= 2^20 (two
# candidates per lane) for K = 1, 4 and 3, with odd N (the last pair's second lane repeats N - 1)
ROLLOUT_CASES = [
    (1, 1000, 8, 1, None, True, 0, 0),
    (3, 1537, 30, 1, (2, 5), False, 2, 0),
    (1, 1000, 49, 1, (2, 5), True, 1, BIG_OFFSET),
    (3, 300, 200, 1, None, True, 3, BIG_OFFSET),
    (1, 257, 200, 1, (20, 43), False, 0, 5),
    (3, 1000, 49, 4, (2, 5), True, 0, 0),
    (1, 1537, 30, 4, None, False, 5, BIG_OFFSET),
    (3, 131, 8, 3, None, True, 1, 0),
    (1, 1000, 49, 3, (2, 5), True, 2, BIG_OFFSET),
    (1, 63, 200, 3, (1, 2), False, 0, 1),
    (1, (1 << 20) + 1, 8, 1, (2, 5), True, 1, 0),
    (3, 349527, 8, 1, None, True, 0, BIG_OFFSET),
    (1, 262147, 8, 4, (2, 5), True, 2, 0),
    (1, 349527, 8, 3, None, False, 1, BIG_OFFSET),
]


@pytest.mark.parametrize("P,N,n,K,window,with_ref,rnd,offset", ROLLOUT_CASES)
def test_fused_rollout_equals_sample_then_rollout(P, N, n, K, window, with_ref, rnd, offset):
    rig = Rig(P, N, n, K=K, window=window, seed=100 + n, with_ref=with_ref)
    try:
        sigma, seed = (0.04, 0.35), 0xC0FFEE1234
        U, costs, keys = _compare_rollouts(rig, N, offset, sigma, seed, rnd)
        if K != 3:     # (K = 3 holds the vehicle whose costs are huge or non-finite; the others must give real costs)
            assert np.isfinite(costs.cpu().numpy()).mean() > 0.5
        _compare_records(rig, U, keys, N, offset, sigma, seed, rnd)
    finally:
        rig.close()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("window", [None, (2, 5)])
def test_fused_rollout_equals_the_specification(K, window):
    """One small shape against tests/dynamic_sampled_spec.py alone: candidates, costs, key, feasible count, record."""
    from acmpc_amd import _capi
    P, N, n, sigma, seed, rnd = 2, 130, 8, (0.05, 0.3), 99, 3
    rig = Rig(P, N, n, K=K, window=window, seed=40, with_ref=True)
    try:
        for offset in (0, BIG_OFFSET):
            costs, keys = rig.fused(N, offset, sigma, seed, rnd)
            rec = rig.finalize_sampled(None, N, sigma, seed, rnd)
            for p in range(P):
                want = dss.rollout_sampled(orc, rig.dps[p], rig.eng.coefficients(p), rig.blocks(), rig.centre_h[p],
                                           rig.ref_h[p], N, offset, p, rnd, seed, sigma, reduce=rig.reduce,
                                           weights=rig.weights, nn_window=window, return_states=True)
                _same_bits(costs[p].cpu().numpy(), want["cost"], "costs, problem %d" % p)
                assert int(keys[p].item()) == want["key"]
                r = _capi.split_record(rec[p], n)
                best = want["best"]
                assert r["owner"] == 1.0 and r["n_feasible"] == want["n_feasible"]
                _same_bits(r["cost"], want["cost"][best])
                _same_bits(r["violation"], want["violation"][best])
                _same_bits(r["u"], want["U"][best])
                _same_bits(r["x"], want["x"][best])
    finally:
        rig.close()


# ---- 2. the re-drawing finalize, four emulated shards --------------------------------------------------------------------
@pytest.mark.parametrize("K,window,with_ref", [(1, (2, 5), True), (1, None, False), (3, (2, 5), True)])
def test_four_shards_end_with_the_unsharded_record(K, window, with_ref):
    from acmpc_amd import _capi
    from acmpc_amd.sharding import shard_range
    import torch
    P, N, n, sigma, seed, rnd = 3, 4102, 30, (0.05, 0.3), 4242, 1
    rig = Rig(P, N, n, K=K, window=window, seed=60, with_ref=with_ref)
    try:
        U, costs, keys = _compare_rollouts(rig, N, 0, sigma, seed, rnd)
        whole = _compare_records(rig, U, keys, N, 0, sigma, seed, rnd)
        slices = [shard_range(N, r, 4) for r in range(4)]
        assert sum(c for _, c in slices) == N and len({c for _, c in slices}) == 2
        shard_keys, shard_costs = [], []
        for off, count in slices:
            c, k = rig.fused(count, off, sigma, seed, rnd)
            shard_keys.append(k.cpu().numpy())
            shard_costs.append(c.cpu().numpy())
        _same_bits(np.concatenate(shard_costs, axis=1), costs.cpu().numpy())
        reduced_h = np.minimum.reduce(shard_keys)                 # the all-reduce(MIN), on the host
        assert np.array_equal(reduced_h, keys.cpu().numpy())
        reduced = torch.tensor(reduced_h, device=rig.dev)
        recs = []
        for off, count in slices:   # each rank: its own rollout (partial counts in the handle), then the finalize on the keys
            rig.fused(count, off, sigma, seed, rnd, want_costs=False, want_keys=False)
            recs.append(rig.finalize_sampled(reduced, count, sigma, seed, rnd))
        foreign = 0
        for p in range(P):
            winner = _capi.key_index(int(reduced_h[p]))
            for (off, count), rec in zip(slices, recs):
                foreign += not (off <= winner < off + count)      # a rank finalizing a winner it never rolled
                assert rec[p][3] == 1.0
                _same_bits(np.delete(rec[p], 2), np.delete(whole[p], 2), "problem %d, shard at %d" % (p, off))
            assert sum(float(rec[p][2]) for rec in recs) == float(whole[p][2])
        assert foreign == 3 * P
    finally:
        rig.close()


# ---- 3. acmpc_solve_sampled_device = rollout + the re-drawing finalize ------------------------------------------------------
@pytest.mark.parametrize("K,layout", [(1, 1), (1, 0), (4, 1)])
def test_solve_sampled_equals_rollout_then_finalize_sampled(K, layout):
    from acmpc_amd import _capi
    import torch
    P, N, n, sigma, seed, rnd = 3, 1537, 49, (0.05, 0.3), 17, 2
    rig = Rig(P, N, n, K=K, window=(2, 5), seed=80, with_ref=True)
    try:
        U, costs_m, keys_m = rig.matrix(N, 0, sigma, seed, rnd)
        want = rig.finalize_sampled(None, N, sigma, seed, rnd)     # on the partial keys rig.matrix's rollout left
        U_in = U if layout == 1 else U.permute(0, 3, 1, 2).contiguous()
        costs = torch.empty(P, N, device=rig.dev)
        keys = torch.empty(P, dtype=torch.int64, device=rig.dev)
        rec = torch.empty(P, _capi.record_floats(n), device=rig.dev)
        rig.eng.solve_sampled_device(rig.x0.data_ptr(), U_in.data_ptr(), rig.centre.data_ptr(), 2 * n, rig.ref_ptr, P, N, n,
                                     layout, sigma, seed, rnd, costs.data_ptr(), keys.data_ptr(), rec.data_ptr(), rig.s)
        torch.cuda.synchronize()
        _same_bits(costs.cpu().numpy(), costs_m.cpu().numpy())
        assert np.array_equal(keys.cpu().numpy(), keys_m.cpu().numpy())
        _same_bits(rec.cpu().numpy(), want)
        _same_bits(rec.cpu().numpy(), rig.finalize_matrix(keys_m, U, N, 0))
    finally:
        rig.close()


# ---- 4. / 5. acmpc_optimize with and without the matrix, ShardedOptimizer at world size 1 --------------------------------
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("with_ref", [False, True])
def test_optimize_with_and_without_the_matrix_and_the_sharded_optimizer(K, with_ref):
    from acmpc_amd.sharding import ShardedOptimizer
    import torch
    P, N, n, rounds, sigma, shrink, seed = 2, 2049, 30, 3, (0.05, 0.3), 0.5, 1234
    rig = Rig(P, N, n, K=K, window=(2, 5), seed=90, with_ref=with_ref)
    try:
        fused = rig.eng.optimize(rig.x0_h, rig.centre_h, rig.ref_h, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        rig.eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", "1")
        matrix = rig.eng.optimize(rig.x0_h, rig.centre_h, rig.ref_h, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        rig.eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", None)
        again = rig.eng.optimize(rig.x0_h, rig.centre_h, rig.ref_h, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        _same_bits(fused, matrix, "two launches per round against three")
        _same_bits(again, matrix)
        assert np.all(fused[:, 3] == 1.0) and np.all(np.isfinite(fused[:, 0]))
        opt = ShardedOptimizer(rig.eng, P, N, n, 0, rig.dev)
        assert opt.U is None                                  # no control matrix on a mode D engine
        rec = opt.solve(rig.x0, rig.centre, rig.ref, rounds, sigma, shrink=shrink, seed=seed, stream=rig.s)
        torch.cuda.synchronize()
        _same_bits(rec.cpu().numpy(), matrix, "ShardedOptimizer at world size 1")
    finally:
        rig.close()


# ---- 6. non-finite entries in the centre and in u_ref --------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_planted_non_finite_centre_and_reference(K):
    P, N, n, sigma, seed, rnd = 3, 1000, 30, (0.05, 0.3), 5, 1
    rig = Rig(P, N, n, K=K, window=(2, 5), seed=120, with_ref=True)
    try:
        rig.centre_h[0, 7, 0] = np.nan       # every drawn candidate of problem 0 carries it: fmax / fmin clip it to the box
        rig.centre_h[1, 3, 1] = np.inf
        rig.centre_h[1, 20, 0] = -np.inf
        rig.ref_h[2, 11, 1] = np.nan         # candidate 1 of problem 2 only
        rig.ref_h[0, 0, 0] = np.inf
        rig.upload()
        U, costs, keys = _compare_rollouts(rig, N, 0, sigma, seed, rnd)
        _compare_records(rig, U, keys, N, 0, sigma, seed, rnd)
        _compare_rollouts(rig, N - 1, BIG_OFFSET, sigma, seed, rnd)
    finally:
        rig.close()


# ---- 7. random shapes ----------------------------------------------------------------------------------------------------
HORIZONS = [3, 4, 9, 17, 33, 50, 65, 66, 100, 130, 257, 513]
CANDIDATES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1000, 2049]
WINDOWS = [None, (2, 5), (1, 2), (0, 2), (3, 12), (20, 43)]
TRACKS = ["monza", "spa", "nordschleife", "silverstone"]
ENSEMBLE_SIZES = [1, 1, 2, 3, 5, 8]


def _case(rng):
    H = int(rng.choice(HORIZONS))
    K = int(rng.choice(ENSEMBLE_SIZES))
    return dict(H=H, N=int(rng.choice(CANDIDATES)), P=int(rng.integers(1, 5)), window=WINDOWS[int(rng.integers(0, 6))],
                track=TRACKS[int(rng.integers(0, 4))], kinds=[int(k) for k in rng.integers(0, 4, 4)], K=K,
                vehicles=[int(v) for v in rng.permutation(8)][:K], reduce=["mean", "max"][int(rng.integers(0, 2))],
                weights=[float(x) for x in rng.uniform(0.2, 3.0, K)] if rng.integers(0, 2) else None,
                with_ref=bool(rng.integers(0, 2)), rnd=int(rng.integers(0, 5)),
                offset=[0, 0, 1, 9, BIG_OFFSET, int(rng.integers(0, (1 << 32) - 4096))][int(rng.integers(0, 6))],
                sigma=(float(rng.uniform(0.0, 0.1)), float(rng.uniform(0.0, 0.6))), seed=int(rng.integers(0, 1 << 62)))


LONGEST = [dict(H=513, N=257, P=2, window=(20, 43), track="silverstone", kinds=[3, 1], K=1, vehicles=[0], reduce="mean",
                weights=None, with_ref=True, rnd=1, offset=0, sigma=(0.05, 0.3), seed=11),
           dict(H=513, N=129, P=1, window=None, track="monza", kinds=[0], K=8, vehicles=list(range(8)), reduce="max",
                weights=None, with_ref=True, rnd=0, offset=BIG_OFFSET, sigma=(0.05, 0.3), seed=12)]


def test_random_shapes_fused_against_the_matrix():
    """Every case is compared (costs, keys and records); nothing is skipped.  ACMPC_FUZZ_CASES sets the
    number of random cases (default 40) behind the two at the 512-step limit."""
    cases = int(os.environ.get("ACMPC_FUZZ_CASES", "40"))
    rng = np.random.default_rng(20261017)
    todo = [("longest %d" % i, c) for i, c in enumerate(LONGEST)] + [(str(i), _case(rng)) for i in range(cases)]
    compared = 0
    for index, c in todo:
        label = "case %s: %r" % (index, c)
        n = c["H"] - 1
        rig = Rig(c["P"], c["N"], n, K=c["K"], window=c["window"], seed=17000 + 10 * compared, with_ref=c["with_ref"],
                  track=c["track"], kinds=c["kinds"][:c["P"]], vehicles=c["vehicles"], weights=c["weights"],
                  reduce=c["reduce"])
        try:
            U, costs, keys = _compare_rollouts(rig, c["N"], c["offset"], c["sigma"], c["seed"], c["rnd"], label)
            _compare_records(rig, U, keys, c["N"], c["offset"], c["sigma"], c["seed"], c["rnd"], label)
            compared += 1
        finally:
            rig.close()
    assert compared == len(todo)
