"""Mode D's rate and slip terms (acmpc_set_dynamics_terms, acmpc_set_previous_control) on the MI355X, from every call
form.  Costs, keys, feasible counts and records must be bit-identical to tests/dynamic_spec.py - alone on the small
shapes, and through the forms already held to it (the one-candidate-per-lane kernels, the control matrix) on the large
ones; a handle whose terms are off must give the bits of a handle that never heard of the calls; and
DynamicSamplingSolver with the terms steers more smoothly through the tightest corner of the loop of test_gpu_dynamic,
inside the rate limit it was given."""
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

pytestmark = pytest.mark.gpu

T = np.float32
INF = float("inf")
BLEND = (3.0, 5.0)
DEFAULT, FINE = (1, None), (3, BLEND)
BIG_OFFSET = tsm.BIG_OFFSET
SETTINGS = {
    "rate": dict(rate_weight=(0.3, 0.02), rate_max=None, slip_weight=0.0, slip_max=None),
    "slip": dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=40.0, slip_max=None),
    "both": dict(rate_weight=(0.3, 0.02), rate_max=(1.5, 6.0), slip_weight=40.0, slip_max=0.08),
    "limits": dict(rate_weight=(0.0, 0.0), rate_max=(1.5, 6.0), slip_weight=0.0, slip_max=0.08),
    "weights": dict(rate_weight=(0.3, 0.02), rate_max=(INF, INF), slip_weight=40.0, slip_max=INF),
}
BOTH = SETTINGS["both"]


def _vehicle():
    from acmpc_amd import DynamicBicycleParams
    return DynamicBicycleParams.reference()


def _previous(P, seed, nan_at=None):
    """[P, 2] previous controls inside the input box; `nan_at`: that problem's steering is a NaN."""
    rng = np.random.default_rng(8800 + seed)
    u = np.column_stack([rng.uniform(-0.1, 0.1, P), rng.uniform(-0.3, 0.5, P)]).astype(T)
    if nan_at is not None:
        u[nan_at, 0] = np.nan
    return u


# ---- one candidate per lane ---------------------------------------------------------------------------------------------
# P = 2, N = 300 (one full 256-lane workgroup and a tail), n = 12.  Layout 0 starts its problems at a standstill and at the
# path's speed, layout 1 inside the blend interval and at the path's speed.  A NaN pedal, an inf steering angle, and in one
# of the previous controls a NaN.  The slip part alone runs with that one only: it must not read it.
# (indices into the test's previous controls: None = none set, 1 = finite, 2 = a NaN in problem 1's)
PREVIOUS = {"rate": (None, 1, 2), "slip": (2,), "both": (None, 1, 2), "limits": (None, 1), "weights": (1, 2)}


@pytest.mark.parametrize("integration", [DEFAULT, FINE], ids=["euler", "M3-blend"])
@pytest.mark.parametrize("layout,window", [(0, None), (1, (2, 5)), (1, None), (0, (2, 5))])
def test_costs_argmin_and_record_are_the_specification(layout, window, integration):
    from acmpc_amd import _capi
    P, N, n = 2, 300, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 700 + p, vx0=v) for p, v in enumerate(((0.0, 4.0)[layout], None))]
    dps[0]["U"][5, n // 2, 1] = np.nan
    dps[1]["U"][7, 0, 0] = np.inf
    previous = (None, _previous(P, 1), _previous(P, 2, nan_at=1))
    eng = tgd._engine(dps, P, N, n, window)
    try:
        eng.set_dynamics_integration(*integration)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        x0 = np.stack([d["x0"] for d in dps])
        seen = set()
        for name, terms in SETTINGS.items():
            eng.set_dynamics_terms(**terms)
            for which in PREVIOUS[name]:
                u_prev = previous[which] if which is not None else None
                eng.set_previous_control(u_prev)
                out = eng.solve(x0, U_in, layout=layout)
                for p in range(P):
                    cost, V, X = ds.spec_costs(orc, dps[p], eng.coefficients(p), _vehicle().coefficients(), nn_window=window,
                                               return_states=True, settings=Settings(*integration, **terms),
                                               u_prev=None if u_prev is None else u_prev[p])
                    label = "%s, previous control %s, problem %d" % (name, which, p)
                    tgd._same_bits(out["costs"][p], cost)
                    rec = _capi.split_record(out["records"][p], n)
                    best = tgd._check_record(rec, U_h[p], cost, V, X, n)
                    assert out["best_idx"][p] == best, label
                    assert out["n_feasible"][p] == np.count_nonzero(V == 0), label
                    # the finalize's re-roll gives the rollout's own cost
                    tgd._same_bits(rec["cost"], out["costs"][p][best])
                    seen.add((name, bool(np.isnan(cost).all()), int(np.count_nonzero(V == 0)) > 0))
                assert np.isnan(out["costs"][0][5]) and not np.isfinite(out["costs"][1][7])
        # a NaN previous control makes every cost of its problem a NaN where the rate part is on - and none where it is off
        assert ("rate", True, True) in seen or ("rate", True, False) in seen
        assert not any(all_nan for name, all_nan, _ in seen if name == "slip")
    finally:
        eng.close()


# ---- ensembles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integration", [DEFAULT, FINE], ids=["euler", "M3-blend"])
@pytest.mark.parametrize("reduce,layout,window", [("mean", 0, None), ("max", 1, (2, 5))])
def test_ensemble_is_the_specification(reduce, layout, window, integration):
    """K = 3: two grips and a longer car (another lr: the slip part differs per vehicle, the rate part does not)."""
    from acmpc_amd import _capi
    P, N, n = 2, 130, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 720 + p, vx0=v) for p, v in enumerate((0.0, None))]
    dps[0]["U"][5, n // 2, 1] = np.nan
    vehicles = [_vehicle(), dataclasses.replace(_vehicle(), lf=1.9, lr=1.1).with_grip(0.6), _vehicle().with_grip(1.3)]
    blocks = [v.coefficients() for v in vehicles]
    weights = (1.0, 2.0, 0.5) if reduce == "mean" else None
    u_prev = _previous(P, 3)
    eng = tge._engine(dps, P, N, n, window)
    try:
        eng.set_dynamics_terms(**BOTH)            # before the vehicles: the setting does not depend on them
        eng.set_previous_control(u_prev)
        eng.set_dynamics_ensemble(vehicles, weights=weights, reduce=reduce)
        eng.set_dynamics_integration(*integration)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        out = eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)
        for p in range(P):
            J, V, X = es.spec_ensemble(orc, dps[p], eng.coefficients(p), blocks, reduce=reduce, weights=weights, nn_window=window,
                                       return_states=True, settings=Settings(*integration, **BOTH), u_prev=u_prev[p])
            tgd._same_bits(out["costs"][p], J)
            best = tgd._check_record(_capi.split_record(out["records"][p], n), U_h[p], J, V, X, n)
            assert out["best_idx"][p] == best
            # the slip part does differ per vehicle: the longer car alone gives other costs
            alone = ds.spec_costs(orc, dps[p], eng.coefficients(p), blocks[1], nn_window=window, settings=Settings(*integration,
                                  **BOTH), u_prev=u_prev[p])[0]
            assert not np.array_equal(alone.view(np.uint32), J.view(np.uint32))
    finally:
        eng.close()


def test_ensemble_of_one_is_the_single_vehicle():
    P, N, n = 2, 130, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 740 + p, vx0=v) for p, v in enumerate((1.0, None))]
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    eng = tge._engine(dps, P, N, n, (2, 5))
    try:
        eng.set_dynamics_terms(**BOTH)
        eng.set_previous_control(_previous(P, 4))
        eng.set_dynamics(_vehicle())
        single = eng.solve(x0, U)
        eng.set_dynamics_ensemble([_vehicle()], reduce="mean")
        one = eng.solve(x0, U)
        assert np.array_equal(one["costs"].view(np.uint32), single["costs"].view(np.uint32))
        assert np.array_equal(one["records"].view(np.uint32), single["records"].view(np.uint32))
    finally:
        eng.close()


# ---- the sampled forms and acmpc_optimize -----------------------------------------------------------------------------------
def _rig(P, N, n, K, window, seed, integration, terms=BOTH, **kw):
    rig = tsm.Rig(P, N, n, K=K, window=window, seed=seed, **kw)
    rig.u_prev = _previous(P, seed)
    rig.eng.set_dynamics_integration(*integration)
    rig.eng.set_dynamics_terms(**terms)
    rig.eng.set_previous_control(rig.u_prev)
    return rig


@pytest.mark.parametrize("P,N,n,K,window,with_ref,rnd,offset,integration", [
    (3, 1537, 30, 1, (2, 5), True, 2, 0, DEFAULT),
    (1, 1000, 49, 1, None, False, 1, BIG_OFFSET, FINE),
    (3, 300, 49, 3, (2, 5), True, 0, BIG_OFFSET, DEFAULT),
    (1, 131, 8, 4, None, True, 1, 0, FINE),
])
def test_fused_rollout_equals_sample_then_rollout(P, N, n, K, window, with_ref, rnd, offset, integration):
    """acmpc_rollout_sampled_device and the re-drawing finalize against their matrix forms: the sampled kernels keep the
    previous step's blended control in registers, the matrix kernels load it again."""
    rig = _rig(P, N, n, K, window, 800 + n, integration, with_ref=with_ref, kinds=[(1, 0, 3)[p % 3] for p in range(P)])
    try:
        sigma, seed = (0.04, 0.35), 0xC0FFEE1234
        U, costs, keys = tsm._compare_rollouts(rig, N, offset, sigma, seed, rnd)
        tsm._compare_records(rig, U, keys, N, offset, sigma, seed, rnd)
    finally:
        rig.close()


@pytest.mark.parametrize("K", [1, 3])
def test_fused_rollout_and_optimize_equal_the_specification(K):
    """96 x 12 against the restatements alone: the fused rollout's costs, key and count, the re-drawn record, and
    acmpc_optimize's argmin rounds - every round against the same previous control."""
    from acmpc_amd import _capi
    P, N, n, sigma, seed, rnd, window = 2, 96, 12, (0.05, 0.3), 99, 3, (2, 5)
    rig = _rig(P, N, n, K, window, 840, FINE, with_ref=True, kinds=[1, 0])
    try:
        for offset in (0, BIG_OFFSET):
            costs, keys = rig.fused(N, offset, sigma, seed, rnd)
            rec = rig.finalize_sampled(None, N, sigma, seed, rnd)
            for p in range(P):
                want = dss.rollout_sampled(orc, rig.dps[p], rig.eng.coefficients(p), rig.blocks(), rig.centre_h[p], rig.ref_h[p],
                                           N, offset, p, rnd, seed, sigma, reduce=rig.reduce, weights=rig.weights,
                                           nn_window=window, return_states=True, settings=Settings(*FINE, **BOTH),
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
                                       return_states=True, settings=Settings(*FINE, **BOTH), u_prev=rig.u_prev[p])
                centre = U[orc.pick_best(cost)[0]]
            tgd._check_record(_capi.split_record(got[p], n), U, cost, V, X, n)
    finally:
        rig.close()


@pytest.mark.parametrize("update", ["argmin", "softmin"])
@pytest.mark.parametrize("vehicles", [None, (0, 1, 2)], ids=["K1", "K3"])
def test_optimize_with_and_without_the_matrix_and_the_sharded_optimizer(vehicles, update):
    """Rounds 2, both centre updates: the default rounds (no control matrix) against ACMPC_DYNAMIC_MATRIX_ROUNDS=1, bit for
    bit, and ShardedOptimizer at world size 1 against both.  The softmin reads whatever J the rollout wrote."""
    import torch
    from acmpc_amd.sharding import ShardedOptimizer
    P, N, n, rounds, sigma, shrink, seed = 2, 1025, 30, 2, (0.05, 0.3), 0.5, 1234
    eng, dps = tsf._dynamic_engine(P, N, n, seed=860, vehicles=vehicles, window=(2, 5), centre_update=update,
                                   softmin_lambda=0.5)
    try:
        centre, ref = tsf._centres(dps, n, 3)
        x0 = np.stack([d["x0"] for d in dps])
        plain = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        eng.set_dynamics_terms(**BOTH)
        eng.set_previous_control(_previous(P, 5))
        default = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        assert not np.array_equal(plain.view(np.uint32), default.view(np.uint32))   # (the terms reach these rounds)
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", "1")
        matrix = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", None)
        tsm._same_bits(default, matrix, "the rounds without a matrix against the rounds through it")
        assert np.all(default[:, 3] == 1.0) and np.all(np.isfinite(default[:, 0]))
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
    rank's handle carries the same terms and the same previous controls."""
    import torch
    from acmpc_amd import _capi
    from acmpc_amd.sharding import shard_range
    P, N, n, sigma, seed, rnd, base = 3, 1030, 30, (0.05, 0.3), 4242, 1, BIG_OFFSET
    rig = _rig(P, N, n, K, (2, 5), 880, DEFAULT, with_ref=True, kinds=[1, 0, 3])
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
        reduced_h = np.minimum.reduce(shard_keys)                 # the all-reduce(MIN), on the host
        assert np.array_equal(reduced_h, keys.cpu().numpy())
        reduced = torch.tensor(reduced_h, device=rig.dev)
        recs = []
        for off, count in slices:
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
@pytest.mark.parametrize("K,layout,window,integration", [(1, 1, (2, 5), DEFAULT), (2, 0, None, FINE)])
def test_packed_rollout(K, layout, window, integration):
    """The smallest launch with P N K >= 2^20 at n = 4 with an odd N: the f32x2 step loop with the terms.  In full against
    the one-candidate-per-lane kernels - two shards of candidates by index_offset, each below 2^20 - and against the
    specification on each problem's first and last candidates, the workgroup boundaries, the planted non-finite controls
    and a seeded draw (test_gpu_dynamic_packed's subset).  A problem's previous control goes by its kind (p % 4)."""
    import torch
    from acmpc_amd import _capi
    N, n = 4099, 4
    P = tpk._problems_for(N, K)
    half = (N + 1) // 2
    assert P * N * K >= tpk.PACKED and P * half * K < tpk.PACKED
    label = "K %d layout %d window %s P %d" % (K, layout, window, P)
    base, U, x0, tables = tpk._make(P, N, n, seed=900 + K)
    x0[2::4, 3] = 4.0          # (kind 1 is the standstill already; kind 2 inside the blend interval)
    planted = tpk._plant(U, N, n)
    by_kind = _previous(4, 6)
    u_prev = by_kind[np.arange(P) % 4]
    vehicles = [_vehicle()] if K == 1 else [_vehicle(), dataclasses.replace(_vehicle(), lf=1.9, lr=1.1).with_grip(0.6)]
    eng = tge._engine([base[p % 4] for p in range(P)], P, N, n, window)
    try:
        eng.set_dynamics_integration(*integration)
        eng.set_dynamics_terms(**BOTH)
        eng.set_previous_control(u_prev)
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
                                     settings=Settings(*integration, **BOTH), u_prev=by_kind[q])
            return es.spec_ensemble(orc, dp, coefs[q], blocks, reduce="mean", nn_window=window, U=U_sub, return_states=states,
                                    settings=Settings(*integration, **BOTH), u_prev=by_kind[q])

        tpk._check_against_spec(whole, base, coefs, U, N, n, tpk.GROUP_ONE if K == 1 else tpk.GROUP_ENSEMBLE, planted, spec,
                                27 + K, label)
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


# ---- handle hygiene ---------------------------------------------------------------------------------------------------------
def test_terms_off_is_a_handle_that_never_made_the_calls():
    """Set then switched off; an explicit all-off call; set then refused (the refused call keeps the setting it found: off);
    a previous control set with the rate part off, and set then cleared with it on: costs, records and acmpc_optimize's
    records of a handle that never called.  And the setting survives acmpc_set_dynamics, _ensemble and _integration."""
    P, N, n = 2, 700, 30
    dps = tgd._problems(P, N, n, seed=910)
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    centre = np.tile(np.stack([np.zeros(n), np.full(n, 0.2)], axis=1).astype(T), (P, 1, 1))
    u_prev = _previous(P, 7, nan_at=0)
    rate_only = SETTINGS["rate"]

    def run(prepare, finish=lambda eng: None):
        eng = tgd._engine(dps, P, N, n, (2, 5))
        try:
            prepare(eng)
            out = eng.solve(x0, U)
            opt = eng.optimize(x0, centre, None, N, 2, (0.05, 0.3), shrink=0.5, seed=77)
            finish(eng)
            return out["costs"], out["records"], opt["records"]
        finally:
            eng.close()

    def differs(eng, want):
        return not np.array_equal(eng.solve(x0, U)["costs"].view(np.uint32), want.view(np.uint32))

    def there_and_back(eng):
        eng.set_dynamics_terms(**BOTH)
        assert differs(eng, never[0])
        eng.set_dynamics_terms()

    def explicit_off(eng):
        eng.set_dynamics_terms((0.0, 0.0), (INF, INF), 0.0, INF)

    def refused(eng):
        w, m = np.zeros(2), np.ones(2)
        assert eng._lib.acmpc_set_dynamics_terms(eng._ctx, w.ctypes.data, m.ctypes.data, -1.0, 1.0) == -1
        m[1] = 0.0
        assert eng._lib.acmpc_set_dynamics_terms(eng._ctx, w.ctypes.data, m.ctypes.data, 0.0, 1.0) == -1

    def previous_unread(eng):
        eng.set_previous_control(u_prev)          # a NaN in it: not read while the rate part is off
        eng.set_dynamics_terms(slip_weight=0.0)

    never = run(lambda eng: None)
    for prepare in (there_and_back, explicit_off, refused, previous_unread):
        for got, want in zip(run(prepare), never):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), prepare.__name__

    # the rate part on: a previous control set then cleared is a handle that never set one
    def rate_on(eng):
        eng.set_dynamics_terms(**rate_only)

    def set_then_cleared(eng):
        eng.set_dynamics_terms(**rate_only)
        eng.set_previous_control(_previous(P, 8))
        assert differs(eng, rated[0])
        eng.set_previous_control(None)

    rated = run(rate_on)
    assert not np.array_equal(rated[0].view(np.uint32), never[0].view(np.uint32))
    for got, want in zip(run(set_then_cleared), rated):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

    # the setting and the previous control survive a change of vehicle(s) and of the integration setting
    def survives(eng):
        eng.set_dynamics_terms(**BOTH)
        eng.set_previous_control(_previous(P, 8))
        eng.set_dynamics_integration(*FINE)
        eng.set_dynamics_ensemble([_vehicle(), _vehicle().with_grip(0.6)])
        eng.set_dynamics(_vehicle())
        eng.set_dynamics_integration(1, None)

    def direct(eng):
        eng.set_dynamics_terms(**BOTH)
        eng.set_previous_control(_previous(P, 8))

    want = run(direct)
    assert not np.array_equal(want[0].view(np.uint32), never[0].view(np.uint32))
    for got, w in zip(run(survives), want):
        assert np.array_equal(got.view(np.uint32), w.view(np.uint32))
    for p in range(P):   # (and that is the specification's)
        cost = ds.spec_costs(orc, dps[p], orc.coefficients_temporal(dps[p]["table"], dps[p]["kw"]["margin"]).astype(T),
                             _vehicle().coefficients(), nn_window=(2, 5), settings=Settings(*DEFAULT, **BOTH), u_prev=_previous(P,
                             8)[p])[0]
        tgd._same_bits(want[0][p], cost)


# ---- the rate limit -----------------------------------------------------------------------------------------------------------
def test_a_previous_control_out_of_reach_leaves_no_feasible_candidate():
    """u_prev so far from every candidate that step 0 breaks the steering rate limit for all: n_feasible == 0, and the
    winner is the smallest J of the restatement."""
    from acmpc_amd import _capi
    P, N, n = 2, 300, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 930 + p) for p in range(P)]
    terms = dict(rate_weight=(0.0, 0.0), rate_max=(2.0, None), slip_weight=0.0, slip_max=None)
    u_prev = np.array([[2.5, 0.0], [-1.9, 0.2]], dtype=T)     # the box is +-0.3 (+0.2 for one planted candidate): >= 28 rad/s
    eng = tgd._engine(dps, P, N, n, None)
    try:
        U = np.stack([d["U"] for d in dps])
        x0 = np.stack([d["x0"] for d in dps])
        before = eng.solve(x0, U)
        assert np.all(before["n_feasible"] > 0)
        eng.set_dynamics_terms(**terms)
        eng.set_previous_control(u_prev)
        out = eng.solve(x0, U)
        for p in range(P):
            cost, V, X = ds.spec_costs(orc, dps[p], eng.coefficients(p), _vehicle().coefficients(), return_states=True,
                                       settings=Settings(*DEFAULT, **terms), u_prev=u_prev[p])
            assert np.all(V > 0) and out["n_feasible"][p] == 0
            tgd._same_bits(out["costs"][p], cost)
            assert out["best_idx"][p] == orc.pick_best(cost)[0] == int(np.argmin(cost))
            tgd._check_record(_capi.split_record(out["records"][p], n), U[p], cost, V, X, n)
    finally:
        eng.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------------
# The loop of test_gpu_dynamic.test_dynamic_sampling_solver_closed_loop - DynamicSamplingSolver drives the float64 mirror
# round the synthetic Monza circuit from 200 m before its tightest corner - for 200 ticks (340 m: through the corner) with
# 4 096 candidates, once with the terms and once without, the same seeds.
TERMS_TICKS = 200
TERMS_CONFIG = dict(tgd.LOOP_CONFIG, n_candidates=4096)
# steering: 1 rad/s is a hinge (0.05 rad per tick, 2.5 sigma of the sampler's 0.02 rad) and its squared rate costs 0.5 per
# (rad/s)^2 - against r_term's 10 per rad^2 of steering error; the pedal is left alone; rear slip beyond 0.1 (the loop's
# own sideslip bar, a 6 degree slip angle) is a hinge
TERMS_KEYS = dict(rate_cost=(0.5, 0.0), rate_limit=(1.0, None), slip_limit=0.1)


def run_terms_loop(config):
    """Per tick: (e_y, |vy| / vx, vx - v_ref, applied steering, applied pedal, n_feasible, violation)."""
    from acmpc_amd import DynamicSamplingSolver
    plant = _vehicle()
    solver = DynamicSamplingSolver(dict(config), plant)
    centre, v_profile, heading, start = tgd.loop_track()
    state = np.array([centre[start, 0], centre[start, 1], heading[start], v_profile[start] - 4.0, 0.0, 0.0])
    n = tgd.LOOP_H - 1
    log = []
    try:
        for _ in range(TERMS_TICKS):
            table, _ = tgd.loop_path(centre, v_profile, state)
            obj = solver.solve(state, table)
            assert obj.info.status == "solved"
            u = obj.x[3 * (n + 1):].reshape(n, 2)
            state = plant.predict_next_state(state, u[0], tgd.LOOP_DT)[0]
            state[3] = max(state[3], 0.0)
            ey, i = tgd.loop_frenet(centre, heading, state)
            log.append((ey, abs(state[4]) / max(state[3], 1.0), state[3] - v_profile[i], u[0, 0], u[0, 1], obj.n_feasible,
                        obj.violation))
    finally:
        solver.close()
    return np.array(log)


def test_closed_loop_steers_more_smoothly_inside_its_rate_limit():
    with_terms = run_terms_loop(dict(TERMS_CONFIG, **TERMS_KEYS))
    without = run_terms_loop(TERMS_CONFIG)
    rms = [float(np.sqrt(np.mean(np.diff(log[:, 3]) ** 2))) for log in (with_terms, without)]
    print("closed loop, %d ticks: RMS steering increment %.6f rad with %r, %.6f rad without" % (TERMS_TICKS, rms[0], TERMS_KEYS,
                                                                                                rms[1]))
    # (a) the existing loop's bars
    ey, slip, dv = with_terms[:, 0], with_terms[:, 1], with_terms[:, 2]
    print("max |e_y| %.3f m, mean %.3f m, sideslip %.4f, speed error %.3f m/s" % (
        np.abs(ey).max(), np.abs(ey).mean(), slip.max(), np.abs(dv[int(2.0 / tgd.LOOP_DT):]).max()))
    assert np.abs(ey).max() < tgd.LOOP_CORRIDOR, "left the corridor: |e_y| %.2f m" % np.abs(ey).max()
    assert np.abs(ey).mean() < tgd.LOOP_MEAN_EY, "does not hold the centre line: mean |e_y| %.2f m" % np.abs(ey).mean()
    assert slip.max() < tgd.LOOP_SLIP, "sideslip |vy| / vx %.4f" % slip.max()
    assert np.abs(dv[int(2.0 / tgd.LOOP_DT):]).max() < tgd.LOOP_SPEED_BAND
    # (b) where a tick had a feasible candidate, the steering applied moved from the one before by at most the limit - in
    # the kernel's own arithmetic: h = max(|(delta_0 - delta_applied) * inv_dt| - rate_limit, 0) == 0 - and a feasible winner
    # has V == 0
    inv_dt, limit = T(1.0 / tgd.LOOP_DT), T(TERMS_KEYS["rate_limit"][0])
    checked = 0
    for tick in range(1, TERMS_TICKS):
        if with_terms[tick, 5] > 0:
            rd = T(T(T(with_terms[tick, 3]) - T(with_terms[tick - 1, 3])) * inv_dt)
            assert T(abs(rd)) - limit <= 0, "tick %d: steering rate %.4f rad/s" % (tick, rd)
            assert with_terms[tick, 6] == 0.0, "tick %d: a winner with V %.3g among %d feasible candidates" % (
                tick, with_terms[tick, 6], with_terms[tick, 5])
            checked += 1
    assert checked > TERMS_TICKS // 2
    # (c) and it steers more smoothly than the same loop without the terms
    assert rms[0] < rms[1]
