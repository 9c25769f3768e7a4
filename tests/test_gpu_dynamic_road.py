"""Mode D's road table (acmpc_set_road) on the MI355X, from every call form.  Costs, keys, feasible counts, records and traces
must be bit-identical to tests/dynamic_road_spec.py (NaN equal to NaN by bits, no candidate left out); the neutral table and a
uniform power-of-two n_z are held to the kernels that were there before; a table for another shape is refused and clearing gives
the bits of a handle that never had one; DynamicSamplingSolver takes `road=`.

Every case unless it says otherwise: P = 2 on the dense problems of tests/test_gpu_dynamic_surface.py (waypoints 1.5 m apart,
problem 0 from a standstill, problem 1 at the path's speed), N = 300 (one full 256-lane workgroup and a tail), n = 12, seeded
tables that differ per problem with the grade within +-0.10 rad and the bank within +-0.12 rad.  Each test asserts what it relies
on: the nearest index reaches 3, some step has lanes on different waypoints, and the road rows used are not all equal."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_road_spec as drs
import dynamic_sampled_spec as dsamp
import dynamic_softmin_spec as sms
import dynamic_spec as ds
import dynamic_surface_spec as dss
from dynamic_spec import Settings
import test_dynamic_actuator as tda
import test_dynamic_road as tdr
import test_gpu_dynamic as tgd
import test_gpu_dynamic_coupling as tgc
import test_gpu_dynamic_ensemble as tge
import test_gpu_dynamic_load_transfer as tgl
import test_gpu_dynamic_packed as tpk
import test_gpu_dynamic_softmin as tsf
import test_gpu_dynamic_surface as tgs
import test_gpu_dynamic_terms as tgt

pytestmark = pytest.mark.gpu

T = np.float32
EINVAL, ESTATE = -1, -5
P, N, n = tgs.P, tgs.N, tgs.n
assert (P, N, n) == (2, 300, 12)
LOAD, AERO = tgs.LOAD, tgs.AERO
DEFAULT, FINE = tgc.DEFAULT, tgc.FINE
OFF, ALL_FOUR = tgc.OFF, tgc.ALL_FOUR
BIG_OFFSET = tgc.BIG_OFFSET
TIERS = tgs.TIERS
GRIPS = tgs.GRIPS
WEIGHTS = (1.0, 2.0, 0.5)
SIGMA = (0.05, 0.3)
TAU = tda.TAU
_vehicle, _u32 = tgc._vehicle, tgc._u32
_same_where_finite = tgl._same_where_finite
_problems, _tables, _crosses_waypoints = tgs._problems, tgs._tables, tgs._crosses_waypoints


def _roads(seed, count=P, steps=n):
    return np.stack([drs.random_road(steps, seed + p) for p in range(count)])


def _vehicles(K):
    return [_vehicle()] if K == 1 else [_vehicle().with_grip(g) for g in GRIPS[:K]]


def _handle(dps, steps, window, K, reduce="mean", count=P, candidates=N, **extra):
    eng = tge._engine(dps, count, candidates, steps, window, **extra)
    if K == 1:
        eng.set_dynamics(_vehicle())
    else:
        eng.set_dynamics_ensemble(_vehicles(K), weights=WEIGHTS[:K], reduce=reduce)
    return eng


def _set(eng, tier, setting=OFF, u_prev=None, integration=DEFAULT):
    eng.set_dynamics_integration(*integration)
    tgs._set(eng, *TIERS[tier], setting, u_prev)


def _settings(tier, setting, integration, clearance=False):
    ratio, load, aero = TIERS[tier]
    extra = dict(clearance_weight=40.0, clearance_margin=1.0) if clearance else {}
    return Settings(*integration, **setting[0], **setting[1], coupling=ratio, load_transfer=load, downforce=aero, **extra)


def _discs(eng, dps, steps, K_obs, seed):
    if not K_obs:
        return None
    discs = [ds.make_obstacles(d, steps, K_obs, seed + p) for p, d in enumerate(dps)]
    eng.set_dynamics_clearance(40.0, 1.0)
    eng.set_obstacles(np.stack([d[0] for d in discs]), np.stack([d[1] for d in discs]))
    return discs


def _kw(p, window, s, prev, road, mu=None, discs=None, tau=None, a0=None):
    return dict(nn_window=window, settings=s, u_prev=None if prev is None else prev[p], road=road[p],
                surface=None if mu is None else mu[p], obstacles=None if discs is None else discs[p], actuator=tau,
                a0=None if a0 is None else a0[p])


def _spec(dp, coef, K, reduce, **kw):
    blocks = [v.coefficients() for v in _vehicles(K)]
    if K == 1:
        return drs.spec_costs(orc, dp, coef, blocks[0], **kw)
    return drs.spec_ensemble(orc, dp, coef, blocks, reduce=reduce, weights=WEIGHTS[:K], **kw)


def _relies_on(dp, coef, road, label="", block=None, **kw):
    """What a test of the table relies on, from the restatement: the nearest index reaches 3, some step has lanes on different
    waypoints, and the road rows the steps used are not all equal.  Returns the trace."""
    trace = {}
    kw.pop("road", None)
    drs.spec_costs(orc, dp, coef, _vehicle().coefficients() if block is None else block, road=road, trace=trace, **kw)
    _crosses_waypoints(trace["j"], label)
    used = np.asarray(road, dtype=T)[np.unique(trace["road_j"])]
    assert len(np.unique(used, axis=0)) > 1, label
    return trace


def _check_solve(eng, out, dps, U_h, steps, K, reduce, kws, label=""):
    from acmpc_amd import _capi
    for p in range(len(dps)):
        cost, V, X = _spec(dps[p], eng.coefficients(p), K, reduce, return_states=True, **kws[p])
        tgd._same_bits(out["costs"][p], cost)
        rec = _capi.split_record(out["records"][p], steps)
        best = tgd._check_record(rec, U_h[p], cost, V, X, steps)
        assert out["best_idx"][p] == best and out["n_feasible"][p] == np.count_nonzero(V == 0), (label, p)
        tgd._same_bits(rec["cost"], out["costs"][p][best])      # the finalize's re-roll gives the rollout's own cost


# ---- the control-matrix solve ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("integration", [DEFAULT, FINE], ids=["euler", "M3-blend"])
@pytest.mark.parametrize("layout,window", [(0, None), (1, (2, 5)), (1, None), (0, (2, 5))])
def test_costs_argmin_and_record_are_the_specification(layout, window, integration, tier):
    dps = _problems()
    u_prev = tgt._previous(P, 71)
    road, mu = _roads(111), _tables(112)
    eng = tgd._engine(dps, P, N, n, window)
    try:
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        x0 = np.stack([d["x0"] for d in dps])
        _set(eng, tier, integration=integration)
        parent = eng.solve(x0, U_in, layout=layout)["costs"]         # the same handle without the table
        eng.set_road(road)
        for name, setting, prev, surface in (("off, no surface", OFF, None, None), ("all four, surface", ALL_FOUR, u_prev, mu)):
            _set(eng, tier, setting, prev, integration)
            eng.set_surface(surface)
            out = eng.solve(x0, U_in, layout=layout)
            s = _settings(tier, setting, integration)
            kws = [_kw(p, window, s, prev, road, surface) for p in range(P)]
            _relies_on(dps[1], eng.coefficients(1), label=name, **kws[1])
            _check_solve(eng, out, dps, U_h, n, 1, "mean", kws, name)
            if surface is None:
                assert not np.array_equal(_u32(out["costs"][1]), _u32(parent[1])), name
        assert np.isnan(out["costs"][0][5]) and not np.isfinite(out["costs"][1][7])
    finally:
        eng.close()


# ---- the sampled forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,integration,tier,terms,surface,K,reduce,offset", [
    ((2, 5), DEFAULT, "none", False, False, 1, "mean", 0),
    (None, FINE, "loaded-coupled-downforce", True, True, 1, "mean", BIG_OFFSET),
    (None, DEFAULT, "coupled", True, True, 3, "max", 0)])
def test_fused_sampled_rollout_and_the_record_redrawn_from_its_index(window, integration, tier, terms, surface, K, reduce, offset):
    import torch
    from acmpc_amd import _capi
    dps = _problems()
    setting, prev = (ALL_FOUR, tgt._previous(P, 72)) if terms else (OFF, None)
    seed, rnd = 77, 1
    road, mu = _roads(121), (_tables(122) if surface else None)
    eng = _handle(dps, n, window, K, reduce)
    try:
        _set(eng, tier, setting, prev, integration)
        eng.set_surface(mu)
        eng.set_road(road)
        centre, ref = tsf._centres(dps, n, 6)
        x0 = np.stack([d["x0"] for d in dps])
        dev, s = torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
        d_x0, d_c, d_r = (torch.tensor(a, device=dev) for a in (x0, centre, ref))
        costs, keys = torch.empty(P, N, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
        rec = torch.empty(P, _capi.record_floats(n), device=dev)
        eng.rollout_sampled_device(d_x0.data_ptr(), d_c.data_ptr(), 2 * n, d_r.data_ptr(), P, N, n, offset, SIGMA, seed, rnd,
                                   costs.data_ptr(), keys.data_ptr(), s)
        eng.finalize_sampled_device(0, d_x0.data_ptr(), d_c.data_ptr(), 2 * n, d_r.data_ptr(), P, N, n, SIGMA, seed, rnd,
                                    rec.data_ptr(), s)
        torch.cuda.synchronize()
        st = _settings(tier, setting, integration)
        for p in range(P):
            U = dsamp.candidates(orc, dps[p], centre[p], ref[p], N, offset, p, rnd, seed, SIGMA)
            kw = _kw(p, window, st, prev, road, mu)
            if p == 1:
                _relies_on(dps[p], eng.coefficients(p), U=U, **kw)
            cost, V, X = _spec(dps[p], eng.coefficients(p), K, reduce, U=U, return_states=True, **kw)
            tgd._same_bits(costs[p].cpu().numpy(), cost)
            best = orc.pick_best(cost)[0]
            assert int(keys[p].item()) == dsamp.pack_key(cost[best], offset + best)
            r = _capi.split_record(rec[p].cpu().numpy(), n)
            assert r["owner"] == 1.0 and r["n_feasible"] == np.count_nonzero(V == 0)
            tgd._same_bits(r["cost"], cost[best])
            tgd._same_bits(r["violation"], V[best])
            tgd._same_bits(r["u"], U[best])
            tgd._same_bits(r["x"], X[best])
    finally:
        eng.close()


@pytest.mark.parametrize("window,integration,tier,terms,surface,K,reduce", [
    ((2, 5), FINE, "loaded-coupled-downforce", True, True, 1, "mean"), (None, DEFAULT, "none", False, False, 3, "mean")])
def test_optimize_of_two_rounds_with_argmin_is_its_restatement(window, integration, tier, terms, surface, K, reduce):
    from acmpc_amd import _capi
    dps = _problems()
    setting, prev = (ALL_FOUR, tgt._previous(P, 73)) if terms else (OFF, None)
    rounds, shrink, seed = 2, 0.5, 1234
    road, mu = _roads(131), (_tables(132) if surface else None)
    eng = _handle(dps, n, window, K, reduce)
    try:
        _set(eng, tier, setting, prev, integration)
        eng.set_surface(mu)
        eng.set_road(road)
        centre, _ = tsf._centres(dps, n, 7)
        x0 = np.stack([d["x0"] for d in dps])
        out = eng.optimize(x0, centre, None, N, rounds, SIGMA, shrink=shrink, seed=seed)
        st = _settings(tier, setting, integration)
        for p in range(P):
            c = centre[p]
            kw = _kw(p, window, st, prev, road, mu)
            for r, sig in enumerate(sms.round_sigmas(SIGMA, shrink, rounds)):
                U = dsamp.candidates(orc, dps[p], c, None, N, 0, p, r, seed, sig)
                cost, V, X = _spec(dps[p], eng.coefficients(p), K, reduce, U=U, return_states=True, **kw)
                c = U[orc.pick_best(cost)[0]]
            if p == 1:
                _relies_on(dps[p], eng.coefficients(p), U=U, **kw)
            tgd._check_record(_capi.split_record(out["records"][p], n), U, cost, V, X, n)
    finally:
        eng.close()


@pytest.mark.parametrize("window,integration,tier,terms,surface,K,reduce", [
    ((2, 5), DEFAULT, "loaded-coupled-downforce", True, True, 1, "mean"), (None, FINE, "coupled", False, False, 3, "max")])
def test_optimize_of_two_rounds_with_softmin_recentring(window, integration, tier, terms, surface, K, reduce):
    """acmpc_optimize under `centre_update="softmin"` against the loop of device calls it stands for - round r samples round the
    softmin mean of round r - 1 with the previous winner as candidate 1 - and every round of that loop against the restatement:
    the costs and the key of the candidates drawn round the mean the device computed, bit for bit."""
    import torch
    from acmpc_amd import _capi
    dps = _problems()
    setting, prev = (ALL_FOUR, tgt._previous(P, 74)) if terms else (OFF, None)
    rounds, shrink, seed, lam = 2, 0.5, 4321, 0.5
    road, mu = _roads(141), (_tables(142) if surface else None)
    eng = _handle(dps, n, window, K, reduce, centre_update="softmin", softmin_lambda=lam)
    try:
        _set(eng, tier, setting, prev, integration)
        eng.set_surface(mu)
        eng.set_road(road)
        centre, ref_h = tsf._centres(dps, n, 8)
        x0 = np.stack([d["x0"] for d in dps])
        got = eng.optimize(x0, centre, ref_h, N, rounds, SIGMA, shrink=shrink, seed=seed)["records"]
        dev, s = torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
        d_x0, d_ref = torch.tensor(x0, device=dev), torch.tensor(ref_h, device=dev)
        mean = torch.tensor(centre, device=dev)
        costs, keys = torch.empty(P, N, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
        rec = torch.empty(P, _capi.record_floats(n), device=dev)
        wsum = torch.empty(P, dtype=torch.float64, device=dev)
        st = _settings(tier, setting, integration)
        for r, sig in enumerate(sms.round_sigmas(SIGMA, shrink, rounds)):
            ref = d_ref if r == 0 else rec[:, _capi.REC_HEADER:_capi.REC_HEADER + 2 * n].contiguous()
            sig = (float(sig[0]), float(sig[1]))
            c_h, r_h = mean.cpu().numpy().copy(), ref.cpu().numpy().reshape(P, n, 2).copy()
            eng.rollout_sampled_device(d_x0.data_ptr(), mean.data_ptr(), 2 * n, ref.data_ptr(), P, N, n, 0, sig, seed, r,
                                       costs.data_ptr(), keys.data_ptr(), s)
            eng.finalize_sampled_device(0, d_x0.data_ptr(), mean.data_ptr(), 2 * n, ref.data_ptr(), P, N, n, sig, seed, r,
                                        rec.data_ptr(), s)
            torch.cuda.synchronize()
            new_mean = torch.empty_like(mean)
            eng.softmin_sampled_device(costs.data_ptr(), keys.data_ptr(), mean.data_ptr(), 2 * n, ref.data_ptr(), P, N, n, 0, sig,
                                       seed, r, new_mean.data_ptr(), wsum.data_ptr(), s)
            torch.cuda.synchronize()
            for p in range(P):
                U = dsamp.candidates(orc, dps[p], c_h[p], r_h[p], N, 0, p, r, seed, sig)
                kw = _kw(p, window, st, prev, road, mu)
                cost, V, X = _spec(dps[p], eng.coefficients(p), K, reduce, U=U, return_states=True, **kw)
                tgd._same_bits(costs[p].cpu().numpy(), cost)
                best = orc.pick_best(cost)[0]
                assert int(keys[p].item()) == dsamp.pack_key(cost[best], best)
                one = _capi.split_record(rec[p].cpu().numpy(), n)
                tgd._same_bits(one["u"], U[best])
                tgd._same_bits(one["x"], X[best])
                np.testing.assert_allclose(new_mean[p].cpu().numpy(), sms.softmin_mean(orc, cost, U, lam), rtol=2e-5, atol=1e-6)
                if p == 1 and r == 0:
                    _relies_on(dps[p], eng.coefficients(p), U=U, **kw)
            mean = new_mean
        assert np.array_equal(got.view(np.uint32), rec.cpu().numpy().view(np.uint32)), "acmpc_optimize against the loop of device calls"
    finally:
        eng.close()


# ---- an ensemble: every vehicle on its own trajectory's j, the table shared ------------------------------------------------------
@pytest.mark.parametrize("reduce,layout,window,integration,setting,tier,surface", [
    ("mean", 0, None, DEFAULT, OFF, "coupled", False), ("max", 1, (2, 5), FINE, ALL_FOUR, "loaded-coupled-downforce", True)])
def test_ensemble_of_three_is_the_specification(reduce, layout, window, integration, setting, tier, surface):
    dps = _problems()
    prev = tgt._previous(P, 75) if setting is ALL_FOUR else None
    road, mu = _roads(151), (_tables(152) if surface else None)
    eng = _handle(dps, n, window, 3, reduce)
    try:
        _set(eng, tier, setting, prev, integration)
        eng.set_surface(mu)
        eng.set_road(road)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        out = eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)
        s = _settings(tier, setting, integration)
        kws = [_kw(p, window, s, prev, road, mu) for p in range(P)]
        js = [_relies_on(dps[1], eng.coefficients(1), block=v.coefficients(), **kws[1])["road_j"] for v in _vehicles(3)]
        assert np.any(js[0] != js[2])          # the vehicles are on different waypoints at some step: each gathers by its own
        _check_solve(eng, out, dps, U_h, n, 3, reduce, kws)
    finally:
        eng.close()


# ---- obstacles and the actuator lag ride on the road pack -----------------------------------------------------------------------
@pytest.mark.parametrize("K,K_obs,layout,integration,tier,surface", [(1, 1, 0, DEFAULT, "none", False),
                                                                     (3, 8, 1, FINE, "loaded-coupled-downforce", True)])
def test_obstacles_ride_on_the_road_pack(K, K_obs, layout, integration, tier, surface):
    dps = _problems()
    prev = tgt._previous(P, 76)
    road, mu = _roads(161), (_tables(162) if surface else None)
    eng = _handle(dps, n, (2, 5), K)
    try:
        _set(eng, tier, ALL_FOUR, prev, integration)
        discs = _discs(eng, dps, n, K_obs, 2470)
        eng.set_surface(mu)
        eng.set_road(road)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        x0 = np.stack([d["x0"] for d in dps])
        out = eng.solve(x0, U_in, layout=layout)
        s = _settings(tier, ALL_FOUR, integration, clearance=True)
        kws = [_kw(p, (2, 5), s, prev, road, mu, discs) for p in range(P)]
        _relies_on(dps[1], eng.coefficients(1), **kws[1])
        _check_solve(eng, out, dps, U_h, n, K, "mean", kws)
        # the discs do something, and so does the road under them
        eng.set_obstacles(None)
        assert not np.array_equal(_u32(eng.solve(x0, U_in, layout=layout)["costs"]), _u32(out["costs"]))
    finally:
        eng.close()


@pytest.mark.parametrize("K,K_obs,layout,window,integration,tier,surface,given", [
    (1, 0, 0, None, DEFAULT, "none", False, True), (3, 0, 1, (2, 5), FINE, "loaded-coupled-downforce", True, False),
    (1, 1, 1, (2, 5), FINE, "coupled", True, True), (3, 8, 0, None, DEFAULT, "loaded-coupled-downforce", False, False)])
def test_the_actuator_lag_rides_on_the_road_pack(K, K_obs, layout, window, integration, tier, surface, given):
    dps = _problems()
    prev = tgt._previous(P, 77)
    road, mu = _roads(171), (_tables(172) if surface else None)
    a0 = tda.positions(P, 78) if given else None
    eng = _handle(dps, n, window, K)
    try:
        _set(eng, tier, ALL_FOUR, prev, integration)
        discs = _discs(eng, dps, n, K_obs, 2480)
        eng.set_surface(mu)
        eng.set_road(road)
        eng.set_dynamics_actuator(TAU)
        eng.set_actuator_state(a0)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        x0 = np.stack([d["x0"] for d in dps])
        out = eng.solve(x0, U_in, layout=layout)
        s = _settings(tier, ALL_FOUR, integration, clearance=K_obs > 0)
        kws = [_kw(p, window, s, prev, road, mu, discs, TAU, a0) for p in range(P)]
        _relies_on(dps[1], eng.coefficients(1), **kws[1])
        _check_solve(eng, out, dps, U_h, n, K, "mean", kws)
        # the sampled form of the same handle, and the lag does something
        if K_obs == 0:
            import torch
            centre, ref = tsf._centres(dps, n, 9)
            dev, st = torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
            d_x0, d_c, d_r = (torch.tensor(a, device=dev) for a in (x0, centre, ref))
            costs, keys = torch.empty(P, N, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
            eng.rollout_sampled_device(d_x0.data_ptr(), d_c.data_ptr(), 2 * n, d_r.data_ptr(), P, N, n, 0, SIGMA, 79, 0,
                                       costs.data_ptr(), keys.data_ptr(), st)
            torch.cuda.synchronize()
            for p in range(P):
                U = dsamp.candidates(orc, dps[p], centre[p], ref[p], N, 0, p, 0, 79, SIGMA)
                tgd._same_bits(costs[p].cpu().numpy(), _spec(dps[p], eng.coefficients(p), K, "mean", U=U, **kws[p])[0])
        eng.set_dynamics_actuator(None)
        assert not np.array_equal(_u32(eng.solve(x0, U_in, layout=layout)["costs"]), _u32(out["costs"]))
    finally:
        eng.close()


# ---- the plan trace -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps,K,window,integration,tier,K_obs,surface,lag", [
    (2, 1, None, DEFAULT, "none", 0, False, False), (2, 3, (2, 5), FINE, "loaded-coupled-downforce", 2, True, True),
    (65, 1, (2, 5), FINE, "coupled", 2, True, False), (65, 3, None, DEFAULT, "loaded-coupled-downforce", 0, False, True)])
def test_trace_plans_is_the_specification(steps, K, window, integration, tier, K_obs, surface, lag):
    from acmpc_amd import _capi
    count = 70
    dps = tda.problems(steps, count, seed=2901)
    prev = tgt._previous(P, 81)
    road = _roads(181, steps=steps)
    mu = np.stack([dss.random_table(steps, 182 + p) for p in range(P)]) if surface else None
    tau = TAU if lag else None
    a0 = tda.positions(P, 83) if lag else None
    eng = _handle(dps, steps, window, K, candidates=count)
    try:
        _set(eng, tier, ALL_FOUR, prev, integration)
        discs = _discs(eng, dps, steps, K_obs, 2490)
        eng.set_surface(mu)
        eng.set_road(road)
        eng.set_dynamics_actuator(tau)
        eng.set_actuator_state(a0)
        U_all = np.stack([d["U"] for d in dps])
        U = np.ascontiguousarray(U_all[:, 20:23])                        # three plans per problem
        x0 = np.stack([d["x0"] for d in dps])
        got = eng.trace_plans(x0, U)
        assert _capi.TRACE_TERM_FLOATS == 22 and got["terms"].shape == (P, 3, K, steps, 22)
        s = _settings(tier, ALL_FOUR, integration, clearance=K_obs > 0)
        per = [drs.trace_plans(dp, eng.coefficients(p), U[p], [v.coefficients() for v in _vehicles(K)], s, window, prev[p],
                               None if discs is None else discs[p], surface=None if mu is None else mu[p], actuator=tau,
                               a0=None if a0 is None else a0[p], road=road[p]) for p, dp in enumerate(dps)]
        want = {name: np.stack([t[name] for t in per]) for name in ("states", "totals", "terms")}
        for name in ("states", "terms"):
            assert np.array_equal(ds.bits(got[name]), ds.bits(want[name])), name
        assert np.array_equal(ds.bits(np.stack([got["cost"], got["violation"]], axis=-1)), ds.bits(want["totals"]))
        # the replay reproduces V
        assert np.array_equal(ds.bits(ds.replay(got["terms"])), ds.bits(got["terms"][..., ds.V_SLOT]))
        if steps == 65:   # slot 0 of row i - 1 names the waypoint whose road row step i used: several of them, rows that differ
            j = got["terms"][1, ..., ds.J].astype(np.int64)
            assert j.max() >= 3 and len(np.unique(road[1][np.unique(j[..., :-1])], axis=0)) > 1
        # vehicle 0's poses are the winner's record: the solve of the same candidates picks one per problem, and the record's x
        # is that plan's trace under vehicle 0
        out = eng.solve(x0, U_all)
        winners = np.ascontiguousarray(np.stack([U_all[p, int(out["best_idx"][p])][None] for p in range(P)]))
        one = eng.trace_plans(x0, winners, want=("states",))
        for p in range(P):
            rec = _capi.split_record(out["records"][p], steps)
            assert np.array_equal(ds.bits(one["states"][p, 0, 0, :, :3]), ds.bits(np.asarray(rec["x"]).reshape(steps + 1, 3))), p
    finally:
        eng.close()


# ---- two candidates per lane ----------------------------------------------------------------------------------------------------
PACKED_N = tgs.PACKED_N


@pytest.mark.parametrize("K,layout,window,surface", [(1, 1, None, True), (2, 0, (2, 5), False)])
def test_packed_rollout_gathers_two_road_rows_per_lane(K, layout, window, surface):
    count, base, U, x0, tables, kinds_mu, mu_all = tgs._packed(K)
    kinds = _roads(191, 4)
    road = np.stack([kinds[p % 4] for p in range(count)])
    mu = mu_all if surface else None
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
        eng.set_road(road)
        U_in = tpk._as_layout(U, layout)
        out = eng.solve(x0, U_in, layout=layout)
        coefs = [eng.coefficients(q) for q in range(4)]
        s = _settings("loaded-coupled-downforce", ALL_FOUR, DEFAULT)

        def spec(q, U_sub, states):
            return drs.spec_ensemble(orc, base[q], coefs[q], [v.coefficients() for v in vehicles], reduce="mean",
                                     weights=(1.0, 2.0)[:K], nn_window=window, U=U_sub, return_states=states, settings=s,
                                     surface=kinds_mu[q] if surface else None, road=kinds[q])

        trace = _relies_on(base[0], coefs[0], kinds[0], label, nn_window=window, U=U[0][:64], settings=s,
                           surface=kinds_mu[0] if surface else None)
        assert np.any(trace["road_j"][0::2] != trace["road_j"][1::2])     # the two candidates of a lane on different waypoints
        group = tpk.GROUP_ONE if K == 1 else tpk.GROUP_ENSEMBLE
        tpk._check_against_spec(out, base, coefs, U, PACKED_N, n, group, planted, spec, 27 + K, label)
        # packed against unpacked slices of the same handle, each slice with its own rows of the tables
        chunk = (tpk.PACKED - 1) // (PACKED_N * K)
        assert 1 <= chunk < count
        for lo in range(0, count, chunk):
            hi = min(lo + chunk, count)
            eng.set_paths(tables[lo:hi])
            eng.set_surface(None if mu is None else mu[lo:hi])
            eng.set_road(road[lo:hi])
            part = eng.solve(x0[lo:hi], U_in[lo:hi], layout=layout)
            tgd._same_bits(part["costs"], out["costs"][lo:hi])
            assert np.array_equal(part["best_idx"], out["best_idx"][lo:hi]), label
            assert np.array_equal(part["records"].view(np.uint32), out["records"][lo:hi].view(np.uint32)), label
    finally:
        eng.close()


# ---- identities against the kernels that were there before ----------------------------------------------------------------------
def _all_forms(dps, K, reduce, update, integration, setting, prev, tier, surface, road):
    """solve in both layouts, the sampled rollout (costs and keys), acmpc_optimize (its re-drawn records) of one handle."""
    import torch
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    U1 = np.ascontiguousarray(U.transpose(0, 2, 3, 1))
    centre, ref = tsf._centres(dps, n, 5)
    eng = _handle(dps, n, (2, 5), K, reduce, centre_update=update, softmin_lambda=0.5)
    try:
        _set(eng, tier, setting, prev, integration)
        eng.set_surface(surface)
        eng.set_road(road)
        a, b = eng.solve(x0, U), eng.solve(x0, U1, layout=1)
        opt = eng.optimize(x0, centre, ref, N, 2, SIGMA, shrink=0.5, seed=31)["records"]
        dev, s = torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
        d_x0, d_c = torch.tensor(x0, device=dev), torch.tensor(centre, device=dev)
        costs, keys = torch.empty(P, N, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
        eng.rollout_sampled_device(d_x0.data_ptr(), d_c.data_ptr(), 2 * n, 0, P, N, n, BIG_OFFSET, SIGMA, 77, 1,
                                   costs.data_ptr(), keys.data_ptr(), s)
        torch.cuda.synchronize()
        trace = eng.trace_plans(x0, U[:, 20:22])
        return [a["costs"], a["records"], b["costs"], b["records"], opt, costs.cpu().numpy(), keys.cpu().numpy(), trace["states"],
                trace["terms"]]
    finally:
        eng.close()


def _same_bits_all(got, want, label):
    for q, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert np.array_equal(g.view(np.uint32 if g.dtype == T else g.dtype), w.view(np.uint32 if w.dtype == T else w.dtype)), (label, q)


@pytest.mark.parametrize("K,reduce,update,integration,setting,tier", [
    (1, "mean", "argmin", DEFAULT, OFF, "loaded-coupled-downforce"), (1, "mean", "softmin", FINE, ALL_FOUR, "none"),
    (3, "max", "argmin", FINE, ALL_FOUR, "coupled")], ids=["K1-aero", "K1-plain-softmin", "K3-max-coupled"])
def test_the_neutral_table_and_a_uniform_half_against_the_kernels_that_were_there_before(K, reduce, update, integration, setting, tier):
    dps = _problems()
    prev = tgt._previous(P, 84) if setting is ALL_FOUR else None
    args = (dps, K, reduce, update, integration, setting, prev, tier)
    neutral = np.tile(np.array([0.0, 0.0, 1.0], dtype=T), (P, n, 1))
    half = np.tile(np.array([0.0, 0.0, 0.5], dtype=T), (P, n, 1))
    ones = np.ones((P, n, 2), dtype=T)
    got = _all_forms(*args, None, neutral)
    # x + (+0) turns a -0 into +0 and leaves every other value: where the surface kernels give a zero the sign may differ, nothing
    # else may (tests/test_dynamic_road.py counts the cases on the restatement)
    want = _all_forms(*args, ones, None)
    for q, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype != T:
            assert np.array_equal(g, w), q
            continue
        differ = _u32(g) != _u32(w)
        assert np.all((g[differ] == 0) & (w[differ] == 0)), ("neutral against a surface table of ones", q)
    # with no table at all, wherever that handle's values are finite (again up to the sign of a zero)
    plain = _all_forms(*args, None, None)
    for q, (g, w) in enumerate(zip(got[:7], plain[:7])):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype != T:
            assert np.array_equal(g, w), q
            continue
        finite = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), finite), ("neutral against no table", q)
        differ = finite & (_u32(g) != _u32(w))
        assert np.all((g[differ] == 0) & (w[differ] == 0)), ("neutral against no table", q)
    # n_z = 0.5 everywhere is the surface (0.5, 0.5) everywhere; over a surface table, the product of the two powers of two
    want = _all_forms(*args, 0.5 * ones, neutral)
    _same_bits_all(_all_forms(*args, None, half), want, "uniform 0.5")
    quarter = np.tile(np.array([0.0, 0.0, 0.25], dtype=T), (P, n, 1))
    _same_bits_all(_all_forms(*args, 0.5 * ones, quarter), _all_forms(*args, 0.125 * ones, neutral), "0.25 over 0.5")
    assert not np.array_equal(_u32(want[0]), _u32(got[0])) and not np.array_equal(_u32(want[5]), _u32(got[5]))


# ---- a table for another shape, and clearing ------------------------------------------------------------------------------------
def test_a_table_for_another_shape_is_refused_and_clearing_gives_the_handle_that_never_had_one():
    from acmpc_amd import EngineError
    dps = _problems()
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    centre, ref = tsf._centres(dps, n, 5)
    road = _roads(201)
    eng = tgd._engine(dps, P, N, n, (2, 5))
    never = tgd._engine(dps, P, N, n, (2, 5))
    try:
        eng.set_road(road)
        want = eng.solve(x0, U)
        for wrong in (road[:1], road[:, : n - 1]):
            eng.set_road(wrong)
            for call in (lambda: eng.solve(x0, U), lambda: eng.optimize(x0, centre, ref, N, 2, SIGMA, shrink=0.5, seed=31),
                         lambda: eng.trace_plans(x0, U[:, :2])):
                with pytest.raises(EngineError) as e:
                    call()
                assert e.value.code == ESTATE and "acmpc_set_road" in str(e.value)
        with pytest.raises(EngineError) as e:
            eng.set_road(np.zeros((P, n, 3), dtype=T))                   # n_z = 0: refused, the wrong table stays
        assert e.value.code == EINVAL
        eng.set_road(road)
        again = eng.solve(x0, U)
        assert np.array_equal(_u32(again["costs"]), _u32(want["costs"])) and np.array_equal(_u32(again["records"]), _u32(want["records"]))
        eng.set_road(None)
        a, b = eng.solve(x0, U), never.solve(x0, U)
        assert np.array_equal(_u32(a["costs"]), _u32(b["costs"])) and np.array_equal(_u32(a["records"]), _u32(b["records"]))
        assert not np.array_equal(_u32(a["costs"]), _u32(want["costs"]))
        ta, tb = eng.trace_plans(x0, U[:, :2]), never.trace_plans(x0, U[:, :2])
        assert np.array_equal(ds.bits(ta["states"]), ds.bits(tb["states"])) and np.array_equal(ds.bits(ta["terms"]), ds.bits(tb["terms"]))
    finally:
        eng.close()
        never.close()


# ---- the solver -----------------------------------------------------------------------------------------------------------------
SOLVER = dict(horizon=n + 1, n_candidates=2048, sampling_rounds=2, sampling_sigma=(0.02, 0.3), sampling_seed=11, progress_cost=3.0,
              speed_ceiling=(1.05, 0.0), r_term=(0.0, 10.0), tyre_coupling=(1.0, 1.0), plan_states=True)


def test_dynamic_sampling_solver_takes_a_road():
    from acmpc_amd import dynamic_model as dm
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    dp = _problems()[1]
    table = dp["table"]
    arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(table[0]), np.diff(table[1])))])[:n]
    road = dm.road_table([(3.0, 100.0, -np.arctan(0.06))], arc_length=arc)                 # 6 % downhill from 3 m on
    assert road[0, 0] == 0.0 and road[-1, 0] > 0.5 and np.all(road[:, 1] == 0.0)
    state = dp["x0"].astype(np.float64)
    unbounded = {k: v for k, v in SOLVER.items() if k != "speed_ceiling"}
    solver, fresh, free = DynamicSamplingSolver(SOLVER), DynamicSamplingSolver(SOLVER), DynamicSamplingSolver(unbounded)
    try:
        obj = solver.solve(state, table, road=road)
        assert obj.info.status == "solved"
        traced = solver.trace()
        assert traced["j"][0].max() >= 3
        plan = solver._plan
        step = dict(dt=0.05, u_min=np.asarray((-0.3, -1.0), dtype=T), u_max=np.asarray((0.3, 1.0), dtype=T), coupling=(1.0, 1.0),
                    speed_ceiling=SOLVER["speed_ceiling"])
        mirror = dm.trace(_vehicle(), state, plan, table[:, :n], road=road, **step)
        assert np.array_equal(mirror["j"], traced["j"][0].astype(np.int64))
        # the ceiling binds: the plan of the same solver without one, on the same road, is over it
        loose = free.solve(state, table, road=road)
        assert loose.info.status == "solved"
        over = dm.trace(_vehicle(), state, free._plan, table[:, :n], road=road, **step)
        assert over["ceiling"].max() > 0.0 and float(mirror["V"][-1]) == 0.0 and float(traced["violation"][0]) == 0.0
        # the plan's cost, float32 on the device against float64 on the host.  Every operand of the cost lines agrees within the
        # CPU file's bound HINGE_TOL (states: STATE_TOL), so a weighted half-square w a^2 / 2 differs by at most w (|a| tol +
        # tol^2 / 2), the progress s = projection of (X, Y) by at most 2 STATE_TOL, and the float32 sums of 4 n + 4 terms round
        # by at most (4 n + 4) 2^-24 of the sum of their magnitudes
        Q, R, QN = np.array((1.0, 1.0, 0.0)), np.array(SOLVER["r_term"]), np.array((1.0, 1.0, 0.0))
        tol = tdr.HINGE_TOL
        lines = [(Q[0], mirror["e_y"]), (Q[1], mirror["e_psi"]), (R[0], mirror["dv"]), (R[1], mirror["dk"]),
                 (QN[0], mirror["e_y"][-1:]), (QN[1], mirror["e_psi"][-1:])]
        stage = sum(0.5 * w * np.sum(a ** 2) for w, a in lines) + 0.5 * QN[2] * (n * 0.05) ** 2
        s, _ = dm.objective_terms(mirror["states"], plan, table[:, :n], progress_weight=3.0)
        want = stage - 3.0 * s
        bound = sum(w * np.sum(np.abs(a) * tol + 0.5 * tol ** 2) for w, a in lines) + 3.0 * 2.0 * tdr.STATE_TOL
        bound += (4 * n + 4) * 2.0 ** -24 * (stage + 3.0 * abs(s))
        assert abs(float(traced["cost"][0]) - want) <= bound, (traced["cost"][0], want, bound)
        # the same plan traced without the table has other states
        without = dm.trace(_vehicle(), state, plan, table[:, :n], **step)
        assert not np.array_equal(without["states"], mirror["states"])
        assert mirror["states"][-1, 3] > without["states"][-1, 3]           # downhill: faster at the end
        # a following solve without `road` gives the bits of a solver that never had one
        a = solver.solve(state, table, warm_steps=0)
        fresh._plan, fresh._calls = plan.copy(), 1
        b = fresh.solve(state, table, warm_steps=0)
        assert np.array_equal(a.x, b.x) and a.cost == b.cost and np.array_equal(a.states, b.states)
    finally:
        solver.close()
        fresh.close()
        free.close()
