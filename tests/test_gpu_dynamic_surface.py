"""Mode D's surface table (acmpc_set_surface) on the MI355X, from every call form.  Costs, keys, feasible counts, records and
traces must be bit-identical to tests/dynamic_surface_spec.py; two forms are held to the kernels that were there before - a table
of ones to the handle without a table, a uniform power-of-two table to the grip-scaled vehicle without one; obstacles ride on
the surface pack; the two-candidates-per-lane kernels gather two waypoints per lane; a table set for another shape is refused;
and DynamicSamplingSolver takes `surface=`.

Shapes: P = 2 on the dense path of dynamic_surface_spec.make_dense_problem (waypoints 1.5 m apart: a 12-step plan crosses
several), problem 0 from a standstill, problem 1 at the path's speed; N = 300 (one full 256-lane workgroup and a tail), n = 12.
Tables are seeded in [0.4, 1], different per problem.  Each test asserts what it relies on: the nearest index reaches 3, and some
step has lanes on different waypoints."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_spec as ds
import dynamic_surface_spec as dss
from dynamic_spec import Settings
import test_dynamic_surface as tds
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
P, N, n = 2, 300, 12
LOAD, AERO = tds.LOAD, tds.AERO
DEFAULT, FINE = tgc.DEFAULT, tgc.FINE
OFF, ALL_FOUR = tgc.OFF, tgc.ALL_FOUR
BIG_OFFSET = tgc.BIG_OFFSET
_vehicle, _u32, _force_pedals = tgc._vehicle, tgc._u32, tgc._force_pedals
_same_where_finite = tgl._same_where_finite
TIERS = {"none": (None, None, None), "coupled": ((1.0, 1.0), None, None), "loaded-coupled-downforce": ((0.9, 1.1), LOAD, AERO)}
GRIPS = (0.5, 0.8, 1.0)     # three vehicles of different grip: they leave a patch boundary at different steps

_cache = {}


def _problems(seed=2401):
    """The two dense problems (shared, never changed: a test that plants controls takes a copy)."""
    if seed not in _cache:
        _cache[seed] = [dss.make_dense_problem(orc, n + 1, N, seed + p, vx0=v) for p, v in enumerate((0.0, None))]
        for d in _cache[seed]:
            _force_pedals(d["U"], n)
    return _cache[seed]


def _tables(seed, count=P):
    return np.stack([dss.random_table(n, seed + p) for p in range(count)])


def _set(eng, ratio, load, aero, setting=OFF, u_prev=None):
    eng.set_dynamics_coupling(ratio)
    eng.set_dynamics_load_transfer(load)
    eng.set_dynamics_downforce(aero)
    eng.set_dynamics_objective(**setting[0])
    eng.set_dynamics_terms(**setting[1])
    eng.set_previous_control(u_prev)


def _crosses_waypoints(j, label=""):
    assert j.max() >= 3, (label, j.max())
    assert any(len(np.unique(j[:, i])) > 1 for i in range(j.shape[1])), label


# ---- the control-matrix solve ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("integration", [DEFAULT, FINE], ids=["euler", "M3-blend"])
@pytest.mark.parametrize("layout,window", [(0, None), (1, (2, 5)), (1, None), (0, (2, 5))])
def test_costs_argmin_and_record_are_the_specification(layout, window, integration, tier):
    from acmpc_amd import _capi
    ratio, load, aero = TIERS[tier]
    dps = _problems()
    u_prev = tgt._previous(P, 41)
    mu = _tables(11)
    eng = tgd._engine(dps, P, N, n, window)
    try:
        eng.set_dynamics_integration(*integration)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        x0 = np.stack([d["x0"] for d in dps])
        _set(eng, ratio, load, aero)
        parent = eng.solve(x0, U_in, layout=layout)["costs"]         # the same handle without the table
        eng.set_surface(mu)
        for name, setting, prev in (("off", OFF, None), ("all four", ALL_FOUR, u_prev)):
            _set(eng, ratio, load, aero, setting, prev)
            out = eng.solve(x0, U_in, layout=layout)
            for p in range(P):
                trace = {}
                cost, V, X = dss.spec_costs(orc, dps[p], eng.coefficients(p), _vehicle().coefficients(), nn_window=window,
                                            return_states=True, settings=Settings(*integration, **setting[0], **setting[1],
                                            coupling=ratio, load_transfer=load, downforce=aero),
                                            u_prev=None if prev is None else prev[p], surface=mu[p], trace=trace)
                label = "%s, problem %d" % (name, p)
                if p == 1:
                    _crosses_waypoints(trace["j"], label)
                tgd._same_bits(out["costs"][p], cost)
                rec = _capi.split_record(out["records"][p], n)
                best = tgd._check_record(rec, U_h[p], cost, V, X, n)
                assert out["best_idx"][p] == best, label
                assert out["n_feasible"][p] == np.count_nonzero(V == 0), label
                tgd._same_bits(rec["cost"], out["costs"][p][best])      # the finalize's re-roll gives the rollout's own cost
                if name == "off" and p == 1:
                    assert not np.array_equal(_u32(out["costs"][p]), _u32(parent[p])), label
        assert np.isnan(out["costs"][0][5]) and not np.isfinite(out["costs"][1][7])
    finally:
        eng.close()


# ---- two forms the kernels that were there before prove ----------------------------------------------------------------------
def _all_forms(dps, vehicles, reduce, update, integration, setting, prev, ratio, load, aero, surface):
    """solve in both layouts, the sampled rollout (costs and keys), acmpc_optimize (its re-drawn records) of one handle."""
    import torch
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    U1 = np.ascontiguousarray(U.transpose(0, 2, 3, 1))
    centre, ref = tsf._centres(dps, n, 5)
    eng = tge._engine(dps, P, N, n, (2, 5), centre_update=update, softmin_lambda=0.5)
    try:
        if len(vehicles) == 1:
            eng.set_dynamics(vehicles[0])
        else:
            eng.set_dynamics_ensemble(vehicles, weights=(1.0, 2.0, 0.5), reduce=reduce)
        eng.set_dynamics_integration(*integration)
        _set(eng, ratio, load, aero, setting, prev)
        eng.set_surface(surface)
        a, b = eng.solve(x0, U), eng.solve(x0, U1, layout=1)
        opt = eng.optimize(x0, centre, ref, N, 2, (0.05, 0.3), shrink=0.5, seed=31)["records"]
        dev, s = torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
        d_x0, d_c = torch.tensor(x0, device=dev), torch.tensor(centre, device=dev)
        costs, keys = torch.empty(P, N, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
        eng.rollout_sampled_device(d_x0.data_ptr(), d_c.data_ptr(), 2 * n, 0, P, N, n, BIG_OFFSET, (0.05, 0.3), 77, 1,
                                   costs.data_ptr(), keys.data_ptr(), s)
        torch.cuda.synchronize()
        return [a["costs"], a["records"], b["costs"], b["records"], opt, costs.cpu().numpy(), keys.cpu().numpy()]
    finally:
        eng.close()


FORMS = [(1, "mean", "argmin", DEFAULT, OFF, (0.9, 1.1), LOAD, AERO), (1, "mean", "softmin", FINE, ALL_FOUR, None, None, None),
         (3, "mean", "softmin", DEFAULT, OFF, (1.0, 1.0), None, None), (3, "max", "argmin", FINE, ALL_FOUR, (0.9, 1.1), LOAD, AERO)]


@pytest.mark.parametrize("K,reduce,update,integration,setting,ratio,load,aero", FORMS,
                         ids=["K1-aero", "K1-plain-softmin", "K3-mean-coupled-softmin", "K3-max-aero"])
def test_ones_and_a_uniform_power_of_two_table_against_the_handle_without_a_table(K, reduce, update, integration, setting, ratio,
                                                                                  load, aero):
    dps = _problems()
    prev = tgt._previous(P, 42) if setting is ALL_FOUR else None
    base = [_vehicle()] if K == 1 else [_vehicle().with_grip(g) for g in GRIPS]
    args = (reduce, update, integration, setting, prev, ratio, load, aero)
    exact = aero is not None      # the table's step IS the handle's: bit for bit; below it, where the parent's value is finite

    def same(got, want, label):
        for q, (g, w) in enumerate(zip(got, want)):
            if exact:
                assert np.array_equal(np.asarray(g).view(np.uint32 if g.dtype == T else g.dtype),
                                      np.asarray(w).view(np.uint32 if w.dtype == T else w.dtype)), (label, q)
            else:
                _same_where_finite(g, w, (label, q))

    plain = _all_forms(dps, base, *args, None)
    same(_all_forms(dps, base, *args, np.ones((P, n, 2), dtype=T)), plain, "ones")
    scaled = [v.with_axle_grip(0.5, 0.25) for v in base]
    want = _all_forms(dps, scaled, *args, None)
    same(_all_forms(dps, base, *args, np.tile(np.array([0.5, 0.25], dtype=T), (P, n, 1))), want, "uniform")
    assert not np.array_equal(_u32(want[0]), _u32(plain[0])) and not np.array_equal(_u32(want[5]), _u32(plain[5]))


# ---- an ensemble under a random table --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce,layout,window,integration,setting,tier", [("mean", 0, None, DEFAULT, OFF, "coupled"),
                                                                           ("max", 1, (2, 5), FINE, ALL_FOUR, "loaded-coupled-downforce")])
def test_ensemble_of_three_is_the_specification(reduce, layout, window, integration, setting, tier):
    from acmpc_amd import _capi
    ratio, load, aero = TIERS[tier]
    dps = _problems()
    vehicles = [_vehicle().with_grip(g) for g in GRIPS]
    weights = (1.0, 2.0, 0.5)
    prev = tgt._previous(P, 43) if setting is ALL_FOUR else None
    mu = _tables(21)
    eng = tge._engine(dps, P, N, n, window)
    try:
        eng.set_dynamics_ensemble(vehicles, weights=weights, reduce=reduce)
        eng.set_dynamics_integration(*integration)
        _set(eng, ratio, load, aero, setting, prev)
        eng.set_surface(mu)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        out = eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)
        s = Settings(*integration, **setting[0], **setting[1], coupling=ratio, load_transfer=load, downforce=aero)
        for p in range(P):
            kw = dict(nn_window=window, settings=s, u_prev=None if prev is None else prev[p], surface=mu[p])
            cost, V, X = dss.spec_ensemble(orc, dps[p], eng.coefficients(p), [v.coefficients() for v in vehicles], reduce=reduce,
                                           weights=weights, return_states=True, **kw)
            if p == 1:   # the three vehicles are on different waypoints at some step: each gathers by its own trajectory
                js = []
                for v in vehicles:
                    trace = {}
                    dss.spec_costs(orc, dps[p], eng.coefficients(p), v.coefficients(), trace=trace, **kw)
                    js.append(trace["j"])
                    _crosses_waypoints(trace["j"])
                assert np.any(js[0] != js[2])
            tgd._same_bits(out["costs"][p], cost)
            rec = _capi.split_record(out["records"][p], n)
            best = tgd._check_record(rec, U_h[p], cost, V, X, n)
            assert out["best_idx"][p] == best and out["n_feasible"][p] == np.count_nonzero(V == 0)
    finally:
        eng.close()


# ---- obstacles over the surface pack --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,layout,integration,tier", [(1, 0, DEFAULT, "none"), (3, 1, FINE, "loaded-coupled-downforce")])
def test_obstacles_ride_on_the_surface_pack(K, layout, integration, tier):
    from acmpc_amd import _capi
    ratio, load, aero = TIERS[tier]
    dps = _problems()
    vehicles = [_vehicle()] if K == 1 else [_vehicle().with_grip(g) for g in GRIPS]
    prev = tgt._previous(P, 44)
    mu = _tables(31)
    discs = [ds.make_obstacles(d, n, 2, 2440 + p) for p, d in enumerate(dps)]
    eng = tge._engine(dps, P, N, n, (2, 5))
    try:
        if K == 1:
            eng.set_dynamics(vehicles[0])
        else:
            eng.set_dynamics_ensemble(vehicles, weights=None, reduce="mean")
        eng.set_dynamics_integration(*integration)
        _set(eng, ratio, load, aero, ALL_FOUR, prev)
        eng.set_dynamics_clearance(40.0, 1.0)
        eng.set_obstacles(np.stack([d[0] for d in discs]), np.stack([d[1] for d in discs]))
        eng.set_surface(mu)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        out = eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)
        s = Settings(*integration, **ALL_FOUR[0], **ALL_FOUR[1], coupling=ratio, load_transfer=load, downforce=aero,
                     clearance_weight=40.0, clearance_margin=1.0)
        for p in range(P):
            cost, V, X = dss.spec_ensemble(orc, dps[p], eng.coefficients(p), [v.coefficients() for v in vehicles], reduce="mean",
                                           nn_window=(2, 5), settings=s, u_prev=prev[p], obstacles=discs[p], surface=mu[p],
                                           return_states=True)
            if K == 1:   # (an ensemble of one is omega = 1: the single vehicle's own cost)
                cost, V, X = dss.spec_costs(orc, dps[p], eng.coefficients(p), vehicles[0].coefficients(), nn_window=(2, 5), settings=s,
                                            u_prev=prev[p], obstacles=discs[p], surface=mu[p], return_states=True)
            tgd._same_bits(out["costs"][p], cost)
            rec = _capi.split_record(out["records"][p], n)
            best = tgd._check_record(rec, U_h[p], cost, V, X, n)
            assert out["best_idx"][p] == best
        # the discs do something, and so does the table under them
        eng.set_obstacles(None)
        assert not np.array_equal(_u32(eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)["costs"]), _u32(out["costs"]))
    finally:
        eng.close()


# ---- the plan trace -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,window,integration,tier,K_obs", [(1, None, DEFAULT, "none", 0), (3, (2, 5), FINE, "loaded-coupled-downforce", 2)])
def test_trace_plans_is_the_specification(K, window, integration, tier, K_obs):
    ratio, load, aero = TIERS[tier]
    dps = _problems()
    vehicles = [_vehicle()] if K == 1 else [_vehicle().with_grip(g) for g in GRIPS]
    prev = tgt._previous(P, 45)
    mu = _tables(41)
    discs = [ds.make_obstacles(d, n, K_obs, 2450 + p) for p, d in enumerate(dps)] if K_obs else None
    eng = tge._engine(dps, P, N, n, window)
    try:
        if K == 1:
            eng.set_dynamics(vehicles[0])
        else:
            eng.set_dynamics_ensemble(vehicles, weights=None, reduce="mean")
        eng.set_dynamics_integration(*integration)
        _set(eng, ratio, load, aero, ALL_FOUR, prev)
        if discs is not None:
            eng.set_obstacles(np.stack([d[0] for d in discs]), np.stack([d[1] for d in discs]))
        eng.set_surface(mu)
        U = np.stack([d["U"][20:23] for d in dps])                       # three plans per problem
        got = eng.trace_plans(np.stack([d["x0"] for d in dps]), U)
        s = Settings(*integration, **ALL_FOUR[0], **ALL_FOUR[1], coupling=ratio, load_transfer=load, downforce=aero)
        per = [dss.trace_plans(dp, eng.coefficients(p), U[p], [v.coefficients() for v in vehicles], s, window, prev[p],
                               None if discs is None else discs[p], surface=mu[p]) for p, dp in enumerate(dps)]
        want = {name: np.stack([t[name] for t in per]) for name in ("states", "totals", "terms")}
        for name in ("states", "terms"):
            assert np.array_equal(ds.bits(got[name]), ds.bits(want[name])), name
        assert np.array_equal(ds.bits(np.stack([got["cost"], got["violation"]], axis=-1)), ds.bits(want["totals"]))
        assert np.array_equal(ds.bits(ds.replay(got["terms"])), ds.bits(got["terms"][..., ds.V_SLOT]))
        assert got["terms"][1, ..., ds.J].max() >= 3      # slot 0 of row i - 1 names the waypoint whose scale step i used
        # and the totals are the rollout's costs of the same plans
        if K == 1 and discs is None:
            out = eng.solve(np.stack([d["x0"] for d in dps]), U)
            assert np.array_equal(ds.bits(out["costs"]), ds.bits(got["cost"][:, :, 0]))
    finally:
        eng.close()


# ---- two candidates per lane ----------------------------------------------------------------------------------------------------
PACKED_N = 4099


def _packed(K):
    """P problems of four dense kinds (problem p is kind p % 4), the smallest P with P N K >= 2^20; a table per kind."""
    count = tpk._problems_for(PACKED_N, K)
    assert count * PACKED_N * K >= tpk.PACKED and (count - 1) * PACKED_N * K < tpk.PACKED
    base = [dss.make_dense_problem(orc, n + 1, PACKED_N, 2460 + q, vx0=v) for q, v in enumerate((None, 0.0, None, 14.0))]
    rng = np.random.default_rng(2460)
    U = np.stack([base[p % 4]["U"] for p in range(count)])
    U[..., 0] += rng.standard_normal(U.shape[:-1], dtype=T) * T(0.01)
    U[..., 0] = np.clip(U[..., 0], ds.U_MIN[0], ds.U_MAX[0])
    x0 = np.stack([base[p % 4]["x0"] for p in range(count)])
    tables = np.stack([base[p % 4]["table"] for p in range(count)])
    kinds = _tables(51, 4)
    return count, base, U, x0, tables, kinds, np.stack([kinds[p % 4] for p in range(count)])


@pytest.mark.parametrize("K,layout,window", [(1, 1, None), (2, 0, (2, 5))])
def test_packed_rollout_gathers_two_waypoints_per_lane(K, layout, window):
    count, base, U, x0, tables, kinds, mu = _packed(K)
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
        _set(eng, (0.9, 1.1), LOAD, AERO, ALL_FOUR, None)
        eng.set_surface(mu)
        U_in = tpk._as_layout(U, layout)
        out = eng.solve(x0, U_in, layout=layout)
        coefs = [eng.coefficients(q) for q in range(4)]
        s = Settings(*DEFAULT, **ALL_FOUR[0], **ALL_FOUR[1], coupling=(0.9, 1.1), load_transfer=LOAD, downforce=AERO)

        def spec(q, U_sub, states):
            return dss.spec_ensemble(orc, base[q], coefs[q], [v.coefficients() for v in vehicles], reduce="mean",
                                     weights=(1.0, 2.0)[:K], nn_window=window, U=U_sub, return_states=states, settings=s,
                                     surface=kinds[q])

        trace = {}
        dss.spec_costs(orc, base[0], coefs[0], vehicles[0].coefficients(), nn_window=window, U=U[0][:64], settings=s,
                       surface=kinds[0], trace=trace)
        _crosses_waypoints(trace["j"], label)
        assert np.any(trace["j"][0::2] != trace["j"][1::2])     # the two candidates of a lane on different waypoints
        group = tpk.GROUP_ONE if K == 1 else tpk.GROUP_ENSEMBLE
        tpk._check_against_spec(out, base, coefs, U, PACKED_N, n, group, planted, spec, 7 + K, label)
        # packed against unpacked slices of the same handle, each slice with its own rows of the table
        chunk = (tpk.PACKED - 1) // (PACKED_N * K)
        assert 1 <= chunk < count
        for lo in range(0, count, chunk):
            hi = min(lo + chunk, count)
            eng.set_paths(tables[lo:hi])
            eng.set_surface(mu[lo:hi])
            part = eng.solve(x0[lo:hi], U_in[lo:hi], layout=layout)
            tgd._same_bits(part["costs"], out["costs"][lo:hi])
            assert np.array_equal(part["best_idx"], out["best_idx"][lo:hi]), label
            assert np.array_equal(part["records"].view(np.uint32), out["records"][lo:hi].view(np.uint32)), label
    finally:
        eng.close()


# ---- a table for another shape --------------------------------------------------------------------------------------------------
def test_a_table_for_another_shape_is_refused_and_the_handle_stays_usable():
    from acmpc_amd import EngineError
    dps = _problems()
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    centre, ref = tsf._centres(dps, n, 5)
    mu = _tables(61)
    eng = tgd._engine(dps, P, N, n, (2, 5))
    try:
        eng.set_surface(mu)
        want = eng.solve(x0, U)
        for wrong in (mu[:1], mu[:, : n - 1]):
            eng.set_surface(wrong)
            for call in (lambda: eng.solve(x0, U), lambda: eng.optimize(x0, centre, ref, N, 2, (0.05, 0.3), shrink=0.5, seed=31),
                         lambda: eng.trace_plans(x0, U[:, :2])):
                with pytest.raises(EngineError) as e:
                    call()
                assert e.value.code == ESTATE and "acmpc_set_surface" in str(e.value)
        eng.set_surface(mu)
        again = eng.solve(x0, U)
        assert np.array_equal(_u32(again["costs"]), _u32(want["costs"])) and np.array_equal(_u32(again["records"]), _u32(want["records"]))
        eng.set_surface(None)
        never = tgd._engine(dps, P, N, n, (2, 5))
        try:
            assert np.array_equal(_u32(eng.solve(x0, U)["costs"]), _u32(never.solve(x0, U)["costs"]))
        finally:
            never.close()
    finally:
        eng.close()


# ---- the solver -----------------------------------------------------------------------------------------------------------------
SOLVER = dict(horizon=n + 1, n_candidates=2048, sampling_rounds=2, sampling_sigma=(0.02, 0.3), sampling_seed=11, progress_cost=3.0,
              r_term=(0.0, 10.0), tyre_coupling=(1.0, 1.0), plan_states=True)


def test_dynamic_sampling_solver_takes_a_surface():
    from acmpc_amd import dynamic_model as dm
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    dp = _problems()[1]
    table = dp["table"]
    arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(table[0]), np.diff(table[1])))])[:n]
    mu = dm.surface_table(arc, [(3.0, 9.0, 0.6), (7.0, 100.0, 0.8, 0.7)])
    assert len(np.unique(mu[:, 0])) == 3 and mu[0, 0] == 1.0
    state = dp["x0"].astype(np.float64)
    solver, fresh = DynamicSamplingSolver(SOLVER), DynamicSamplingSolver(SOLVER)
    try:
        obj = solver.solve(state, table, surface=mu)
        assert obj.info.status == "solved"
        traced = solver.trace()
        assert traced["j"][0].max() >= 3
        plan = solver._plan
        mirror = dm.trace(_vehicle(), state, plan, table[:, :n], dt=0.05, u_min=np.asarray((-0.3, -1.0), dtype=T),
                          u_max=np.asarray((0.3, 1.0), dtype=T), coupling=(1.0, 1.0), surface=mu)
        assert np.array_equal(mirror["j"], traced["j"][0].astype(np.int64))
        # the plan's cost proper under the table, float32 on the device against float64 on the host: the bound of the CPU file
        Q, R, QN = np.array((1.0, 1.0, 0.0)), np.array(SOLVER["r_term"]), np.array((1.0, 1.0, 0.0))
        stage = 0.5 * (Q[0] * np.sum(mirror["e_y"] ** 2) + Q[1] * np.sum(mirror["e_psi"] ** 2) + R[0] * np.sum(mirror["dv"] ** 2)
                       + R[1] * np.sum(mirror["dk"] ** 2))
        terminal = 0.5 * (QN[0] * mirror["e_y"][-1] ** 2 + QN[1] * mirror["e_psi"][-1] ** 2 + QN[2] * (n * 0.05) ** 2)
        s, _ = dm.objective_terms(mirror["states"], plan, table[:, :n], progress_weight=3.0)
        want = stage + terminal - 3.0 * s
        assert float(mirror["V"][-1]) == 0.0 and float(traced["violation"][0]) == 0.0
        assert abs(float(traced["cost"][0]) - want) <= tds.MIRROR_RTOL * max(abs(want), 1.0), (traced["cost"][0], want)
        # without the table the plan's trace is another
        without = dm.trace(_vehicle(), state, plan, table[:, :n], dt=0.05, coupling=(1.0, 1.0))
        assert not np.array_equal(without["states"], mirror["states"])
        # a following solve without `surface` gives the bits of a solver that never had one
        a = solver.solve(state, table, warm_steps=0)
        fresh._plan, fresh._calls = plan.copy(), 1
        b = fresh.solve(state, table, warm_steps=0)
        assert np.array_equal(a.x, b.x) and a.cost == b.cost and np.array_equal(a.states, b.states)
    finally:
        solver.close()
        fresh.close()
