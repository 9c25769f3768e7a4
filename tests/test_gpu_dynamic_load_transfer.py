"""Mode D's longitudinal load transfer (acmpc_set_dynamics_load_transfer) on the MI355X, from every call form.  Costs, keys,
feasible counts and records must be bit-identical to tests/dynamic_spec.py - alone on the small shapes, and through the
forms already held to it (the one-candidate-per-lane kernels, the control matrix) on the large ones; a handle with h_cg = 0 runs
the loaded kernels and must give the bits of the same handle without the setting, coupled or not; a handle whose setting is off
must give the bits of a handle that never heard of the call; acmpc_score_grips takes the handle's setting with the base
vehicle's factors on each hypothesis' own peaks; and DynamicSamplingSolver with `load_transfer` drives the loop of
test_gpu_dynamic_coupling on a plant whose axle loads move."""
import dataclasses

import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_ensemble_spec as es
import dynamic_sampled_spec as dss
import dynamic_spec as ds
from dynamic_spec import Settings
import grip_spec as gs
import test_gpu_dynamic as tgd
import test_gpu_dynamic_coupling as tgc
import test_gpu_dynamic_ensemble as tge
import test_gpu_dynamic_objective as tgo
import test_gpu_dynamic_packed as tpk
import test_gpu_dynamic_sampled as tsm
import test_gpu_dynamic_softmin as tsf
import test_gpu_dynamic_terms as tgt
import test_gpu_grip_identification as tgi

pytestmark = pytest.mark.gpu

T = np.float32
LOAD = (0.35, 0.9)
DEFAULT, FINE = tgc.DEFAULT, tgc.FINE
RATIOS = tgc.RATIOS
BIG_OFFSET = tgc.BIG_OFFSET
OFF, ALL_FOUR = tgc.OFF, tgc.ALL_FOUR
GRID = tgc.GRID
_vehicle, _grip_vehicles, _u32, _force_pedals = tgc._vehicle, tgc._grip_vehicles, tgc._u32, tgc._force_pedals


def _set(eng, ratio, load, setting=OFF, u_prev=None):
    eng.set_dynamics_coupling(ratio)
    eng.set_dynamics_load_transfer(load)
    eng.set_dynamics_objective(**setting[0])
    eng.set_dynamics_terms(**setting[1])
    eng.set_previous_control(u_prev)


def _same_where_finite(got, want, label=""):
    """Bit-identical where the parent's value is finite; non-finite where the parent's is (the identities hold for finite
    forces: a NaN or an infinity of the parent may be the other of the two here)."""
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype != np.float32:
        assert np.array_equal(got, want), label
        return
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite), label
    assert np.array_equal(got[finite].view(np.uint32), want[finite].view(np.uint32)), label


# ---- one candidate per lane ---------------------------------------------------------------------------------------------
# test_gpu_dynamic_coupling's shape and forced candidates: P = 2, N = 300 (one full 256-lane workgroup and a tail), n = 12;
# problem 0 starts from a standstill, problem 1 at the path's speed.
@pytest.mark.parametrize("ratio", RATIOS + [None], ids=["1-1", "0.9-1.1", "uncoupled"])
@pytest.mark.parametrize("integration", [DEFAULT, FINE], ids=["euler", "M3-blend"])
@pytest.mark.parametrize("layout,window", [(0, None), (1, (2, 5)), (1, None), (0, (2, 5))])
def test_costs_argmin_and_record_are_the_specification(layout, window, integration, ratio):
    from acmpc_amd import _capi
    P, N, n = 2, 300, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 2300 + p, vx0=v) for p, v in enumerate((0.0, None))]
    for d in dps:
        _force_pedals(d["U"], n)
    u_prev = tgt._previous(P, 31)
    eng = tgd._engine(dps, P, N, n, window)
    try:
        eng.set_dynamics_integration(*integration)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        x0 = np.stack([d["x0"] for d in dps])
        eng.set_dynamics_coupling(ratio)
        parent = eng.solve(x0, U_in, layout=layout)["costs"]         # the same handle without the load transfer
        for name, setting, prev in (("off", OFF, None), ("all four", ALL_FOUR, u_prev)):
            _set(eng, ratio, LOAD, setting, prev)
            out = eng.solve(x0, U_in, layout=layout)
            for p in range(P):
                cost, V, X = ds.spec_costs(orc, dps[p], eng.coefficients(p), _vehicle().coefficients(), nn_window=window,
                                           return_states=True, settings=Settings(*integration, **setting[0], **setting[1],
                                           coupling=ratio, load_transfer=LOAD), u_prev=None if prev is None else prev[p])
                label = "%s, problem %d" % (name, p)
                tgd._same_bits(out["costs"][p], cost)
                rec = _capi.split_record(out["records"][p], n)
                best = tgd._check_record(rec, U_h[p], cost, V, X, n)
                assert out["best_idx"][p] == best, label
                assert out["n_feasible"][p] == np.count_nonzero(V == 0), label
                tgd._same_bits(rec["cost"], out["costs"][p][best])      # the finalize's re-roll gives the rollout's own cost
                if name == "off":
                    # the zero-pedal candidate has the parent setting's bits; at speed, full brake and full drive have not
                    tgd._same_bits(out["costs"][p][11], parent[p][11])
                    for c in ((10, 12, 13, 14) if p == 1 else ()):
                        assert out["costs"][p][c] != parent[p][c], (label, c)
            assert np.isnan(out["costs"][0][5]) and not np.isfinite(out["costs"][1][7])
    finally:
        eng.close()


# ---- h_cg = 0: the loaded kernels, the parent's bits ------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_zero_height_runs_the_loaded_kernels_and_gives_the_parents_bits(K):
    """Every call form of test_infinite_ratios_run_the_coupled_kernels...: solve in both layouts, the sampled rollout and its
    record, acmpc_optimize with argmin and softmin, and acmpc_score_grips - coupled and uncoupled, under the default
    integration and the fine one, with all four term parts and with none."""
    P, N, n = 2, 300, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 2310 + p, vx0=v) for p, v in enumerate((0.0, None))]
    for d in dps:
        _force_pedals(d["U"], n)
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    U1 = np.ascontiguousarray(U.transpose(0, 2, 3, 1))
    centre, ref = tsf._centres(dps, n, 5)
    u_prev = tgt._previous(P, 32)
    states, controls = gs.braking_log(_vehicle().with_grip(0.5), (1.0, 1.0), steps=20)
    scales = tgi._scales(70)

    def run(ratio, load, update, integration, setting, prev):
        import torch
        eng = tge._engine(dps, P, N, n, (2, 5), centre_update=update, softmin_lambda=0.5)
        try:
            if K == 1:
                eng.set_dynamics(_vehicle())
            else:
                eng.set_dynamics_ensemble(_grip_vehicles(), weights=(1.0, 2.0, 0.5), reduce="mean")
            eng.set_dynamics_integration(*integration)
            _set(eng, ratio, load, setting, prev)
            a, b = eng.solve(x0, U), eng.solve(x0, U1, layout=1)
            opt = eng.optimize(x0, centre, ref, N, 2, (0.05, 0.3), shrink=0.5, seed=31)["records"]
            dev, s = torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
            d_x0, d_c = torch.tensor(x0, device=dev), torch.tensor(centre, device=dev)
            costs, keys = torch.empty(P, N, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
            eng.rollout_sampled_device(d_x0.data_ptr(), d_c.data_ptr(), 2 * n, 0, P, N, n, BIG_OFFSET, (0.05, 0.3), 77, 1,
                                       costs.data_ptr(), keys.data_ptr(), s)
            torch.cuda.synchronize()
            errors, best = eng.score_grips(states, controls, 0.05, scales, segment=5)
            return [a["costs"], a["records"], b["costs"], b["records"], opt, costs.cpu().numpy(), keys.cpu().numpy(), errors,
                    np.array([best])]
        finally:
            eng.close()

    for ratio, update, integration, setting, prev in (((0.9, 1.1), "argmin", DEFAULT, OFF, None),
                                                      (None, "softmin", FINE, ALL_FOUR, u_prev),
                                                      (None, "softmin", DEFAULT, OFF, None),
                                                      ((0.9, 1.1), "argmin", FINE, ALL_FOUR, u_prev)):
        want = run(ratio, None, update, integration, setting, prev)
        got = run(ratio, (0.0, 0.9), update, integration, setting, prev)
        for q, (g, w) in enumerate(zip(got, want)):
            _same_where_finite(g, w, (ratio, update, q))
        loaded = run(ratio, LOAD, update, integration, setting, prev)
        # a height does something - to the identification only under the coupling: uncoupled, the straight-line braking log
        # has no side force and its longitudinal forces do not know the peaks
        assert not np.array_equal(_u32(loaded[0]), _u32(want[0]))
        assert np.array_equal(_u32(loaded[7]), _u32(want[7])) == (ratio is None)


# ---- handle hygiene ---------------------------------------------------------------------------------------------------------
def test_load_transfer_off_is_a_handle_that_never_made_the_call():
    """NULL; set then switched off; set then refused from off: costs, records and acmpc_optimize's records of a handle that
    never called - alone, and beside the coupling with all four term parts, whose kernels are then the ones that ran before.
    A refusal while on leaves the setting, and it survives acmpc_set_dynamics, _ensemble, _integration, _terms, _objective and
    _coupling."""
    P, N, n = 2, 700, 30
    dps = tgd._problems(P, N, n, seed=2320)
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    centre = np.tile(np.stack([np.zeros(n), np.full(n, 0.2)], axis=1).astype(T), (P, 1, 1))
    ratio = (0.9, 1.1)

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
        assert eng._lib.acmpc_set_dynamics_load_transfer(eng._ctx, None) == 0

    def there_and_back(eng):
        eng.set_dynamics_load_transfer(LOAD)
        assert differs(eng, never[0])
        eng.set_dynamics_load_transfer(None)

    def refused(eng):
        for bad in ((-1.0, 0.9), (0.35, 0.0), (0.35, 1.0), (float("nan"), 0.9)):
            r = np.array(bad)
            assert eng._lib.acmpc_set_dynamics_load_transfer(eng._ctx, r.ctypes.data) == -1

    never = run(lambda eng: None)
    for prepare in (explicit_off, there_and_back, refused):
        for got, want in zip(run(prepare), never):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), prepare.__name__

    def coupled_four_only(eng):
        eng.set_dynamics_coupling(ratio)
        eng.set_dynamics_objective(**ALL_FOUR[0])
        eng.set_dynamics_terms(**ALL_FOUR[1])

    def coupled_four_and_back(eng):
        coupled_four_only(eng)
        eng.set_dynamics_load_transfer(LOAD)
        assert differs(eng, termed[0])
        eng.set_dynamics_load_transfer(None)

    termed = run(coupled_four_only)
    for got, want in zip(run(coupled_four_and_back), termed):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

    # a refused setting leaves the one that was on; the setting survives every other one
    def refused_while_on(eng):
        eng.set_dynamics_load_transfer(LOAD)
        refused(eng)

    def survives(eng):
        eng.set_dynamics_load_transfer(LOAD)
        eng.set_dynamics_integration(*FINE)
        eng.set_dynamics_ensemble([_vehicle(), _vehicle().with_grip(0.6)])
        eng.set_dynamics(_vehicle())
        eng.set_dynamics_terms(**tgt.BOTH)
        eng.set_dynamics_terms()
        eng.set_dynamics_objective(2.0, 1.1)
        eng.set_dynamics_objective()
        eng.set_dynamics_coupling(ratio)
        eng.set_dynamics_coupling(None)
        eng.set_dynamics_integration(1, None)

    want = run(lambda eng: eng.set_dynamics_load_transfer(LOAD))
    assert not np.array_equal(want[0].view(np.uint32), never[0].view(np.uint32))
    for prepare in (refused_while_on, survives):
        for got, w in zip(run(prepare), want):
            assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), prepare.__name__
    for p in range(P):   # (and that is the specification's)
        cost = ds.spec_costs(orc, dps[p], orc.coefficients_temporal(dps[p]["table"], dps[p]["kw"]["margin"]).astype(T),
                             _vehicle().coefficients(), nn_window=(2, 5), settings=Settings(*DEFAULT, **OFF[0], **OFF[1],
                             coupling=None, load_transfer=LOAD))[0]
        tgd._same_bits(want[0][p], cost)


# ---- ensembles -------------------------------------------------------------------------------------------------------------
def _geometry_vehicles():
    """Members that differ in lf / lr - lf +-0.1 with lr -+0.1, at the same wheelbase - so that w_max, a1, a2 are per vehicle,
    and a fourth with a longer wheelbase, so that c_h is too."""
    v = _vehicle()
    return [v, dataclasses.replace(v, lf=v.lf + 0.1, lr=v.lr - 0.1), dataclasses.replace(v, lf=v.lf - 0.1, lr=v.lr + 0.1),
            dataclasses.replace(v, lf=v.lf + 0.05)]


@pytest.mark.parametrize("members", ["grips", "geometry"])
@pytest.mark.parametrize("reduce,layout,window,integration,setting,ratio", [("mean", 0, None, DEFAULT, OFF, (1.0, 1.0)),
                                                                            ("max", 1, (2, 5), FINE, ALL_FOUR, (0.9, 1.1))])
def test_ensemble_is_the_specification(reduce, layout, window, integration, setting, ratio, members):
    from acmpc_amd import _capi
    P, N, n = 2, 300, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 2330 + p, vx0=v) for p, v in enumerate((0.0, None))]
    for d in dps:
        _force_pedals(d["U"], n)
    vehicles = _grip_vehicles() if members == "grips" else _geometry_vehicles()
    blocks = [v.coefficients() for v in vehicles]
    if members == "geometry":
        scalars = [ds.constants(b, Settings(load_transfer=LOAD)).k for b in blocks]
        for key in ds.LOAD_KEYS:                                                  # really per vehicle
            assert len(set(float(s[key]) for s in scalars)) == (2 if key == "c_h" else 4), key
    weights = (1.0, 2.0, 0.5, 1.5)[:len(vehicles)] if reduce == "mean" else None
    u_prev = tgt._previous(P, 33) if setting is ALL_FOUR else None
    eng = tge._engine(dps, P, N, n, window)
    try:
        _set(eng, ratio, LOAD, setting, u_prev)               # before the vehicles: nothing to check yet
        eng.set_dynamics_ensemble(vehicles, weights=weights, reduce=reduce)
        eng.set_dynamics_integration(*integration)
        U_h = np.stack([d["U"] for d in dps])
        U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
        out = eng.solve(np.stack([d["x0"] for d in dps]), U_in, layout=layout)
        for p in range(P):
            prev = None if u_prev is None else u_prev[p]
            J, V, X = es.spec_ensemble(orc, dps[p], eng.coefficients(p), blocks, reduce=reduce, weights=weights, nn_window=window,
                                       return_states=True, settings=Settings(*integration, **setting[0], **setting[1],
                                       coupling=ratio, load_transfer=LOAD), u_prev=prev)
            tgd._same_bits(out["costs"][p], J)
            best = tgd._check_record(_capi.split_record(out["records"][p], n), U_h[p], J, V, X, n)
            assert out["best_idx"][p] == best
    finally:
        eng.close()


def test_ensemble_of_one_is_the_single_vehicle():
    P, N, n = 2, 300, 12
    dps = [ds.make_dynamic_problem(orc, "monza", n + 1, N, 2340 + p, vx0=v) for p, v in enumerate((1.0, None))]
    x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
    eng = tge._engine(dps, P, N, n, (2, 5))
    try:
        _set(eng, (0.9, 1.1), LOAD, ALL_FOUR, tgt._previous(P, 34))
        eng.set_dynamics(_vehicle().with_grip(0.8))
        single = eng.solve(x0, U)
        eng.set_dynamics_ensemble([_vehicle().with_grip(0.8)], reduce="mean")
        one = eng.solve(x0, U)
        assert np.array_equal(one["costs"].view(np.uint32), single["costs"].view(np.uint32))
        assert np.array_equal(one["records"].view(np.uint32), single["records"].view(np.uint32))
        eng.set_dynamics_load_transfer(None)
        assert not np.array_equal(eng.solve(x0, U)["costs"].view(np.uint32), single["costs"].view(np.uint32))
    finally:
        eng.close()


# ---- two candidates per lane ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,layout,window,integration,setting", [(1, 1, (2, 5), DEFAULT, OFF), (3, 0, None, FINE, ALL_FOUR)])
def test_packed_rollout(K, layout, window, integration, setting):
    """test_gpu_dynamic_coupling's packed launch (N = 4099, n = 4, P N K >= 2^20) with the load transfer: the f32x2 step loop.
    In full against the one-candidate-per-lane kernels - two shards of candidates by index_offset, each below 2^20 - and
    against the specification on test_gpu_dynamic_packed's subset."""
    import torch
    from acmpc_amd import _capi
    ratio = (0.9, 1.1)
    N, n = 4099, 4
    P = tpk._problems_for(N, K)
    half = (N + 1) // 2
    assert P * N * K >= tpk.PACKED and P * half * K < tpk.PACKED
    label = "K %d layout %d window %s P %d" % (K, layout, window, P)
    base, U, x0, tables = tpk._make(P, N, n, seed=2350 + K)
    x0[2::4, 3] = 4.0
    U[:, 20, :, 1], U[:, 21, :, 1], U[:, 23, :, 1] = -1.0, 1.0, 0.0
    planted = tpk._plant(U, N, n)
    by_kind = tgt._previous(4, 36)
    u_prev = by_kind[np.arange(P) % 4] if setting is ALL_FOUR else None
    vehicles = [_vehicle()] if K == 1 else _grip_vehicles()
    eng = tge._engine([base[p % 4] for p in range(P)], P, N, n, window)
    try:
        eng.set_dynamics_integration(*integration)
        _set(eng, ratio, LOAD, setting, u_prev)
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
            prev = None if u_prev is None else by_kind[q]
            if K == 1:
                return ds.spec_costs(orc, dp, coefs[q], blocks[0], nn_window=window, U=U_sub, return_states=states,
                                     settings=Settings(*integration, **setting[0], **setting[1], coupling=ratio,
                                                       load_transfer=LOAD), u_prev=prev)
            return es.spec_ensemble(orc, dp, coefs[q], blocks, reduce="mean", nn_window=window, U=U_sub, return_states=states,
                                    settings=Settings(*integration, **setting[0], **setting[1], coupling=ratio,
                                                      load_transfer=LOAD), u_prev=prev)

        tpk._check_against_spec(whole, base, coefs, U, N, n, tpk.GROUP_ONE if K == 1 else tpk.GROUP_ENSEMBLE, planted, spec,
                                67 + K, label)
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


# ---- the sampled forms and acmpc_optimize -----------------------------------------------------------------------------------
def _rig(P, N, n, K, window, seed, integration, ratio, setting=ALL_FOUR, **kw):
    rig = tsm.Rig(P, N, n, K=K, window=window, seed=seed, **dict(tgc.GRIPS3 if K == 3 else {}, **kw))
    rig.u_prev = tgt._previous(P, seed)
    rig.eng.set_dynamics_integration(*integration)
    _set(rig.eng, ratio, LOAD, setting, rig.u_prev)
    return rig


@pytest.mark.parametrize("P,N,n,K,window,with_ref,rnd,offset,integration", [
    (3, 1537, 30, 1, (2, 5), True, 2, 0, DEFAULT),
    (1, 1000, 49, 1, None, False, 1, BIG_OFFSET, FINE),
    (3, 300, 49, 3, (2, 5), True, 0, BIG_OFFSET, DEFAULT),
    (1, 131, 8, 3, None, True, 1, 0, FINE),
])
def test_fused_rollout_equals_sample_then_rollout(P, N, n, K, window, with_ref, rnd, offset, integration):
    rig = _rig(P, N, n, K, window, 2360 + n, integration, (0.9, 1.1), with_ref=with_ref, kinds=[(1, 0, 3)[p % 3] for p in range(P)])
    try:
        sigma, seed = (0.04, 0.6), 0xC0FFEE1234          # (a pedal spread that reaches both caps)
        U, costs, keys = tsm._compare_rollouts(rig, N, offset, sigma, seed, rnd)
        tsm._compare_records(rig, U, keys, N, offset, sigma, seed, rnd)
    finally:
        rig.close()


@pytest.mark.parametrize("K", [1, 3])
def test_fused_rollout_and_optimize_equal_the_specification(K):
    """96 x 12 against the restatements alone: the fused rollout's costs, key and count, the re-drawn record, and
    acmpc_optimize's argmin rounds."""
    from acmpc_amd import _capi
    ratio = (1.0, 1.0)
    P, N, n, sigma, seed, rnd, window = 2, 96, 12, (0.05, 0.6), 99, 3, (2, 5)
    rig = _rig(P, N, n, K, window, 2370, FINE, ratio, with_ref=True, kinds=[1, 0])
    try:
        for offset in (0, BIG_OFFSET):
            costs, keys = rig.fused(N, offset, sigma, seed, rnd)
            rec = rig.finalize_sampled(None, N, sigma, seed, rnd)
            for p in range(P):
                want = dss.rollout_sampled(orc, rig.dps[p], rig.eng.coefficients(p), rig.blocks(), rig.centre_h[p], rig.ref_h[p],
                                           N, offset, p, rnd, seed, sigma, reduce=rig.reduce, weights=rig.weights,
                                           nn_window=window, return_states=True, settings=Settings(*FINE, **ALL_FOUR[0],
                                           **ALL_FOUR[1], coupling=ratio, load_transfer=LOAD), u_prev=rig.u_prev[p])
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
                                       return_states=True, settings=Settings(*FINE, **ALL_FOUR[0], **ALL_FOUR[1], coupling=ratio,
                                       load_transfer=LOAD), u_prev=rig.u_prev[p])
                centre = U[orc.pick_best(cost)[0]]
            tgd._check_record(_capi.split_record(got[p], n), U, cost, V, X, n)
    finally:
        rig.close()


@pytest.mark.parametrize("update", ["argmin", "softmin"])
@pytest.mark.parametrize("vehicles", [None, (0, 1, 2)], ids=["K1", "K3"])
def test_optimize_with_and_without_the_matrix_and_the_sharded_optimizer(vehicles, update):
    """Rounds 2, both centre updates: the default rounds (no control matrix) against ACMPC_DYNAMIC_MATRIX_ROUNDS=1 - whose
    costs are the solve's, held to the specification above - bit for bit, and ShardedOptimizer at world size 1 against both:
    the handle carries the setting."""
    import torch
    from acmpc_amd.sharding import ShardedOptimizer
    P, N, n, rounds, sigma, shrink, seed = 2, 1025, 30, 2, (0.05, 0.6), 0.5, 1234
    eng, dps = tsf._dynamic_engine(P, N, n, seed=2380, vehicles=vehicles, window=(2, 5), centre_update=update,
                                   softmin_lambda=0.5)
    try:
        centre, ref = tsf._centres(dps, n, 3)
        x0 = np.stack([d["x0"] for d in dps])
        eng.set_dynamics_coupling((1.0, 1.0))
        coupled = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        eng.set_dynamics_load_transfer(0.35)
        default = eng.optimize(x0, centre, ref, N, rounds, sigma, shrink=shrink, seed=seed)["records"]
        assert not np.array_equal(coupled.view(np.uint32), default.view(np.uint32))   # (the setting reaches these rounds)
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


# ---- acmpc_score_grips under the load transfer ------------------------------------------------------------------------------
def _braking_log(W):
    """test_gpu_dynamic_coupling's log that brakes hard and steers, driven on the loaded, coupled mirror at grip 0.7."""
    rng = np.random.default_rng(2200 + W)
    t = np.arange(W) * 0.05
    controls = np.stack([0.02 * np.sin(np.pi * t) + 0.01, np.clip(-0.6 + 0.4 * np.sin(2.0 * t) + 0.05 * rng.standard_normal(W), -1, 1)],
                        axis=1).astype(T)
    traj = _vehicle().with_grip(0.7).rollout(np.array([0.0, 0.0, 0.0, 40.0, 0.0, 0.0]), controls.astype(np.float64), 0.05,
                                             substeps=4, coupling=(1.0, 1.0), load_transfer=LOAD)
    return traj[:, 3:].astype(T), controls


@pytest.mark.parametrize("integration", [(1, None), (4, (3.0, 5.0))], ids=["default", "fine"])
@pytest.mark.parametrize("L,K", [(1, 25), (8, 625), (40, 25), (1, 625)])
def test_score_grips_is_the_specification(L, K, integration):
    from acmpc_amd.grip_estimator import grip_scales
    W, ratio = 40, (0.9, 1.1)
    states, controls = _braking_log(W)
    scales = grip_scales(GRID, "tied" if K == 25 else "split")
    eng = tgi._engine(integration)
    try:
        eng.set_dynamics_coupling(ratio)
        coupled, _ = eng.score_grips(states, controls, 0.05, scales, segment=L)
        eng.set_dynamics_load_transfer(LOAD)
        errors, best = eng.score_grips(states, controls, 0.05, scales, segment=L)
        want, want_best = gs.score(_vehicle().coefficients(), states, controls, 0.05, scales, segment=L,
                                   settings=Settings(substeps=integration[0], low_speed_blend=integration[1], coupling=ratio,
                                                     load_transfer=LOAD))
        tgi._same_bits(errors, want)
        assert best == want_best and np.isfinite(want).all()
        assert not np.array_equal(_u32(errors), _u32(coupled))
        eng.set_dynamics_load_transfer(None)
        again, _ = eng.score_grips(states, controls, 0.05, scales, segment=L)
        tgi._same_bits(again, coupled)
        # without the coupling: the loaded identify kernel with both ratios +inf
        eng.set_dynamics_coupling(None)
        eng.set_dynamics_load_transfer(LOAD)
        errors, best = eng.score_grips(states, controls, 0.05, scales, segment=L)
        want, want_best = gs.score(_vehicle().coefficients(), states, controls, 0.05, scales, segment=L,
                                   settings=Settings(substeps=integration[0], low_speed_blend=integration[1], load_transfer=LOAD))
        tgi._same_bits(errors, want)
        assert best == want_best
    finally:
        eng.close()


def test_score_grips_finds_the_grip_of_a_straight_line_braking_log():
    from acmpc_amd.grip_estimator import grip_scales
    tied = grip_scales(GRID, "tied")
    states, controls = gs.braking_log(_vehicle().with_grip(0.5), (1.0, 1.0), LOAD)
    eng = tgi._engine()
    try:
        eng.set_dynamics_coupling(1.0)
        eng.set_dynamics_load_transfer(LOAD)
        errors, best = eng.score_grips(states, controls, 0.05, tied)
        assert tied[best, 0] == pytest.approx(0.5)
        want, want_best = gs.score(_vehicle().coefficients(), states, controls, 0.05, tied, settings=Settings(coupling=(1.0, 1.0),
                                   load_transfer=LOAD))
        tgi._same_bits(errors, want)
        assert best == want_best and errors[best] < 1e-6 < np.sort(errors)[1]
    finally:
        eng.close()


def test_a_solve_gives_the_same_bits_before_and_after_score_grips():
    P, N, n = 2, 512, 30
    dps = tgd._problems(P, N, n, seed=2390)
    eng = tgd._engine(dps, P, N, n, (2, 5))
    try:
        eng.set_dynamics_ensemble(_grip_vehicles(), reduce="mean")
        _set(eng, (0.9, 1.1), LOAD, ALL_FOUR, np.array([[0.01, 0.1], [0.0, -0.2]], dtype=T))
        x0, U = np.stack([d["x0"] for d in dps]), np.stack([d["U"] for d in dps])
        before = eng.solve(x0, U)
        states, controls = _braking_log(40)
        errors, best = eng.score_grips(states, controls, 0.05, tgi._scales(625), segment=8)
        assert np.isfinite(errors).all()
        after = eng.solve(x0, U)
        tgd._same_bits(after["costs"], before["costs"])
        tgd._same_bits(after["records"], before["records"])
        assert list(after["best_idx"]) == list(before["best_idx"])
    finally:
        eng.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------------
# The loop of test_gpu_dynamic_coupling (its circuit, tick count, bars and progress configuration LOOP_B) on a plant that has the
# friction ellipse AND the load transfer: the float64 mirror coupled at (1, 1) with (0.35, 0.9).  The solver with
# `tyre_coupling: 1.0, load_transfer: 0.35` must solve every tick and stay inside the project's corridor and slip bars.  The same
# plant with `tyre_coupling` alone is run and logged beside it: its figures are recorded, not asserted.
def _run_loop(config):
    """tgc._run_loop's loop with the loaded, coupled plant."""
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
            solved = obj.info.status == "solved"
            if solved:
                u = obj.x[3 * (n + 1):].reshape(n, 2)
                state = plant.predict_next_state(state, u[0], tgd.LOOP_DT, coupling=tgc.LOOP_RATIO, load_transfer=LOAD)[0]
                state[3] = max(state[3], 0.0)
            ey, i = tgd.loop_frenet(centre, heading, state)
            log.append((ey, abs(state[4]) / max(state[3], 1.0), i, state[3], float(solved)))
            if not solved:
                break
    finally:
        solver.close()
    log = np.array(log)
    steps = np.diff(np.concatenate([[start], log[:, 2]])) % len(centre)       # centre-line samples passed per tick, 0.5 m each
    return log, 0.5 * float(np.sum(np.where(steps > len(centre) // 2, steps - len(centre), steps)))


def test_closed_loop_on_a_plant_whose_axle_loads_move():
    log, dist = _run_loop(dict(tgo.LOOP_B, tyre_coupling=1.0, load_transfer=0.35))
    other, other_dist = _run_loop(dict(tgo.LOOP_B, tyre_coupling=1.0))
    for name, l, d in (("tyre_coupling 1.0, load_transfer 0.35", log, dist), ("tyre_coupling 1.0 alone", other, other_dist)):
        print("loaded plant, %d ticks, %s: %.1f m of centre line, max |e_y| %.3f m, mean %.3f m, sideslip %.4f, top speed "
              "%.2f m/s, solved %d" % (tgt.TERMS_TICKS, name, d, np.abs(l[:, 0]).max(), np.abs(l[:, 0]).mean(), l[:, 1].max(),
                                       l[:, 3].max(), int(l[:, 4].sum())))
    assert np.all(log[:, 4] == 1.0), "ticks not solved: %s" % np.flatnonzero(log[:, 4] != 1.0)[:8]
    assert np.abs(log[:, 0]).max() < tgd.LOOP_CORRIDOR, "left the corridor: |e_y| %.2f m" % np.abs(log[:, 0]).max()
    assert log[:, 1].max() < tgd.LOOP_SLIP, "sideslip |vy| / vx %.4f" % log[:, 1].max()
