"""Mode D's settings and call forms drawn together, on the MI355X: tests/test_gpu_fuzz_dynamic.py's random shapes with the
integration, the rate and slip terms (each weight and each limit its own switch), the previous control, the objective, the
coupling (one-sided ratios among them) and the load transfer drawn beside them by tests/dynamic_fuzz_cases.py, per kernel
family of the dispatch of csrc/acmpc_dynamic.hip (fine, terms, objective, coupled, loaded) and per call form - the control
matrix (Engine.solve), or the fused sampled rollout with the record re-drawn from the index.  The handle is set through the
public setters in a drawn order; the float32 restatement takes the same settings as one Settings value;
every per-candidate cost, the argmin (the key), the feasible count and the winner's record must have the restatement's bits,
and the record's cost the rollout's own.

In front of the random cases: the longest horizon (H = 513) for the terms / objective, coupled and loaded families, both
layouts; two candidates per lane (test_gpu_dynamic_packed's launch) for drawn partial parts; and acmpc_score_grips under
drawn (ratio, load, integration, L, K).  tests/test_dynamic_fuzz_cases.py holds, on the CPU, that the committed seed covers
what it should and that every part that is on changes something.

ACMPC_FUZZ_CASES scales the draw as it does test_gpu_fuzz_dynamic's: of its default 40, 6 cases per family and form run here
(ACMPC_FUZZ_CASES * 6 // 40, one at least).  The NumPy restatement is a test's wall time: about a second a case."""
import os

import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_fuzz_cases as fz
import grip_spec as gs
from dynamic_spec import Settings

pytestmark = pytest.mark.gpu

T = np.float32


def _count():
    return max(1, int(os.environ.get("ACMPC_FUZZ_CASES", "40")) * fz.DEFAULT_CASES // 40)


def same_bits(got, want, message=""):
    """Bit-identical float32, a NaN for a NaN."""
    got, want = np.asarray(got, dtype=T), np.asarray(want, dtype=T)
    assert got.shape == want.shape, message
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), message
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), message


def check_solve(out, U, want, n, label):
    """Engine.solve's dict against the restatement's (cost, V, states) per problem: test_gpu_fuzz_dynamic._solve_and_check and
    test_gpu_dynamic._check_record."""
    from acmpc_amd import _capi
    for p, (cost, V, X) in enumerate(want):
        where = "%s, problem %d" % (label, p)
        same_bits(out["costs"][p], cost, where + ": costs")
        best = orc.pick_best(cost)[0]
        assert out["best_idx"][p] == best, where
        assert out["n_feasible"][p] == np.count_nonzero(V == 0), where
        rec = _capi.split_record(out["records"][p], n)
        assert rec["owner"] == 1.0 and rec["n_feasible"] == np.count_nonzero(V == 0), where
        same_bits(rec["cost"], cost[best], where + ": the record's cost")
        same_bits(rec["cost"], out["costs"][p][best], where + ": the record's cost against the rollout's")
        same_bits(rec["violation"], V[best], where + ": the record's violation")
        same_bits(rec["u"], U[p][best], where + ": the record's controls")
        same_bits(rec["x"], X[best], where + ": the record's states")


def check_sampled(costs, keys, records, want, n, label):
    """The fused rollout's costs and keys and the re-drawn records against dynamic_sampled_spec.rollout_sampled's dicts."""
    from acmpc_amd import _capi
    for p, w in enumerate(want):
        where = "%s, problem %d" % (label, p)
        same_bits(costs[p], w["cost"], where + ": costs")
        assert int(keys[p]) == w["key"], where + ": key"
        r, best = _capi.split_record(records[p], n), w["best"]
        assert r["owner"] == 1.0 and r["n_feasible"] == w["n_feasible"], where
        for name, value in (("cost", w["cost"][best]), ("violation", w["violation"][best]), ("u", w["U"][best]),
                            ("x", w["x"][best])):
            same_bits(r[name], value, "%s: the record's %s" % (where, name))


def run_matrix(c, layouts=None):
    from acmpc_amd import Engine
    n = c["H"] - 1
    dps = fz.problems(c, orc)
    U = np.stack([d["U"] for d in dps])
    x0 = np.stack([d["x0"] for d in dps])
    want = None
    for layout in (layouts or (c["layout"],)):
        label = fz.label(dict(c, layout=layout))
        eng = Engine(**dict(dps[0]["kw"], max_problems=c["P"], max_candidates=c["N"], max_steps=n, nn_window=c["window"]))
        try:
            fz.apply(eng, c)
            eng.set_paths(np.stack([d["table"] for d in dps]))
            if want is None:
                want = fz.specification(c, orc, dps, [eng.coefficients(p) for p in range(c["P"])])
            data = U if layout == 0 else np.ascontiguousarray(U.transpose(0, 2, 3, 1))
            check_solve(eng.solve(x0, data, layout=layout), U, want, n, label)
        finally:
            eng.close()


def run_sampled(c):
    import test_gpu_dynamic_sampled as tsm
    n, N = c["H"] - 1, c["N"]
    label = fz.label(c)
    rig = tsm.Rig(c["P"], N, n, K=1, window=c["window"], seed=c["seed"], with_ref=c["with_ref"], track=c["track"],
                  kinds=c["kinds"])
    try:
        fz.apply(rig.eng, c)
        centre, ref = fz.centres(c, orc, rig.dps)
        assert np.array_equal(centre, rig.centre_h), label      # (the generator's centres are the rig's)
        rig.centre_h, rig.ref_h = centre, ref
        rig.upload()
        costs, keys = rig.fused(N, c["index_offset"], c["sigma"], c["sample_seed"], c["round"])
        records = rig.finalize_sampled(None, N, c["sigma"], c["sample_seed"], c["round"])
        want = fz.specification(c, orc, rig.dps, [rig.eng.coefficients(p) for p in range(c["P"])], centre, ref)
        check_sampled(costs.cpu().numpy(), keys.cpu().numpy(), records, want, n, label)
    finally:
        rig.close()


@pytest.mark.parametrize("family", fz.FAMILIES)
def test_control_matrix_against_the_composed_specification(family):
    for c in fz.cases(family, "matrix", _count()):
        run_matrix(c)


@pytest.mark.parametrize("family", fz.FAMILIES)
def test_sampled_rollout_and_record_against_the_composed_specification(family):
    for c in fz.cases(family, "sampled", _count()):
        run_sampled(c)


@pytest.mark.parametrize("index", range(len(fz.LONGEST)), ids=lambda i: "%s-%d" % (fz.LONGEST[i]["family"], i))
def test_the_longest_horizon(index):
    """H = 513, kDynamicMaxSteps steps: one restatement, both layouts."""
    run_matrix(fz.LONGEST[index], layouts=(0, 1))


# ---- two candidates per lane ------------------------------------------------------------------------------------------------
PACKED = fz.packed_cases()


@pytest.mark.parametrize("index", range(len(PACKED)), ids=lambda i: "%s-K%d" % (PACKED[i]["family"], PACKED[i]["K"]))
def test_packed_rollout(index):
    """test_gpu_dynamic_load_transfer.test_packed_rollout with a drawn case's settings: N = 4099, n = 4, P N K >= 2^20.  In
    full against the one-candidate-per-lane kernels - two shards of candidates by index_offset, each below 2^20 - and against
    the restatement on test_gpu_dynamic_packed's subset."""
    import torch
    from acmpc_amd import _capi
    import dynamic_ensemble_spec as es
    import dynamic_spec as ds
    import test_gpu_dynamic as tgd
    import test_gpu_dynamic_ensemble as tge
    import test_gpu_dynamic_load_transfer as tgl
    import test_gpu_dynamic_packed as tpk
    import test_gpu_dynamic_terms as tgt
    c = PACKED[index]
    K, layout, window = c["K"], c["layout"], c["window"]
    N, n = 4099, 4
    P = tpk._problems_for(N, K)
    half = (N + 1) // 2
    assert P * N * K >= tpk.PACKED and P * half * K < tpk.PACKED
    label = "packed %r P %d" % (c, P)
    base, U, x0, tables = tpk._make(P, N, n, seed=2450 + index)
    x0[2::4, 3] = 4.0
    U[:, 20, :, 1], U[:, 21, :, 1], U[:, 23, :, 1] = -1.0, 1.0, 0.0
    planted = tpk._plant(U, N, n)
    by_kind = tgt._previous(4, 46 + index)
    u_prev = by_kind[np.arange(P) % 4] if c["previous"] != "none" else None
    vehicles = [tgl._vehicle()] if K == 1 else tgl._grip_vehicles()
    setting, integration = (c["objective"], c["terms"]), (c["M"], c["blend"])
    eng = tge._engine([base[p % 4] for p in range(P)], P, N, n, window)
    try:
        eng.set_dynamics_integration(*integration)
        tgl._set(eng, c["ratio"], c["load"], setting, u_prev)
        if K == 1:
            eng.set_dynamics(vehicles[0])
        else:
            eng.set_dynamics_ensemble(vehicles, reduce="mean")
        whole = eng.solve(x0, tpk._as_layout(U, layout), layout=layout)
        coefs = [eng.coefficients(q) for q in range(4)]
        blocks = [v.coefficients() for v in vehicles]

        def spec(q, U_sub, states):
            dp = dict(base[q], x0=x0[q])
            prev = None if u_prev is None else by_kind[q]
            if K == 1:
                return ds.spec_costs(orc, dp, coefs[q], blocks[0], nn_window=window, U=U_sub, return_states=states,
                                     settings=Settings(*integration, **setting[0], **setting[1], coupling=c["ratio"],
                                                       load_transfer=c["load"]), u_prev=prev)
            return es.spec_ensemble(orc, dp, coefs[q], blocks, reduce="mean", nn_window=window, U=U_sub, return_states=states,
                                    settings=Settings(*integration, **setting[0], **setting[1], coupling=c["ratio"],
                                                      load_transfer=c["load"]), u_prev=prev)

        tpk._check_against_spec(whole, base, coefs, U, N, n, tpk.GROUP_ONE if K == 1 else tpk.GROUP_ENSEMBLE, planted, spec,
                                77 + index, label)
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream().cuda_stream
        rf = _capi.record_floats(n)
        d_x0 = torch.tensor(x0, device=dev)
        shards = []
        for lo, hi in ((0, half), (half, N)):
            d_U = torch.tensor(tpk._as_layout(U[:, lo:hi], layout), device=dev)
            shards.append((lo, hi - lo, d_U, torch.empty(P, hi - lo, device=dev), torch.empty(P, dtype=torch.int64, device=dev)))
        for lo, count, d_U, cs, ks in shards:
            eng.rollout_device(d_x0.data_ptr(), d_U.data_ptr(), P, count, n, layout, lo, cs.data_ptr(), ks.data_ptr(), s)
        torch.cuda.synchronize()
        tgd._same_bits(np.concatenate([shards[0][3].cpu().numpy(), shards[1][3].cpu().numpy()], axis=1), whole["costs"])
        combined = torch.minimum(shards[0][4], shards[1][4])
        assert [_capi.key_index(int(k)) for k in combined.cpu().numpy()] == list(whole["best_idx"]), label
        records = []
        for lo, count, d_U, cs, ks in shards:
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


# ---- acmpc_score_grips ------------------------------------------------------------------------------------------------------
IDENTIFICATION = fz.identification_cases()


@pytest.mark.parametrize("index", range(len(IDENTIFICATION)))
def test_score_grips_against_the_specification(index):
    """acmpc_score_grips on test_gpu_dynamic_load_transfer's braking log under a drawn (ratio, load, integration, L, K)."""
    from acmpc_amd.grip_estimator import grip_scales
    import test_gpu_dynamic_load_transfer as tgl
    import test_gpu_grip_identification as tgi
    c = IDENTIFICATION[index]
    states, controls = tgl._braking_log(40)
    scales = grip_scales(tgl.GRID, "tied" if c["K"] == 25 else "split")
    eng = tgi._engine(c["integration"])
    try:
        eng.set_dynamics_load_transfer(c["load"])
        eng.set_dynamics_coupling(c["ratio"])
        errors, best = eng.score_grips(states, controls, 0.05, scales, segment=c["L"])
        want, want_best = gs.score(tgl._vehicle().coefficients(), states, controls, 0.05, scales, segment=c["L"],
                                   settings=Settings(substeps=c["integration"][0], low_speed_blend=c["integration"][1],
                                                     coupling=c["ratio"], load_transfer=c["load"]))
        same_bits(errors, want, repr(c))
        assert best == want_best and np.isfinite(want).all(), c
    finally:
        eng.close()
