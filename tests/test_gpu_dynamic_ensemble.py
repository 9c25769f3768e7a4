"""Mode D's ensemble of vehicles on the MI355X: every candidate's cost, the argmin and the winner's record bit-identical
to the restatement (tests/dynamic_ensemble_spec.py) from every call form; an ensemble of one (or of copies of one
vehicle) is the single vehicle bit for bit; two candidates per lane; and a closed loop on a road with less grip than the
nominal vehicle's, where scoring under a grip ensemble keeps the car on the road and the nominal vehicle alone does not."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_ensemble_spec as es
import dynamic_spec as ds
import test_gpu_dynamic as tgd

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4096, 49), (3, 130, 2), (2, 257, 128)]
# problem kinds per shape (test_gpu_dynamic's mix): 0 plain with a NaN pedal, 1 standstill, 2 a yaw a turn beyond -pi,
# 3 a path 4 km from the origin
KINDS = {(1, 4096, 49): (0,), (3, 130, 2): (1, 2, 3), (2, 257, 128): (3, 1)}


def _vehicles():
    """The vehicles the ensembles draw from: the default, grips round it, and the reference's literal block, whose unit
    mismatch gives some candidates huge or non-finite costs under that vehicle only."""
    from acmpc_amd import DynamicBicycleParams
    base = DynamicBicycleParams.reference()
    return [base, base.with_grip(0.85), base.with_grip(1.1), DynamicBicycleParams.reference(literal=True),
            base.with_grip(0.7), base.with_grip(0.95), base.with_grip(1.2), base.with_grip(0.8)]


# K -> (vehicle indices, weights); K = 8 runs on one shape only
ENSEMBLES = {2: ((0, 1), None), 3: ((0, 3, 2), (1.0, 2.0, 0.5)), 8: (tuple(range(8)), None)}
CASES = [(shape, K) for shape in SHAPES for K in (2, 3)] + [((3, 130, 2), 8)]

_problem_cache = {}
_spec_cache = {}


def _problems(shape, seed=0):
    if shape not in _problem_cache:
        P, N, n = shape
        out = []
        for p, kind in enumerate(KINDS[shape]):
            dp = ds.make_dynamic_problem(orc, "monza", n + 1, N, seed + p, vx0=0.0 if kind == 1 else None,
                                         yaw_turns=-1 if kind == 2 else 0,
                                         origin=(3000.0, 2700.0) if kind == 3 else (0.0, 0.0))
            if kind == 0 and N > 10:
                dp["U"][5, n // 2, 1] = np.nan      # a NaN pedal ranks last
            out.append(dp)
        _problem_cache[shape] = out
    return _problem_cache[shape]


def _engine(dps, P, N, n, nn_window=None, **extra):
    from acmpc_amd import Engine
    kw = dict(dps[0]["kw"], max_problems=P, max_candidates=N, max_steps=n, nn_window=nn_window)
    kw.update(extra)
    eng = Engine(**kw)
    eng.set_paths(np.stack([d["table"] for d in dps]))
    return eng


def _per_vehicle(key, dp, coef, v, nn_window, U=None):
    """dynamic_spec's (cost, V, states) of one problem under one vehicle, cached: it depends on neither the reduce nor
    the layout."""
    if key not in _spec_cache:
        _spec_cache[key] = ds.spec_costs(orc, dp, coef, _vehicles()[v].coefficients(), nn_window=nn_window, U=U,
                                         return_states=True)
    return _spec_cache[key]


def _spec(shape, eng, dps, p, idx, weights, reduce, nn_window):
    per = [_per_vehicle((shape, nn_window, p, v), dps[p], eng.coefficients(p), v, nn_window) for v in idx]
    J, V = es.combine([r[0] for r in per], [r[1] for r in per], reduce, weights)
    return J, V, per[0][2]


def _set(eng, idx, weights, reduce):
    vs = _vehicles()
    eng.set_dynamics_ensemble([vs[i] for i in idx], weights=weights, reduce=reduce)


@pytest.mark.parametrize("nn_window", [None, (2, 5)])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("shape,K", CASES)
def test_costs_argmin_and_record_are_the_specification(shape, K, reduce, layout, nn_window):
    from acmpc_amd import _capi
    P, N, n = shape
    dps = _problems(shape)
    idx, weights = ENSEMBLES[K]
    eng = _engine(dps, P, N, n, nn_window)
    _set(eng, idx, weights, reduce)
    U_h = np.stack([d["U"] for d in dps])
    U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
    x0 = np.stack([d["x0"] for d in dps])
    out = eng.solve(x0, U_in, layout=layout)
    for p in range(P):
        J, V, X = _spec(shape, eng, dps, p, idx, weights, reduce, nn_window)
        tgd._same_bits(out["costs"][p], J)
        best = tgd._check_record(_capi.split_record(out["records"][p], n), U_h[p], J, V, X, n)
        assert out["best_idx"][p] == best
    if KINDS[shape][0] == 0:
        assert np.isnan(out["costs"][0][5])
    eng.close()


def _all_forms(eng, P, N, n, x0_h, U_h, layout, softmin=True):
    """What every call form returns on this handle: host solve, solve_device, two shards by index_offset with MIN-combined
    keys (one owner and one blank record), the softmin over the rollout's costs."""
    import torch
    from acmpc_amd import _capi
    U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
    out = {}
    host = eng.solve(x0_h, U_in, layout=layout)
    out["host_costs"], out["host_records"], out["host_best"] = host["costs"], host["records"], np.array(host["best_idx"])
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    x0 = torch.tensor(x0_h, device=dev)
    U = torch.tensor(U_in, device=dev)
    rf = _capi.record_floats(n)
    costs = torch.empty(P, N, device=dev)
    keys = torch.empty(P, dtype=torch.int64, device=dev)
    recs = torch.empty(P, rf, device=dev)
    eng.solve_device(x0.data_ptr(), U.data_ptr(), P, N, n, layout, costs.data_ptr(), keys.data_ptr(), recs.data_ptr(), s)
    half = N // 2
    parts = []
    for lo, hi in ((0, half), (half, N)):
        Us = U_h[:, lo:hi]
        Us = Us if layout == 0 else np.ascontiguousarray(Us.transpose(0, 2, 3, 1))
        parts.append((lo, hi, torch.tensor(Us, device=dev), torch.empty(P, hi - lo, device=dev),
                      torch.empty(P, dtype=torch.int64, device=dev)))
    for lo, hi, Us, cs, ks in parts:
        eng.rollout_device(x0.data_ptr(), Us.data_ptr(), P, hi - lo, n, layout, lo, cs.data_ptr(), ks.data_ptr(), s)
    torch.cuda.synchronize()
    combined = torch.minimum(parts[0][4], parts[1][4])
    shard_recs = []
    for lo, hi, Us, cs, ks in parts:
        r = torch.empty(P, rf, device=dev)
        eng.rollout_device(x0.data_ptr(), Us.data_ptr(), P, hi - lo, n, layout, lo, cs.data_ptr(), 0, s)
        eng.finalize_device(combined.data_ptr(), x0.data_ptr(), Us.data_ptr(), P, hi - lo, n, layout, lo, r.data_ptr(), s)
        shard_recs.append(r)
    torch.cuda.synchronize()
    out["dev_costs"], out["dev_records"] = costs.cpu().numpy(), recs.cpu().numpy()
    out["dev_best"] = np.array([_capi.key_index(int(k)) for k in keys.cpu().numpy()])
    out["shard_costs"] = np.concatenate([parts[0][3].cpu().numpy(), parts[1][3].cpu().numpy()], axis=1)
    out["shard_keys"] = combined.cpu().numpy()
    out["shard_records"] = [r.cpu().numpy() for r in shard_recs]
    if softmin and layout == 0:
        sc = torch.empty(P, N, device=dev)
        sk = torch.empty(P, dtype=torch.int64, device=dev)
        mean = torch.empty(P, n, 2, device=dev)
        wsum = torch.empty(P, dtype=torch.float64, device=dev)
        eng.rollout_device(x0.data_ptr(), U.data_ptr(), P, N, n, 0, 0, sc.data_ptr(), sk.data_ptr(), s)
        eng.softmin_device(sc.data_ptr(), sk.data_ptr(), U.data_ptr(), P, N, n, 0, mean.data_ptr(), wsum.data_ptr(), s)
        torch.cuda.synchronize()
        out["soft_costs"], out["soft_mean"], out["soft_wsum"] = sc.cpu().numpy(), mean.cpu().numpy(), wsum.cpu().numpy()
    return out


def _check_forms_agree(out, P):
    """Every call form gives the host solve's bits; of the two shard records, one is the owner's and one is blank."""
    tgd._same_bits(out["dev_costs"], out["host_costs"])
    tgd._same_bits(out["dev_records"], out["host_records"])
    assert list(out["dev_best"]) == list(out["host_best"])
    tgd._same_bits(out["shard_costs"], out["host_costs"])
    r0, r1 = out["shard_records"]
    for p in range(P):
        owner = r0[p] if r0[p][3] == 1.0 else r1[p]
        other = r1[p] if r0[p][3] == 1.0 else r0[p]
        assert other[3] == 0.0 and not np.any(np.delete(other, 2))
        assert owner[2] + other[2] == out["host_records"][p][2]
        tgd._same_bits(np.delete(owner, 2), np.delete(out["host_records"][p], 2))
    if "soft_costs" in out:
        tgd._same_bits(out["soft_costs"], out["host_costs"])


def _same_outputs(a, b):
    for key in a:
        if key == "shard_records":
            for x, y in zip(a[key], b[key]):
                tgd._same_bits(x, y)
        elif key in ("host_best", "dev_best", "shard_keys"):
            assert np.array_equal(a[key], b[key]), key
        elif key in ("soft_mean", "soft_wsum"):
            assert np.array_equal(np.asarray(a[key]).view(np.uint8), np.asarray(b[key]).view(np.uint8)), key
        else:
            tgd._same_bits(a[key], b[key])


def test_an_ensemble_of_one_is_the_single_vehicle():
    """set_dynamics_ensemble([v]) == set_dynamics(v) in every call form, and so are two copies of v under MEAN
    (omega = 0.5: fma(0.5, c, 0.5 c) = c) and four under MAX; set_dynamics after an ensemble restores the old bits."""
    from acmpc_amd import DynamicBicycleParams
    P, N, n = 3, 1536, 49
    dps = tgd._problems(P, N, n, seed=40)
    x0_h = np.stack([d["x0"] for d in dps])
    U_h = np.stack([d["U"] for d in dps])
    v = DynamicBicycleParams.reference()
    for layout in (0, 1):
        eng = _engine(dps, P, N, n, softmin_lambda=0.5)
        eng.set_dynamics(v)
        want = _all_forms(eng, P, N, n, x0_h, U_h, layout)
        for vehicles, reduce in (([v], "mean"), ([v], "max"), ([v, v], "mean"), ([v] * 4, "max")):
            eng.set_dynamics_ensemble(vehicles, reduce=reduce)
            _same_outputs(_all_forms(eng, P, N, n, x0_h, U_h, layout), want)
        eng.set_dynamics_ensemble([v, v.with_grip(0.8)], reduce="max")
        other = _all_forms(eng, P, N, n, x0_h, U_h, layout, softmin=False)
        assert not np.array_equal(other["host_costs"], want["host_costs"])
        eng.set_dynamics(v)
        _same_outputs(_all_forms(eng, P, N, n, x0_h, U_h, layout), want)
        eng.close()


def test_every_call_form_gives_the_same_bits_with_four_vehicles():
    """K = 4: host solve, solve_device, two shards by index_offset, and the softmin agree bit for bit, and the host solve
    is the specification; a refused ensemble leaves the handle's four vehicles in place."""
    from acmpc_amd import DynamicBicycleParams, EngineError
    from acmpc_amd import _capi
    P, N, n, window = 3, 1536, 49, (2, 5)
    dps = tgd._problems(P, N, n, seed=40)
    x0_h = np.stack([d["x0"] for d in dps])
    U_h = np.stack([d["U"] for d in dps])
    idx = (0, 1, 2, 4)
    eng = _engine(dps, P, N, n, window, softmin_lambda=0.5)
    _set(eng, idx, None, "mean")
    out = _all_forms(eng, P, N, n, x0_h, U_h, 0)
    _check_forms_agree(out, P)
    for p in range(P):
        J, V, X = _spec(("forms", N, n), eng, dps, p, idx, None, "mean", window)
        tgd._same_bits(out["host_costs"][p], J)
        tgd._check_record(_capi.split_record(out["host_records"][p], n), U_h[p], J, V, X, n)
        w = orc.softmin_weights(J, 0.5).astype(np.float64)
        mean = np.tensordot(w, U_h[p].astype(np.float64), axes=(0, 0)) / w.sum()
        np.testing.assert_allclose(out["soft_mean"][p], mean, rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(out["soft_wsum"][p], w.sum(), rtol=1e-5)
    step_major = _all_forms(eng, P, N, n, x0_h, U_h, 1, softmin=False)
    _check_forms_agree(step_major, P)
    tgd._same_bits(step_major["host_costs"], out["host_costs"])
    bad = DynamicBicycleParams.reference().coefficients()
    bad[ds.FIELDS.index("mass")] = -1.0
    with pytest.raises(EngineError):
        eng.set_dynamics_ensemble([DynamicBicycleParams.reference(), bad])
    again = eng.solve(x0_h, U_h)
    tgd._same_bits(again["costs"], out["host_costs"])
    tgd._same_bits(again["records"], out["host_records"])
    eng.close()


def test_optimize_equals_its_restatement_with_an_ensemble():
    """acmpc_optimize under a K = 4 MAX ensemble, 2 rounds of 1 024: the product's sampler draws round the previous
    winner, then the ensemble specification's argmin and recentre."""
    import torch
    from acmpc_amd import _capi
    P, N, n, rounds, sigma, shrink, seed, window = 2, 1024, 30, 2, (0.05, 0.3), 0.5, 1234, (2, 5)
    dps = tgd._problems(P, N, n, seed=90)
    idx, reduce = (0, 1, 4, 2), "max"
    eng = _engine(dps, P, N, n, window)
    _set(eng, idx, None, reduce)
    x0_h = np.stack([d["x0"] for d in dps])
    centre_h = np.stack([np.stack([np.zeros(n), np.full(n, 0.2)], axis=1) for _ in dps]).astype(np.float32)
    out = eng.optimize(x0_h, centre_h, None, N, rounds, sigma, shrink=shrink, seed=seed)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    vs = _vehicles()
    centre = centre_h.copy()
    scale = 1.0
    for r in range(rounds):
        d_centre = torch.tensor(centre, device=dev)
        d_U = torch.empty(P, n, 2, N, device=dev)
        eng.sample_device(d_centre.data_ptr(), 2 * n, 0, P, N, n, 1, 0, (sigma[0] * scale, sigma[1] * scale), seed, r,
                          d_U.data_ptr(), s)
        torch.cuda.synchronize()
        U_all = d_U.cpu().numpy().transpose(0, 3, 1, 2)
        want = []
        for p in range(P):
            J, V, X = es.spec_ensemble(orc, dps[p], eng.coefficients(p), [vs[i].coefficients() for i in idx],
                                       reduce=reduce, nn_window=window, U=U_all[p], return_states=True)
            best = orc.pick_best(J)[0]
            want.append((J, V, X))
            centre[p] = U_all[p][best]
        scale *= shrink
    for p in range(P):
        J, V, X = want[p]
        tgd._check_record(_capi.split_record(out["records"][p], n), U_all[p], J, V, X, n)
    eng.close()


def test_two_candidates_per_lane():
    """P N K = 2^20 (128 x 4 096, K = 2): the rollout takes two candidates per lane.  Every key agrees with its costs,
    and two problems are checked in full against the specification."""
    from acmpc_amd import _capi
    P, N, n, window, K = 128, 4096, 20, (2, 5), 2
    assert P * N * K >= 1 << 20
    base = tgd._problems(4, N, n, seed=7)
    rng = np.random.default_rng(17)
    dps = [base[p % 4] for p in range(P)]
    U_h = np.stack([base[p % 4]["U"] for p in range(P)])
    U_h[..., 0] += rng.standard_normal(U_h.shape[:-1], dtype=np.float32) * np.float32(0.01)
    U_h[..., 0] = np.clip(U_h[..., 0], ds.U_MIN[0], ds.U_MAX[0])
    x0_h = np.stack([d["x0"] for d in dps])
    idx, reduce = (0, 1), "max"
    eng = _engine(dps, P, N, n, window)
    _set(eng, idx, None, reduce)
    out = eng.solve(x0_h, np.ascontiguousarray(U_h.transpose(0, 2, 3, 1)), layout=1)
    for p in range(P):
        c = out["costs"][p]
        best = orc.pick_best(c)[0]
        assert out["best_idx"][p] == best
        tgd._same_bits(out["records"][p][0], c[best])
    vs = _vehicles()
    for p in (0, 3):
        J, V, X = es.spec_ensemble(orc, dps[p], eng.coefficients(p), [vs[i].coefficients() for i in idx],
                                   reduce=reduce, nn_window=window, U=U_h[p], return_states=True)
        tgd._same_bits(out["costs"][p], J)
        tgd._check_record(_capi.split_record(out["records"][p], n), U_h[p], J, V, X, n)
    eng.close()


# ---- closed loop on a road with less grip -------------------------------------------------------------------------
# test_gpu_dynamic's loop (same circuit, speed profile at ay 8 m/s^2, horizon, candidates, weights) with the plant
# reference().with_grip(LOOP_GRIP): the nominal solver (grip 1) plans for tyres it does not have; the ensemble solver
# scores every candidate under ENSEMBLE_GRIPS, which bracket the plant's, and ranks by their mean.  Measured on the
# MI355X (the loop is deterministic), max |e_y| / max sideslip |vy| / vx against the bars 3.78 m / 0.1:
#   nominal only                          44.26 m / 30.06  - spins off the road in the tightest corner (818 waypoints)
#   grip_ensemble (0.4, 0.6), mean         1.45 m / 0.074  - holds both, 1 344 waypoints (672 m)
# (a worst case over (0.4, 0.6, 1.0) does not hold this road: 24.2 m / 22.4 - DESIGN.md section 4.10)
LOOP_GRIP = 0.5
ENSEMBLE_GRIPS = (0.4, 0.6)
ENSEMBLE_REDUCE = "mean"


def run_grip_loop(config, plant):
    """test_gpu_dynamic.run_loop with a DynamicSamplingSolver for the nominal vehicle built from `config`: (max |e_y|,
    max sideslip, waypoints travelled), or infinities when a solve fails (run_loop asserts every status)."""
    from acmpc_amd import DynamicBicycleParams, DynamicSamplingSolver
    solver = DynamicSamplingSolver(config, DynamicBicycleParams.reference())
    try:
        log = tgd.run_loop(solver.solve, plant)
    except AssertionError:
        return float("inf"), float("inf"), 0
    finally:
        solver.close()
    ey, slip, dv, idx = log.T
    return float(np.abs(ey).max()), float(slip.max()), int((idx[-1] - idx[0]) % 11586)


def test_grip_ensemble_holds_a_road_with_less_grip():
    """The plant has half the nominal grip: scored under a grip ensemble that brackets it, the solver keeps the car inside
    the corridor without a slide; scored under the nominal vehicle alone, it does not.  No speed band: a robust
    controller slows below the profile."""
    from acmpc_amd import DynamicBicycleParams
    assert tgd.LOOP_AY == 8.0
    plant = DynamicBicycleParams.reference().with_grip(LOOP_GRIP)
    robust = dict(tgd.LOOP_CONFIG, grip_ensemble=ENSEMBLE_GRIPS, ensemble_reduce=ENSEMBLE_REDUCE)
    ey, slip, travelled = run_grip_loop(robust, plant)
    assert ey < tgd.LOOP_CORRIDOR, "ensemble left the corridor: |e_y| %.2f m" % ey
    assert slip < tgd.LOOP_SLIP, "ensemble sideslip %.4f" % slip
    assert travelled > 1000                                   # > 500 m, through the tightest corner
    ey_n, slip_n, _ = run_grip_loop(dict(tgd.LOOP_CONFIG), plant)
    assert ey_n >= tgd.LOOP_CORRIDOR or slip_n >= tgd.LOOP_SLIP, \
        "the nominal solver holds both bars too: |e_y| %.2f m, sideslip %.4f" % (ey_n, slip_n)
