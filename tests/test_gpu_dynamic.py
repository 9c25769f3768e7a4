"""Mode D on the MI355X: every candidate's cost, the argmin and the winner's record bit-identical to the float32
specification (tests/dynamic_spec.py), from every call form; the softmin over mode D costs; acmpc_optimize against its
restatement (the product's own sampler draws, then the specification's rollout, argmin and recentre)."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_spec as ds

pytestmark = pytest.mark.gpu

# (3, 130, 2) stands for a one-step horizon: acmpc_set_paths takes n >= 2 waypoints, and mode D rolls one step per waypoint
SHAPES = [(1, 4096, 49), (8, 1000, 20), (3, 130, 2), (2, 257, 128)]


def _problems(P, N, n, seed=0):
    """P problems on the same shape; problem p % 4: 0 plain, 1 starting at standstill, 2 a yaw a turn beyond -pi,
    3 a path 4 km from the origin."""
    out = []
    for p in range(P):
        v = p % 4
        out.append(ds.make_dynamic_problem(orc, "monza", n + 1, N, seed + p, vx0=0.0 if v == 1 else None,
                                           yaw_turns=-1 if v == 2 else 0,
                                           origin=(3000.0, 2700.0) if v == 3 else (0.0, 0.0)))
    return out


def _engine(dps, P, N, n, nn_window=None, **extra):
    from acmpc_amd import DynamicBicycleParams, Engine
    kw = dict(dps[0]["kw"], max_problems=P, max_candidates=N, max_steps=n, nn_window=nn_window)
    kw.update(extra)
    eng = Engine(**kw)
    eng.set_dynamics(DynamicBicycleParams.reference())
    eng.set_paths(np.stack([d["table"] for d in dps]))
    return eng


def _same_bits(got, want):
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def _spec(eng, dps, nn_window, p):
    from acmpc_amd import DynamicBicycleParams
    return ds.spec_costs(orc, dps[p], eng.coefficients(p), DynamicBicycleParams.reference().coefficients(),
                         nn_window=nn_window, return_states=True)


def _check_record(rec, U, cost, V, X, n):
    best = orc.pick_best(cost)[0]
    assert rec["owner"] == 1.0
    _same_bits(rec["cost"], cost[best])
    _same_bits(rec["violation"], V[best])
    assert rec["n_feasible"] == np.count_nonzero(V == 0)
    _same_bits(rec["u"], U[best])
    _same_bits(rec["x"], X[best])
    return best


@pytest.mark.parametrize("nn_window", [None, (2, 5)])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("P,N,n", SHAPES)
def test_costs_argmin_and_record_are_the_specification(P, N, n, layout, nn_window):
    from acmpc_amd import _capi
    dps = _problems(P, N, n)
    if N > 10:
        dps[0]["U"][5, n // 2, 1] = np.nan      # a NaN pedal ranks last
    eng = _engine(dps, P, N, n, nn_window)
    U_h = np.stack([d["U"] for d in dps])
    U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
    x0 = np.stack([d["x0"] for d in dps])
    out = eng.solve(x0, U_in, layout=layout)
    for p in range(P):
        cost, V, X = _spec(eng, dps, nn_window, p)
        _same_bits(out["costs"][p], cost)
        best = _check_record(_capi.split_record(out["records"][p], n), U_h[p], cost, V, X, n)
        assert out["best_idx"][p] == best
    if N > 10:
        assert np.isnan(out["costs"][0][5])
    eng.close()


@pytest.mark.parametrize("layout", [0, 1])
def test_every_call_form_gives_the_same_bits(layout):
    import torch
    from acmpc_amd import _capi
    P, N, n = 3, 1536, 49
    dps = _problems(P, N, n, seed=40)
    eng = _engine(dps, P, N, n)
    U_h = np.stack([d["U"] for d in dps])
    U_in = U_h if layout == 0 else np.ascontiguousarray(U_h.transpose(0, 2, 3, 1))
    x0_h = np.stack([d["x0"] for d in dps])
    host = eng.solve(x0_h, U_in, layout=layout)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    x0 = torch.tensor(x0_h, device=dev)
    U = torch.tensor(U_in, device=dev)
    rf = _capi.record_floats(n)
    costs = torch.empty(P, N, device=dev)
    keys = torch.empty(P, dtype=torch.int64, device=dev)
    recs = torch.empty(P, rf, device=dev)
    eng.solve_device(x0.data_ptr(), U.data_ptr(), P, N, n, layout, costs.data_ptr(), keys.data_ptr(), recs.data_ptr(), s)
    torch.cuda.synchronize()
    _same_bits(costs.cpu().numpy(), host["costs"])
    assert np.array_equal(recs.cpu().numpy().view(np.uint32), host["records"].view(np.uint32))
    assert [_capi.key_index(int(k)) for k in keys.cpu().numpy()] == list(host["best_idx"])
    # two shards by index_offset, keys MIN-combined as the all-reduce would leave them
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
    for lo, hi, Us, cs, ks in parts:   # each rank: its rollout (partials in the handle), then the finalize on the keys
        r = torch.empty(P, rf, device=dev)
        eng.rollout_device(x0.data_ptr(), Us.data_ptr(), P, hi - lo, n, layout, lo, cs.data_ptr(), 0, s)
        eng.finalize_device(combined.data_ptr(), x0.data_ptr(), Us.data_ptr(), P, hi - lo, n, layout, lo, r.data_ptr(), s)
        shard_recs.append(r)
    torch.cuda.synchronize()
    _same_bits(np.concatenate([parts[0][3].cpu().numpy(), parts[1][3].cpu().numpy()], axis=1), host["costs"])
    r0, r1 = (r.cpu().numpy() for r in shard_recs)
    for p in range(P):
        owner = r0[p] if r0[p][3] == 1.0 else r1[p]
        other = r1[p] if r0[p][3] == 1.0 else r0[p]
        assert other[3] == 0.0 and not np.any(np.delete(other, 2))
        assert owner[2] + other[2] == host["records"][p][2]
        assert np.array_equal(np.delete(owner, 2).view(np.uint32), np.delete(host["records"][p], 2).view(np.uint32))
    eng.close()


def test_softmin_over_mode_d_costs():
    import torch
    P, N, n = 2, 3000, 30
    dps = _problems(P, N, n, seed=70)
    eng = _engine(dps, P, N, n, softmin_lambda=0.5)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    U_h = np.stack([d["U"] for d in dps])
    U = torch.tensor(U_h, device=dev)
    x0 = torch.tensor(np.stack([d["x0"] for d in dps]), device=dev)
    costs = torch.empty(P, N, device=dev)
    keys = torch.empty(P, dtype=torch.int64, device=dev)
    mean = torch.empty(P, n, 2, device=dev)
    wsum = torch.empty(P, dtype=torch.float64, device=dev)
    eng.rollout_device(x0.data_ptr(), U.data_ptr(), P, N, n, 0, 0, costs.data_ptr(), keys.data_ptr(), s)
    eng.softmin_device(costs.data_ptr(), keys.data_ptr(), U.data_ptr(), P, N, n, 0, mean.data_ptr(), wsum.data_ptr(), s)
    torch.cuda.synchronize()
    for p in range(P):
        c = costs[p].cpu().numpy()
        _same_bits(c, _spec(eng, dps, None, p)[0])
        w = orc.softmin_weights(c, 0.5).astype(np.float64)
        want = np.tensordot(w, U_h[p].astype(np.float64), axes=(0, 0)) / w.sum()
        np.testing.assert_allclose(mean[p].cpu().numpy(), want, rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(wsum[p].item(), w.sum(), rtol=1e-5)
    eng.close()


def test_optimize_equals_its_restatement():
    """acmpc_optimize in mode D, 2 rounds of 1 024: round r's candidates are what acmpc_sample_device draws round the
    previous winner (the product's own sampler, read back), then the specification's rollout, argmin and recentre."""
    import torch
    from acmpc_amd import _capi
    P, N, n, rounds, sigma, shrink, seed = 2, 1024, 30, 2, (0.05, 0.3), 0.5, 1234
    dps = _problems(P, N, n, seed=90)
    eng = _engine(dps, P, N, n)
    x0_h = np.stack([d["x0"] for d in dps])
    centre_h = np.stack([np.stack([np.zeros(n), np.full(n, 0.2)], axis=1) for _ in dps]).astype(np.float32)
    out = eng.optimize(x0_h, centre_h, None, N, rounds, sigma, shrink=shrink, seed=seed)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
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
            cost, V, X = ds.spec_costs(orc, dps[p], eng.coefficients(p),
                                       _dyn_block(), U=U_all[p], return_states=True)
            best = orc.pick_best(cost)[0]
            want.append((cost, V, X, best))
            centre[p] = U_all[p][best]
        scale *= shrink
    for p in range(P):
        cost, V, X, best = want[p]
        rec = _capi.split_record(out["records"][p], n)
        _check_record(rec, U_all[p], cost, V, X, n)
    eng.close()


def _dyn_block():
    from acmpc_amd import DynamicBicycleParams
    return DynamicBicycleParams.reference().coefficients()


# ---- closed loop ---------------------------------------------------------------------------------------------------
# DynamicSamplingSolver drives the float64 mirror (the plant) for 400 ticks of 0.05 s round the synthetic Monza circuit
# of workloads.py, from 200 m before its tightest corner (radius 170 m), fed each tick the path window ahead of the car
LOOP_TICKS = 400
LOOP_DT = 0.05
LOOP_H = 50
LOOP_STRIDE = 4              # waypoints 2 m apart along the 0.5 m centreline: a 98 m window
LOOP_WIDTH = 9.5             # the circuit's road width
LOOP_AY = 8.0                # m/s^2 the speed profile allows (the default vehicle's tyres give ~11.4) ...
LOOP_V_MAX = 34.0            # ... capped at 34 m/s: 6.8 m/s^2 in the tightest corner
LOOP_CONFIG = dict(horizon=LOOP_H, n_candidates=2048, sampling_rounds=2, sampling_sigma=(0.02, 0.3), sampling_seed=11,
                   nn_window=(2, 5), rollout_dt=LOOP_DT, step_cost=(1.0, 20.0, 0.0), r_term=(1.0, 10.0),
                   final_cost=(1.0, 20.0, 0.0), margin=0.97, w_bound=1.0e4)
# what the loop must hold (the specification's restatement of this very loop - optimize == restatement bit for bit, the
# same float64 plant - gives max |e_y| 0.35 m, mean 0.03 m, sideslip 0.038, speed within 0.09 m/s of the profile, 676 m):
# |e_y| inside the corridor (width / 2 - margin) and on average near the centre line, sideslip |vy| / vx well short of a
# slide (0.1: a 6 degree slip angle), speed within a band of the profile once the start transient (2 s) is over
LOOP_CORRIDOR = LOOP_WIDTH / 2 - 0.97
LOOP_MEAN_EY = 0.25
LOOP_SLIP = 0.1
LOOP_SPEED_BAND = 0.5


def loop_track():
    from acmpc_amd import workloads
    centre = workloads.synthetic_track("monza")["centre"]
    tangent = np.gradient(centre, axis=0)
    heading = np.unwrap(np.arctan2(tangent[:, 1], tangent[:, 0]))
    kappa = np.gradient(heading) / 0.5
    v_profile = np.minimum(LOOP_V_MAX, np.sqrt(LOOP_AY / np.maximum(np.abs(kappa), 1e-9)))
    start = (int(np.argmax(np.abs(kappa))) - 400) % len(centre)
    return centre, v_profile, heading, start


def loop_path(centre, v_profile, pose):
    """The 7 x (H - 1) table of the path window ahead of the car (world frame), widths of the road, v = the profile."""
    i0 = int(np.argmin(((centre - pose[:2]) ** 2).sum(axis=1)))
    idx = (i0 + LOOP_STRIDE * np.arange(LOOP_H)) % len(centre)
    table = orc.construct_waypoints(np.column_stack([centre[idx], np.full(LOOP_H, LOOP_WIDTH)]))
    table[orc.ROW_V] = v_profile[idx[:-1]]
    return table, i0


def loop_frenet(centre, heading, pose):
    i = int(np.argmin(((centre - pose[:2]) ** 2).sum(axis=1)))
    d = pose[:2] - centre[i]
    return float(np.cos(heading[i]) * d[1] - np.sin(heading[i]) * d[0]), i


def run_loop(solve, plant):
    """Runs the loop with `solve(state, table) -> obj`; returns per tick (e_y, |vy| / vx, vx - v_ref, index)."""
    centre, v_profile, heading, start = loop_track()
    state = np.array([centre[start, 0], centre[start, 1], heading[start], v_profile[start] - 4.0, 0.0, 0.0])
    n = LOOP_H - 1
    log = []
    for _ in range(LOOP_TICKS):
        table, _ = loop_path(centre, v_profile, state)
        obj = solve(state, table)
        assert obj.info.status == "solved"
        u = obj.x[3 * (n + 1):].reshape(n, 2)
        state = plant.predict_next_state(state, u[0], LOOP_DT)[0]
        state[3] = max(state[3], 0.0)
        ey, i = loop_frenet(centre, heading, state)
        log.append((ey, abs(state[4]) / max(state[3], 1.0), state[3] - v_profile[i], i))
    return np.array(log)


def check_loop(log):
    ey, slip, dv, idx = log.T
    assert np.abs(ey).max() < LOOP_CORRIDOR, "left the corridor: |e_y| %.2f m" % np.abs(ey).max()
    assert np.abs(ey).mean() < LOOP_MEAN_EY, "does not hold the centre line: mean |e_y| %.2f m" % np.abs(ey).mean()
    assert slip.max() < LOOP_SLIP, "sideslip |vy| / vx %.4f" % slip.max()
    assert np.abs(dv[int(2.0 / LOOP_DT):]).max() < LOOP_SPEED_BAND, "speed off the profile by %.2f m/s" % np.abs(dv[40:]).max()
    assert (idx[-1] - idx[0]) % 11586 > 1000                 # > 500 m travelled, through the tightest corner


def test_dynamic_sampling_solver_closed_loop():
    """DynamicSamplingSolver's seam (obj.x = [x_0..x_n ; u_0..u_{n-1}], obj.info.status) in closed loop with the float64
    mirror as the plant: inside the corridor, no sideslip beyond LOOP_SLIP, the speed profile held within LOOP_SPEED_BAND."""
    from acmpc_amd import DynamicBicycleParams, DynamicSamplingSolver
    plant = DynamicBicycleParams.reference()
    solver = DynamicSamplingSolver(dict(LOOP_CONFIG), plant)
    n = LOOP_H - 1

    def solve(state, table):
        obj = solver.solve(state, table)
        assert obj.x.shape == (3 * (n + 1) + 2 * n,)
        u = obj.x[3 * (n + 1):].reshape(n, 2)
        assert np.all(np.abs(u[:, 0]) <= 0.3) and np.all(np.abs(u[:, 1]) <= 1.0)
        return obj

    check_loop(run_loop(solve, plant))
    solver.close()
