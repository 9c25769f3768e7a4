"""Every launch shape of the rollouts over a control matrix, run on the device at its thresholds (the literals of
tests/test_rollout_shapes.py, one case either side of each).  Every case first asserts the form it is about through
`Engine.describe_rollout` - which answers from the functions the launches ask - and then compares ALL per-candidate costs, the
argmin, the feasible count and the winner's record bit for bit with c_oracle, the float32 restatement in C (tied to the NumPy
oracle and the reference's vectors by tests/test_oracle_c_vs_numpy.py and tests/test_oracle_golden.py).  No tolerance anywhere.

Horizons are short (2 ... 12 steps) wherever the rule under test does not look at the horizon: a 1 M-candidate launch is then
a 16 MB matrix and a tenth of a second of c_oracle."""
import functools
import os

import numpy as np
import pytest

import acmpc_oracle as orc
import c_oracle
from test_support import engine_kwargs, make_problem

pytestmark = pytest.mark.gpu

CM, SM = 0, 1
SIGMA = (2.0, 0.01)


@functools.lru_cache(maxsize=None)
def _problem(track, H, seed):
    return make_problem(orc, track, H, 4, seed=seed)


def _weights(prob, window):
    cfg = prob["cfg"]
    return c_oracle.make_weights(cfg["step_cost"], cfg["r_term"], cfg["final_cost"], prob["u_lo"], prob["u_hi"], 1.0e6,
                                 nn_window=window)


def _reference(mode, x0, coef, U, layout, w):
    """c_oracle over U [P,n,2,N] (step-major) or [P,N,n,2]: costs [P,N], violations [P,N], argmin [P], the winners' states."""
    P = U.shape[0]
    if mode == 0 and layout == SM:
        cost, viol = c_oracle.rollout_spatial_batch(x0, coef, U, w)
    else:
        both = [c_oracle.rollout(mode, x0[p], coef[p], U[p], layout, w) for p in range(P)]
        cost, viol = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    best = np.array([c_oracle.argmin(cost[p]) for p in range(P)])
    u = np.stack([U[p, :, :, best[p]] if layout == SM else U[p, best[p]] for p in range(P)])          # [P,n,2]
    states = np.stack([c_oracle.rollout(mode, x0[p], coef[p], u[p][None], CM, w, return_states=True)[2][0] for p in range(P)])
    return dict(cost=cost, viol=viol, best=best, u=u, x=states)


def _moved(ref, moves):
    """The reference of a matrix with candidates a and b of problem p exchanged, for (p, a, b) in moves."""
    cost, viol = ref["cost"].copy(), ref["viol"].copy()
    for p, a, b in moves:
        cost[p, [a, b]] = cost[p, [b, a]]
        viol[p, [a, b]] = viol[p, [b, a]]
    best = np.array([c_oracle.argmin(cost[p]) for p in range(cost.shape[0])])
    return dict(cost=cost, viol=viol, best=best, u=ref["u"], x=ref["x"])


def _verify(label, ref, n, costs=None, keys=None, rec=None, best_idx=None):
    from acmpc_amd import _capi
    P = ref["cost"].shape[0]
    if costs is not None:
        np.testing.assert_array_equal(costs, ref["cost"], err_msg=label + ": per-candidate costs")
    for p in range(P):
        best = int(ref["best"][p])
        want_cost = ref["cost"][p, best]
        if keys is not None:
            assert _capi.key_index(int(keys[p])) == best, "%s: argmin of problem %d" % (label, p)
        if best_idx is not None:
            assert int(best_idx[p]) == best, "%s: argmin of problem %d" % (label, p)
        if rec is not None:
            out = _capi.split_record(rec[p], n)
            assert int(out["n_feasible"]) == int(np.count_nonzero(ref["viol"][p] == 0)), "%s: n_feasible of problem %d" % (label, p)
            np.testing.assert_array_equal(out["cost"], want_cost, err_msg="%s: winner's cost, problem %d" % (label, p))
            np.testing.assert_array_equal(out["violation"], ref["viol"][p, best], err_msg="%s: winner's violation, problem %d" % (label, p))
            if np.isfinite(want_cost):
                np.testing.assert_array_equal(out["u"], ref["u"][p], err_msg="%s: winner's controls, problem %d" % (label, p))
                np.testing.assert_array_equal(out["x"], ref["x"][p], err_msg="%s: winner's states, problem %d" % (label, p))


def _expect_form(eng, P, N, n, layout, kernel, block, cpt, pack, **flags):
    d = eng.describe_rollout(P, N, n, layout)
    got = (d["kernel"], d["block"], d["cpt"], d["pack"])
    assert got == (kernel, block, cpt, pack), "form of %d x %d x %d, layout %d: %s" % (P, N, n, layout, d)
    assert d["workgroups"] == (N + block * cpt - 1) // (block * cpt), d
    for name, value in flags.items():
        assert d[name] == value, "%s of %d x %d x %d: %s" % (name, P, N, n, d)
    return d


class _Device:
    """One handle and its device buffers for step-major launches of (P, up to N_max, n)."""

    def __init__(self, mode, window, track, H, P, N_max, seed=900):
        import torch
        from acmpc_amd import Engine, _capi
        self.torch, self.capi = torch, _capi
        self.mode, self.window, self.P, self.n = mode, window, P, H - 1
        self.problems = [_problem(track, H, seed + p % 7) for p in range(P)]
        self.eng = Engine(**engine_kwargs(self.problems[0], mode, P, N_max, self.n, nn_window=window))
        self.eng.set_paths(np.stack([p["table"] for p in self.problems]))
        self.eng.set_option("ACMPC_NO_SOLO", 1)          # (the one-launch solve takes no launch shape)
        self.w = _weights(self.problems[0], window)
        self.x0_host = np.stack([p["x0"] if mode == 0 else p["pose0"] for p in self.problems])
        self.coef = np.stack([self.eng.coefficients(p) for p in range(P)])
        self.dev = torch.device("cuda", 0)
        self.s = torch.cuda.current_stream().cuda_stream
        self.x0 = torch.tensor(self.x0_host, device=self.dev)
        u_ref = np.stack([np.stack([p["table"][orc.ROW_V], p["table"][orc.ROW_KAPPA]], axis=1) for p in self.problems])
        self.centre = torch.tensor((u_ref + np.array([-0.4, 0.001])).astype(np.float32), device=self.dev).contiguous()
        self.R = _capi.record_floats(self.n)

    def close(self):
        self.eng.close()

    def matrix(self, N, seed, rnd):
        """What acmpc_sample_device draws round the centre, then NaN in one control of candidates 4k + 1 and inf in one of
        4k + 2 - in the first lane and in the last - so that those lanes hold finite and non-finite candidates side by side."""
        torch, n, P = self.torch, self.n, self.P
        U = torch.empty(P, n, 2, N, device=self.dev)
        self.eng.sample_device(self.centre.data_ptr(), 2 * n, 0, P, N, n, SM, 0, SIGMA, seed, rnd, U.data_ptr(), self.s)
        for k in sorted({0, (N - 1) // 4}):
            if 4 * k + 1 < N:
                U[:, n // 2, 0, 4 * k + 1] = float("nan")
            if 4 * k + 2 < N:
                U[:, 0, 1, 4 * k + 2] = float("inf")
        torch.cuda.synchronize()
        return U

    def reference(self, U):
        return _reference(self.mode, self.x0_host, self.coef, U.cpu().numpy(), SM, self.w)

    def outputs(self, N):
        torch = self.torch
        return (torch.full((self.P, N), -7.0, device=self.dev), torch.zeros(self.P, dtype=torch.int64, device=self.dev),
                torch.full((self.P, self.R), -7.0, device=self.dev))

    def host(self, *tensors):
        self.torch.cuda.synchronize()
        return [t.cpu().numpy() for t in tensors]

    # ---- the paths that take a launch shape ----
    def rollout_then_finalize(self, label, U, ref, N, with_keys):
        eng, P, n, s = self.eng, self.P, self.n, self.s
        costs, keys, rec = self.outputs(N)
        k = keys.data_ptr() if with_keys else 0
        eng.rollout_device(self.x0.data_ptr(), U.data_ptr(), P, N, n, SM, 0, costs.data_ptr(), k, s)
        eng.finalize_device(k, self.x0.data_ptr(), U.data_ptr(), P, N, n, SM, 0, rec.data_ptr(), s)
        costs, keys, rec = self.host(costs, keys, rec)
        _verify(label + ": rollout_device + finalize_device" + (" (keys)" if with_keys else " (partial keys)"), ref, n, costs,
                keys if with_keys else None, rec)

    def solve(self, label, U, ref, N, sampled, seed, rnd):
        eng, P, n, s = self.eng, self.P, self.n, self.s
        costs, keys, rec = self.outputs(N)
        if sampled:
            eng.solve_sampled_device(self.x0.data_ptr(), U.data_ptr(), self.centre.data_ptr(), 2 * n, 0, P, N, n, SM, SIGMA, seed,
                                     rnd, costs.data_ptr(), keys.data_ptr(), rec.data_ptr(), s)
        else:
            eng.solve_device(self.x0.data_ptr(), U.data_ptr(), P, N, n, SM, costs.data_ptr(), keys.data_ptr(), rec.data_ptr(), s)
        costs, keys, rec = self.host(costs, keys, rec)
        _verify(label + (": solve_sampled_device" if sampled else ": solve_device"), ref, n, costs, keys, rec)

    def finalize_sampled_from_keys(self, label, U, ref, N, seed, rnd, with_keys):
        """The multi-rank step's calls: the rollout's keys (or, on one GPU, the partial keys it left in the handle: as many
        per problem as the finalize expects of this shape), then the records re-drawn from the keys alone."""
        eng, P, n, s = self.eng, self.P, self.n, self.s
        costs, keys, rec = self.outputs(N)
        k = keys.data_ptr() if with_keys else 0
        eng.rollout_device(self.x0.data_ptr(), U.data_ptr(), P, N, n, SM, 0, costs.data_ptr(), k, s)
        eng.finalize_sampled_device(k, self.x0.data_ptr(), self.centre.data_ptr(), 2 * n, 0, P, N, n, SIGMA, seed, rnd,
                                    rec.data_ptr(), s)
        costs, keys, rec = self.host(costs, keys, rec)
        _verify(label + ": finalize_sampled_device" + (" (keys)" if with_keys else " (partial keys)"), ref, n, costs,
                keys if with_keys else None, rec)

    def stream(self, label, batches, N, sampled):
        """Three batches through acmpc_solve_stream_device and the flush: batches = [(U, ref, seed, round)]."""
        eng, P, n, s = self.eng, self.P, self.n, self.s
        outs = [self.outputs(N) for _ in batches]
        for (U, _, seed, rnd), (costs, keys, rec) in zip(batches, outs):
            eng.solve_stream_device(self.x0.data_ptr(), U.data_ptr(), self.centre.data_ptr() if sampled else 0, 2 * n, 0, P, N, n,
                                    SM, SIGMA, seed, rnd, costs.data_ptr(), keys.data_ptr(), rec.data_ptr(), s)
        eng.solve_stream_flush(s)
        for index, ((_, ref, _, _), out) in enumerate(zip(batches, outs)):
            costs, keys, rec = self.host(*out)
            _verify("%s: batch %d of a %s stream" % (label, index, "sampled" if sampled else "matrix"), ref, n, costs, keys, rec)

    def every_path(self, label, N, cpt, seed=4321):
        """Three matrices of this size through every call that takes a launch shape.  The calls that re-draw the winner from
        its index run on the matrices as sampled (+ the non-finite candidates, which never win); the calls that read the
        winner from the matrix run on copies in which every problem's winner has changed places with the LAST candidate of
        its lane, so that with several candidates per lane the record must be that of candidate j = cpt - 1."""
        batches, moved = [], []
        for k in range(3):
            U = self.matrix(N, seed + 13 * k, k)
            ref = self.reference(U)
            batches.append((U, ref, seed + 13 * k, k))
            moves = [(p, int(b), int(b) - int(b) % cpt + cpt - 1) for p, b in enumerate(ref["best"])]
            U2 = U.clone()
            for p, a, b in moves:
                U2[p, :, :, [a, b]] = U[p, :, :, [b, a]]
            ref2 = _moved(ref, moves)
            moved.append((U2, ref2, seed + 13 * k, k))
        mode_s_256 = self.mode == 0 and self.eng.describe_rollout(self.P, N, self.n, SM)["tailed_fits"]
        U, ref, sd, rnd = batches[0]
        U2, ref2, _, _ = moved[0]
        for with_keys in (True, False):
            self.rollout_then_finalize(label, U2, ref2, N, with_keys)
            self.finalize_sampled_from_keys(label, U, ref, N, sd, rnd, with_keys)
        self.solve(label, U2, ref2, N, False, sd, rnd)
        self.solve(label, U, ref, N, True, sd, rnd)
        if mode_s_256:   # rollout + finalize in one launch (rollout_tailed_kernel)
            self.eng.set_option("ACMPC_TAILED_ROLLOUT", 1)
            self.solve(label + ", tailed", U2, ref2, N, False, sd, rnd)
            self.solve(label + ", tailed", U, ref, N, True, sd, rnd)
            self.eng.set_option("ACMPC_TAILED_ROLLOUT", None)
        for chained in (True, False):   # batch k's finalize inside batch k + 1's launch (rollout_chained_kernel), or not
            self.eng.set_option("ACMPC_NO_CHAINED_STREAM", None if chained else 1)
            tag = label + (", chained" if chained else ", not chained")
            self.stream(tag, moved, N, False)
            self.stream(tag, batches, N, True)
        self.eng.set_option("ACMPC_NO_CHAINED_STREAM", None)


# ---------------------------------------------------------------------------------------------------------------------------
# a. the default rule, both sides of each threshold
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,N,block,cpt", [(256, 4096, 256, 4),     # 1 048 576 candidates, N % 4 == 0: rollout_kernel<0,1,4,256,2>,
                                                                    # and the tailed and chained kernels of that width
                                           (255, 4096, 256, 1),     # 4 096 short of it
                                           (256, 4098, 256, 1),     # past 1 M with N % 4 == 2
                                           (33, 4096, 256, 1),      # 135 168 candidates: 256-thread workgroups
                                           (32, 4096, 64, 1)])      # 131 072: 64-thread workgroups
def test_mode_s_step_major_by_the_default_rule(P, N, block, cpt):
    dev = _Device(0, None, "monza", 3, P, N)
    wide = block == 256
    _expect_form(dev.eng, P, N, dev.n, SM, "step", block, cpt, 2 if cpt > 1 else 1, tailed_fits=wide, chained_fits=wide, solo=False)
    dev.every_path("mode S %d x %d" % (P, N), N, cpt)
    dev.close()


@pytest.mark.parametrize("window", [None, (2, 5), (1, 2)])
@pytest.mark.parametrize("P,N,block,cpt", [(33, 4096, 256, 2),      # N even: launch_rollout_t<1,1,2,256,1,8>
                                           (33, 4095, 256, 1),      # N odd: launch_rollout_t<1,1,1,256,1>; a ragged last workgroup
                                           (32, 4096, 64, 1)])
def test_mode_t_step_major_by_the_default_rule(P, N, block, cpt, window):
    dev = _Device(1, window, "silverstone", 13, P, N)
    _expect_form(dev.eng, P, N, dev.n, SM, "step", block, cpt, 1, tailed_fits=False, chained_fits=False, solo=False)
    dev.every_path("mode T %s %d x %d" % (window, P, N), N, cpt)
    dev.close()


def _host_matrix(problems, N, n, seed):
    """U [P,N,n,2]: noise round each problem's reference controls with a per-candidate spread, clipped into the input box;
    NaN and inf in candidates 5 and 6 of problem 0 and in the last two of the last problem."""
    rng = np.random.default_rng(seed)
    P = len(problems)
    u_ref = np.stack([np.stack([p["table"][orc.ROW_V], p["table"][orc.ROW_KAPPA]], axis=1) for p in problems]).astype(np.float32)
    U = u_ref[:, None] + rng.standard_normal((P, N, n, 2), dtype=np.float32) * np.array(SIGMA, dtype=np.float32) * \
        rng.uniform(0.02, 1.0, (P, N, 1, 1)).astype(np.float32)
    np.clip(U, problems[0]["u_lo"].astype(np.float32), problems[0]["u_hi"].astype(np.float32), out=U)
    if N > 8:
        U[0, 5, n // 2, 0] = np.nan
        U[0, 6, 0, 1] = np.inf
        U[P - 1, N - 2, n - 1, 1] = np.nan
        U[P - 1, N - 1, n // 2, 0] = np.inf
    return U


def _host_solve_against_the_oracle(label, eng, mode, window, problems, N, n, layout, seed=5):
    P = len(problems)
    U = _host_matrix(problems, N, n, seed)
    x0 = np.stack([p["x0"] if mode == 0 else p["pose0"] for p in problems])
    coef = np.stack([eng.coefficients(p) for p in range(P)])
    out = eng.solve(x0, U if layout == CM else np.ascontiguousarray(U.transpose(0, 2, 3, 1)), layout=layout)
    ref = _reference(mode, x0, coef, U, CM, _weights(problems[0], window))
    _verify(label, ref, n, out["costs"], None, out["records"], out["best_idx"])


@pytest.mark.parametrize("mode,H,P,N,kernel", [(0, 129, 2, 65, "tile"),     # 128 steps: 64 KiB of LDS, the tile's last horizon
                                               (0, 130, 2, 65, "step"),     # 129: rollout_kernel on the candidate-major matrix
                                               (0, 129, 3, 1000, "tile"),
                                               (0, 130, 3, 1000, "step"),
                                               (1, 114, 2, 65, "tile"),     # mode T, 113 steps: tile + waypoint and key tables;
                                                                            # N n odd: problem 1's span starts on 8 bytes only
                                               (1, 115, 2, 65, "step"),
                                               (1, 114, 3, 1000, "tile"),
                                               (1, 115, 3, 1000, "step")])
def test_the_candidate_major_tile_at_its_last_horizon_and_the_step_kernel_past_it(mode, H, P, N, kernel):
    from acmpc_amd import Engine
    n = H - 1
    problems = [_problem("nordschleife", H, 40 + p) for p in range(P)]
    for window in ((None,) if mode == 0 else (None, (2, 5))):
        eng = Engine(**engine_kwargs(problems[0], mode, P, N, n, nn_window=window))
        eng.set_paths(np.stack([p["table"] for p in problems]))
        eng.set_option("ACMPC_NO_SOLO", 1)
        _expect_form(eng, P, N, n, CM, kernel, 64, 1, 1, tailed_fits=False, chained_fits=False)
        _host_solve_against_the_oracle("mode %d %s, %d x %d x %d candidate-major" % (mode, window, P, N, n), eng, mode, window,
                                       problems, N, n, CM)
        eng.close()


@pytest.mark.parametrize("H,P,N,kernel,table", [(9, 32, 4096, "rows", "scalar"),     # 2 048 tiles: the rows kernel
                                                (9, 31, 4096, "tile", None),         # 1 984
                                                (9, 32, 4095, "rows", "scalar"),     # ... with a ragged last tile in every problem
                                                (9, 2048, 65, "rows", "scalar"),     # 2 N n % 4 == 0: two tiles per problem, one row in the second
                                                (4, 2048, 65, "tile", None),         # 3 steps: 2 N n % 4 == 2, problems' spans on 8 bytes
                                                (81, 32, 4096, "rows", "scalar"),    # 80 steps: the largest register size
                                                (82, 32, 4096, "tile", None),        # 81
                                                (50, 32, 4096, "rows", "lds")])      # the table's rows from LDS
def test_the_rows_kernel_on_and_off(H, P, N, kernel, table):
    from acmpc_amd import Engine
    n = H - 1
    problems = [_problem("monza", H, 300 + p % 7) for p in range(P)]
    eng = Engine(**engine_kwargs(problems[0], 0, P, N, n))
    eng.set_paths(np.stack([p["table"] for p in problems]))
    d = _expect_form(eng, P, N, n, CM, kernel, 64, 1, 1, solo=False)
    assert d["table"] == table
    _host_solve_against_the_oracle("%d x %d x %d candidate-major" % (P, N, n), eng, 0, None, problems, N, n, CM)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# b. forced shapes, at sizes where lanes of several candidates go wrong
# ---------------------------------------------------------------------------------------------------------------------------
SIZES = {4: (4,        # one active lane
             8,        # two
             1020,     # a ragged last wave
             1028,     # a second workgroup with one active lane
             2052),    # a third
         2: (2, 510, 514)}


@pytest.mark.parametrize("H", [3, 20, 50])
@pytest.mark.parametrize("cpt", [4, 2])
def test_mode_s_forced_lane_widths_through_every_path(cpt, H):
    for P in (1, 3):
        dev = _Device(0, None, "monza", H, P, max(SIZES[cpt]))
        dev.eng.set_option("ACMPC_SHAPE", "256,%d" % cpt)
        for N in SIZES[cpt]:
            _expect_form(dev.eng, P, N, dev.n, SM, "step", 256, cpt, 2, tailed_fits=True, chained_fits=True, solo=False)
            dev.every_path("mode S 256,%d: %d x %d x %d" % (cpt, P, N, dev.n), N, cpt)
        dev.close()


@pytest.mark.parametrize("pack", [1, 2])     # ACMPC_T_PACK=2: the packed arithmetic - the plain form's bits
@pytest.mark.parametrize("window", [None, (2, 5), (1, 2)])
@pytest.mark.parametrize("cpt", [4, 2])
def test_mode_t_forced_lane_widths_through_every_path(cpt, window, pack):
    """With the exhaustive search (window None, horizons of 8 steps and more) the tail lanes of the last workgroup roll a
    dummy - the problem's last cpt candidates - because every lane must reach the wave-wide fallback of the verified search:
    N = 4, 8, 1020 and 1028 leave such lanes behind lanes of two and four candidates."""
    for H in (3, 20, 50):
        for P in (1, 3):
            dev = _Device(1, window, "silverstone", H, P, max(SIZES[cpt]))
            dev.eng.set_option("ACMPC_SHAPE", "256,%d" % cpt)
            dev.eng.set_option("ACMPC_T_PACK", pack if pack == 2 else None)
            for N in SIZES[cpt]:
                _expect_form(dev.eng, P, N, dev.n, SM, "step", 256, cpt, pack, tailed_fits=False, chained_fits=False, solo=False)
                dev.every_path("mode T %s pack %d 256,%d: %d x %d x %d" % (window, pack, cpt, P, N, dev.n), N, cpt)
            dev.close()


@pytest.mark.parametrize("cpt", [1, 2, 4])
@pytest.mark.parametrize("H,fits", [(60, True), (61, False)])
def test_the_chained_stream_at_its_last_horizon(H, fits, cpt):
    """59 steps: the last horizon whose pending finalize (four problems per workgroup) rides in the next batch's rollout
    launch; at 60 the stream runs it as a launch of its own in front.  The same records either way."""
    P, N = 5, 1028
    dev = _Device(0, None, "monza", H, P, N)
    dev.eng.set_option("ACMPC_SHAPE", "256,%d" % cpt)
    _expect_form(dev.eng, P, N, dev.n, SM, "step", 256, cpt, 2 if cpt > 1 else 1, tailed_fits=True, chained_fits=fits, solo=False)
    batches = []
    for k in range(3):
        U = dev.matrix(N, 99 + k, k)
        batches.append((U, dev.reference(U), 99 + k, k))
    dev.stream("%d steps, 256,%d" % (dev.n, cpt), batches, N, True)
    dev.stream("%d steps, 256,%d" % (dev.n, cpt), batches, N, False)
    dev.close()


def test_one_candidate_per_lane_takes_a_matrix_on_any_float_boundary():
    """include/acmpc.h: only lanes of two or four candidates need `d_U` and `d_costs` on an 8- / 16-byte boundary
    (tests/test_rollout_shapes.py has the refusal).  Views four bytes into their buffers, one candidate per lane."""
    import torch
    P, N, H = 3, 1028, 20
    dev = _Device(0, None, "monza", H, P, N)
    n = dev.n
    dev.eng.set_option("ACMPC_SHAPE", "256,1")
    _expect_form(dev.eng, P, N, n, SM, "step", 256, 1, 1)
    U = dev.matrix(N, 77, 0)
    ref = dev.reference(U)
    raw_U = torch.empty(U.numel() + 1, device=dev.dev)
    raw_costs = torch.empty(P * N + 1, device=dev.dev)
    raw_U[1:] = U.reshape(-1)
    assert raw_U[1:].data_ptr() % 8 == 4 and raw_costs[1:].data_ptr() % 8 == 4
    _, keys, rec = dev.outputs(N)
    dev.eng.solve_device(dev.x0.data_ptr(), raw_U[1:].data_ptr(), P, N, n, SM, raw_costs[1:].data_ptr(), keys.data_ptr(),
                         rec.data_ptr(), dev.s)
    costs, keys, rec = dev.host(raw_costs[1:].reshape(P, N), keys, rec)
    _verify("views four bytes in", ref, n, costs, keys, rec)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# c. random shapes
# ---------------------------------------------------------------------------------------------------------------------------
def _fuzz_case(rng):
    mode = int(rng.integers(0, 2))
    layout = int(rng.integers(0, 2))
    forced = [None, (64, 1), (256, 1), (256, 2), (256, 4)][int(rng.integers(0, 5))]
    cpt = forced[1] if forced else 1
    edge = int(rng.choice([64, 256, 1024])) * cpt                       # a wave's, a workgroup's, four workgroups' candidates
    N = max(cpt, edge + cpt * int(rng.integers(-2, 3)))                 # ... and multiples of the lane's candidates round it
    P = int(rng.integers(1, 5))
    H = int(rng.choice([3, 4, 9, 17, 20, 33, 50, 66, 114, 115, 129, 130]))
    window = [None, (2, 5), (1, 2), (0, 2)][int(rng.integers(0, 4))] if mode == 1 else None
    pack = int(rng.integers(1, 3)) if mode == 1 else 0
    track = ["monza", "spa", "nordschleife", "silverstone"][int(rng.integers(0, 4))]
    return mode, layout, forced, N, P, H, window, pack, track


def test_random_shapes_and_forced_forms_against_the_c_oracle():
    """Mode, layout, a forced shape or none, N in multiples of the lane's candidates round 64 / 256 / 1 024 lanes, 1 - 4
    problems, horizon, search window and track from a seeded generator (ACMPC_FUZZ_CASES cases, default 40)."""
    from acmpc_amd import Engine
    cases = int(os.environ.get("ACMPC_FUZZ_CASES", "40"))
    rng = np.random.default_rng(20261019)
    for index in range(cases):
        mode, layout, forced, N, P, H, window, pack, track = _fuzz_case(rng)
        n = H - 1
        label = "case %d: mode %d layout %d forced %s N %d P %d H %d window %s pack %d %s" % (index, mode, layout, forced, N, P, H,
                                                                                          window, pack, track)
        problems = [_problem(track, H, 9000 + 10 * (index % 5) + p) for p in range(P)]
        eng = Engine(**engine_kwargs(problems[0], mode, P, N, n, nn_window=window))
        eng.set_paths(np.stack([p["table"] for p in problems]))
        eng.set_option("ACMPC_NO_SOLO", 1)
        if forced:
            eng.set_option("ACMPC_SHAPE", "%d,%d" % forced)
        if pack == 2:
            eng.set_option("ACMPC_T_PACK", 2)
        # (all these launches have at most 131 072 candidates: 64 x 1 unless forced; candidate-major takes no forced width)
        if layout == CM and n <= (128 if mode == 0 else 113):
            want = ("tile", 64, 1, 1)
        elif forced and (layout == SM or forced[1] == 1):
            want = ("step", forced[0], forced[1], 1 if forced[1] == 1 else 2 if mode == 0 else pack)
        else:
            want = ("step", 64, 1, 1)
        _expect_form(eng, P, N, n, layout, *want, solo=False)
        _host_solve_against_the_oracle(label, eng, mode, window, problems, N, n, layout, seed=index)
        eng.close()
