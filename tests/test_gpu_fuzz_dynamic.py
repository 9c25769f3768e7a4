"""Randomised shapes for mode D, in the style of tests/test_gpu_fuzz.py: layout, horizon, candidate count, problem
count, search window, path family, problem kind, ensemble size, reduce and weights drawn from a seeded generator; every
per-candidate cost, the argmin, the feasible count and the winner's record must equal the float32 specification
(tests/dynamic_spec.py, tests/dynamic_ensemble_spec.py) bit for bit.  In front of the random cases, the longest horizon
the kernels accept (kDynamicMaxSteps = 512 steps) with both searches, one vehicle and three, both layouts.
ACMPC_FUZZ_CASES sets the number of random cases (default 40).  Every handle here keeps its default settings: the plain
kernels.  tests/test_gpu_fuzz_dynamic_settings.py draws the settings (integration, terms, objective, coupling, load transfer) and
the sampled call forms beside these shapes.

The specification is NumPy: a case costs about P K (3.3 ms n + 80 ns N n W) seconds of it (W waypoints searched per
step).  A case drawn above BUDGET_S gives up problems first, then vehicles, then candidates - never its horizon, window
or layout; beyond 130 waypoints N is drawn from the values up to 257."""
import os

import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_ensemble_spec as es
import dynamic_spec as ds
import test_gpu_dynamic_ensemble as tge

pytestmark = pytest.mark.gpu

HORIZONS = [3, 4, 9, 17, 33, 50, 65, 66, 100, 130, 257, 513]
CANDIDATES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1000, 2049]
WINDOWS = [None, (2, 5), (1, 2), (0, 2), (3, 12), (20, 43)]   # (20, 43): 64 waypoints, the widest acmpc_create accepts
TRACKS = ["monza", "spa", "nordschleife", "silverstone"]
ENSEMBLE_SIZES = [1, 1, 2, 3, 5, 8]
KIND = [dict(), dict(vx0=0.0), dict(yaw_turns=-1), dict(origin=(3000.0, 2700.0))]   # test_gpu_dynamic._problems' four
BUDGET_S = 2.0


def _spec_seconds(P, K, N, n, window):
    W = n if window is None else min(window[0] + window[1] + 1, n)
    return P * K * (3.3e-3 * n + 8.0e-8 * N * n * W)


def _case(rng):
    layout = int(rng.integers(0, 2))
    H = int(rng.choice(HORIZONS))
    N = int(rng.choice(CANDIDATES if H <= 130 else [c for c in CANDIDATES if c <= 257]))
    P = int(rng.integers(1, 5))
    window = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
    track = TRACKS[int(rng.integers(0, 4))]
    kinds = [int(k) for k in rng.integers(0, 4, 4)]
    K = int(rng.choice(ENSEMBLE_SIZES))
    vehicles = [int(v) for v in rng.permutation(8)]
    reduce = ["mean", "max"][int(rng.integers(0, 2))]
    weights = [float(x) for x in rng.uniform(0.2, 3.0, 8)] if rng.integers(0, 2) else None
    n = H - 1
    while _spec_seconds(P, K, N, n, window) > BUDGET_S:
        if P > 1:
            P -= 1
        elif K > 1:
            K = max(k for k in ENSEMBLE_SIZES if k < K)
        elif N > 1:
            N = max(c for c in CANDIDATES if c < N)
        else:
            break
    return dict(layout=layout, H=H, N=N, P=P, window=window, track=track, kinds=kinds[:P], K=K, vehicles=vehicles[:K],
                reduce=reduce, weights=None if weights is None else weights[:K])


def _label(index, c):
    return "case %s: layout %d H %d N %d P %d window %s %s kinds %s K %d vehicles %s %s weights %s" % (
        index, c["layout"], c["H"], c["N"], c["P"], c["window"], c["track"], c["kinds"], c["K"], c["vehicles"], c["reduce"],
        c["weights"])


def _problems(c, seed, plant):
    out = [ds.make_dynamic_problem(orc, c["track"], c["H"], c["N"], seed + p, **KIND[kind])
           for p, kind in enumerate(c["kinds"])]
    if plant and c["N"] > 8:                      # some non-finite candidates
        n = c["H"] - 1
        out[0]["U"][5, n // 2, 0] = np.nan
        out[0]["U"][7, 0, 1] = np.inf
    return out


def _specification(c, problems, coefs):
    blocks = [tge._vehicles()[v].coefficients() for v in c["vehicles"]]
    want = []
    for dp, coef in zip(problems, coefs):
        if c["K"] == 1:
            want.append(ds.spec_costs(orc, dp, coef, blocks[0], nn_window=c["window"], return_states=True))
        else:
            want.append(es.spec_ensemble(orc, dp, coef, blocks, reduce=c["reduce"], weights=c["weights"],
                                         nn_window=c["window"], return_states=True))
    return want


def _engine(c, problems):
    from acmpc_amd import Engine
    n = c["H"] - 1
    eng = Engine(**dict(problems[0]["kw"], max_problems=c["P"], max_candidates=c["N"], max_steps=n, nn_window=c["window"]))
    try:
        if c["K"] == 1:
            eng.set_dynamics(tge._vehicles()[c["vehicles"][0]])
        else:
            eng.set_dynamics_ensemble([tge._vehicles()[v] for v in c["vehicles"]], weights=c["weights"], reduce=c["reduce"])
        eng.set_paths(np.stack([dp["table"] for dp in problems]))
    except Exception:
        eng.close()
        raise
    return eng


def _same_bits(got, want, message):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), message
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), message


def _solve_and_check(eng, c, problems, want, label):
    from acmpc_amd import _capi
    n = c["H"] - 1
    U = np.stack([dp["U"] for dp in problems])
    data = U if c["layout"] == 0 else np.ascontiguousarray(U.transpose(0, 2, 3, 1))
    out = eng.solve(np.stack([dp["x0"] for dp in problems]), data, layout=c["layout"])
    for p, (cost, V, X) in enumerate(want):
        where = "%s, problem %d" % (label, p)
        _same_bits(out["costs"][p], cost, where + ": costs")
        best = orc.pick_best(cost)[0]
        assert out["best_idx"][p] == best, where
        assert out["n_feasible"][p] == np.count_nonzero(V == 0), where
        rec = _capi.split_record(out["records"][p], n)
        assert rec["owner"] == 1.0, where
        _same_bits(rec["cost"], cost[best], where + ": the record's cost")
        _same_bits(rec["violation"], V[best], where + ": the record's violation")
        _same_bits(rec["u"], U[p][best], where + ": the record's controls")
        _same_bits(rec["x"], X[best], where + ": the record's states")


# the longest horizon, H = 513: both searches, one vehicle and three; each specification serves both layouts
LONGEST = [dict(H=513, N=17, P=1, window=None, track="monza", kinds=[0], K=1, vehicles=[0], reduce="mean", weights=None),
           dict(H=513, N=257, P=2, window=(20, 43), track="silverstone", kinds=[3, 1], K=1, vehicles=[0], reduce="mean",
                weights=None),
           dict(H=513, N=9, P=1, window=None, track="silverstone", kinds=[2], K=3, vehicles=[0, 3, 2], reduce="mean",
                weights=[1.0, 2.0, 0.5]),
           dict(H=513, N=129, P=1, window=(2, 5), track="monza", kinds=[0], K=3, vehicles=[0, 1, 3], reduce="max",
                weights=None)]


def test_random_mode_d_shapes_against_the_specification():
    cases = int(os.environ.get("ACMPC_FUZZ_CASES", "40"))
    rng = np.random.default_rng(20261016)
    todo = [("longest %d" % i, c, 15000 + 10 * i, i == 1, (0, 1)) for i, c in enumerate(LONGEST)]
    for index in range(cases):
        c = _case(rng)
        todo.append((str(index), c, 16000 + 10 * index, index % 7 == 3, (c["layout"],)))
    for index, c, seed, plant, layouts in todo:
        problems = _problems(c, seed, plant)
        want = None
        for layout in layouts:
            c = dict(c, layout=layout)
            label = _label(index, c)
            eng = _engine(c, problems)
            try:
                if want is None:
                    want = _specification(c, problems, [eng.coefficients(p) for p in range(c["P"])])
                _solve_and_check(eng, c, problems, want, label)
            finally:
                eng.close()
