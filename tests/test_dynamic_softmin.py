"""Mode D's softmin recentring without a GPU: acmpc_softmin_sampled_device exists on handles of every mode and refuses what
it must before any device work, acmpc_optimize no longer refuses centre_update = 1 on a mode D handle, the solver's config
key, and the restatement of one softmin solve (tests/dynamic_softmin_spec.py)."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_softmin_spec as dsm
import dynamic_spec as ds
from test_support import engine_kwargs, make_problem

FAKE = 0x1000   # a non-null "device pointer": every call below must return before anything reads it
N_CAP, N_STEPS = 64, 19


def _softmin_sampled(eng, costs=FAKE, keys=FAKE, centre=FAKE, mean=FAKE, stride=None, P=1, N=N_CAP, n=N_STEPS, offset=0):
    eng.softmin_sampled_device(costs, keys, centre, 2 * n if stride is None else stride, 0, P, N, n, offset, (0.05, 0.3), 7,
                               0, mean, 0, 0)


def _handle(mode, with_tables=True, **extra):
    from acmpc_amd import DynamicBicycleParams, Engine
    if mode == 2:
        dp = ds.make_dynamic_problem(orc, "monza", N_STEPS + 1, N_CAP, 0)
        eng = Engine(**dict(dp["kw"], max_problems=1, max_candidates=N_CAP, max_steps=N_STEPS, **extra))
        if with_tables:
            eng.set_dynamics(DynamicBicycleParams.reference())
            eng.set_paths(dp["table"])
        return eng, dp
    prob = make_problem(orc, "monza", N_STEPS + 1, N_CAP, seed=0)
    eng = Engine(**engine_kwargs(prob, mode, 1, N_CAP, N_STEPS, **extra))
    if with_tables:
        eng.set_paths(prob["table"])
    return eng, prob


def test_the_symbol_is_declared_and_bound():
    from acmpc_amd import _capi
    lib = _capi.load_library()
    assert hasattr(lib, "acmpc_softmin_sampled_device")
    assert "acmpc_softmin_sampled_device" in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["acmpc_softmin_sampled_device"][1]) == 17
    assert hasattr(_capi.Engine, "softmin_sampled_device")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_argument_checks_come_before_any_device_work(mode):
    from acmpc_amd import EngineError, _capi
    eng, _ = _handle(mode)

    def refused(code, **kw):
        with pytest.raises(EngineError) as e:
            _softmin_sampled(eng, **kw)
        assert e.value.code == code, (kw, str(e.value))

    for name in ("costs", "keys", "centre", "mean"):
        refused(_capi.EINVAL, **{name: 0})
    refused(_capi.EINVAL, stride=2 * N_STEPS - 1)
    refused(_capi.EINVAL, offset=-1)
    refused(_capi.EINVAL, offset=(1 << 32) - 10)   # global indices are 32 bits
    refused(_capi.ECAPACITY, N=N_CAP + 1)
    refused(_capi.ECAPACITY, P=2)
    refused(_capi.EINVAL, N=0)
    eng.close()
    for lam in (0.0, -1.0, float("nan")):
        eng, _ = _handle(mode, softmin_lambda=lam)
        with pytest.raises(EngineError) as e:
            _softmin_sampled(eng)
        assert e.value.code == _capi.EINVAL and "softmin_lambda" in str(e.value)
        eng.close()
    eng, _ = _handle(mode, with_tables=False)   # no paths (mode D: no vehicle) yet
    with pytest.raises(EngineError) as e:
        _softmin_sampled(eng)
    assert e.value.code == _capi.ESTATE
    eng.close()


def test_optimize_accepts_the_softmin_update_on_a_mode_d_handle():
    """centre_update = 1 used to come back as ACMPC_ESTATE from acmpc_optimize's argument path: it now reaches the device
    (and, where there is none, fails there)."""
    from acmpc_amd import EngineError, _capi
    eng, dp = _handle(2, centre_update="softmin")
    centre = np.zeros((1, N_STEPS, 2), dtype=np.float32)
    try:
        out = eng.optimize(dp["x0"][None], centre, None, N_CAP, 2, (0.05, 0.3), seed=3)
        assert np.isfinite(out["cost"][0])
    except EngineError as e:
        assert e.code == _capi.ENODEVICE, str(e)
    with pytest.raises(EngineError) as e:   # the other argument checks are still there
        eng.optimize(dp["x0"][None], centre, None, N_CAP, 0, (0.05, 0.3), seed=3)
    assert e.value.code == _capi.EINVAL
    eng.close()


def test_the_solver_reads_sampling_update():
    from acmpc_amd import DynamicBicycleParams
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver
    base = DynamicBicycleParams.reference()
    cfg = dict(horizon=20, n_candidates=256)
    with pytest.raises(ValueError, match="sampling_update"):
        DynamicSamplingSolver(dict(cfg, sampling_update="mean"), base)
    with pytest.raises(ValueError, match="softmin_lambda"):
        DynamicSamplingSolver(dict(cfg, sampling_update="softmin", softmin_lambda=0.0), base)
    for update, want in (("argmin", 0), ("softmin", 1)):   # built without device work
        solver = DynamicSamplingSolver(dict(cfg, sampling_update=update, softmin_lambda=0.25), base)
        assert solver.engine.params.centre_update == want and solver.engine.params.softmin_lambda == 0.25
        solver.close()
    solver = DynamicSamplingSolver(cfg, base)
    assert solver.engine.params.centre_update == 0 and solver.engine.params.softmin_lambda == 1.0
    solver.close()


def test_sharded_optimizer_rejects_an_unknown_update():
    torch = pytest.importorskip("torch")
    from acmpc_amd.sharding import ShardedOptimizer
    eng, _ = _handle(2)
    with pytest.raises(ValueError, match="centre_update"):
        ShardedOptimizer(eng, 1, N_CAP, N_STEPS, 0, torch.device("cpu"), centre_update="mean")
    eng.close()


@pytest.fixture(scope="module")
def restated():
    """One softmin solve at a small size: N = 256, n = 12, 3 rounds, candidate 1 of round 0 given."""
    from acmpc_amd import DynamicBicycleParams
    N, n, rounds = 256, 12, 3
    dp = ds.make_dynamic_problem(orc, "monza", n + 1, 8, 3)
    coef = orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(np.float32)
    rng = np.random.default_rng(2)
    centre = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.2, 0.4, n)], axis=1).astype(np.float32)
    u_ref = np.stack([np.zeros(n), np.full(n, 0.1)], axis=1).astype(np.float32)
    sigma, shrink, lam = (0.05, 0.3), 0.5, 1.0
    out = dsm.solve(orc, dp, coef, [DynamicBicycleParams.reference().coefficients()], centre, u_ref, N, rounds, sigma,
                    shrink, 77, lam)
    return dict(rounds=out, centre=centre, u_ref=u_ref, sigma=sigma, shrink=shrink, lam=lam, dp=dp)


def test_restated_rounds_follow_the_protocol(restated):
    rounds = restated["rounds"]
    assert len(rounds) == 3
    lo, hi = np.float32(restated["dp"]["kw"]["u_min"]), np.float32(restated["dp"]["kw"]["u_max"])
    # round 0: the caller's centre and reference; sigma shrink^r
    assert np.array_equal(rounds[0]["U"][0], np.clip(restated["centre"], lo, hi))
    assert np.array_equal(rounds[0]["U"][1], np.clip(restated["u_ref"], lo, hi))
    for r, rd in enumerate(rounds):
        assert rd["sigma"] == (restated["sigma"][0] * restated["shrink"] ** r, restated["sigma"][1] * restated["shrink"] ** r)
    # candidate 0 of round r + 1 is round r's mean, candidate 1 its winner; no mean after the last round
    for prev, nxt in zip(rounds, rounds[1:]):
        assert prev["mean"] is not None and prev["mean"].dtype == np.float32
        assert np.all(prev["mean"] >= lo) and np.all(prev["mean"] <= hi)
        assert np.array_equal(nxt["U"][0].view(np.uint32), prev["mean"].view(np.uint32))
        assert np.array_equal(nxt["U"][1].view(np.uint32), prev["U"][prev["best"]].view(np.uint32))
        assert nxt["cost"][1] == prev["cost"][prev["best"]]
    assert rounds[-1]["mean"] is None
    # the mean is the weighted mean: between the candidates' extremes, and not the winner itself at lambda = 1
    first = rounds[0]
    assert np.all(first["mean"] >= first["U"].min(axis=0)) and np.all(first["mean"] <= first["U"].max(axis=0))
    assert not np.array_equal(first["mean"], first["U"][first["best"]])


def test_restated_winner_cost_never_rises(restated):
    best = [rd["cost"][rd["best"]] for rd in restated["rounds"]]
    assert all(np.isfinite(best))
    assert all(b <= a for a, b in zip(best, best[1:]))


def test_restated_mean_falls_back_to_the_plain_mean_without_a_finite_cost():
    U = np.arange(24, dtype=np.float32).reshape(4, 3, 2)
    cost = np.array([np.nan, np.inf, np.nan, np.inf], dtype=np.float32)
    assert np.array_equal(dsm.softmin_mean(orc, cost, U, 1.0), U.mean(axis=0))
    cost[2] = 1.0   # one finite cost: that candidate alone
    assert np.array_equal(dsm.softmin_mean(orc, cost, U, 1.0), U[2])
