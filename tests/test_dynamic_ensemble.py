"""Mode D's ensemble of vehicles on the CPU: acmpc_set_dynamics_ensemble's refusals (host-side, no device work), the
grip scaling of a vehicle, the NumPy restatement of the combine (tests/dynamic_ensemble_spec.py) and the solver's
config checks."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "ac-mpc_amd"), os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acmpc_oracle as orc  # noqa: E402
import dynamic_ensemble_spec as es  # noqa: E402
import dynamic_spec as ds  # noqa: E402

EINVAL, ESTATE = -1, -5


def _engine(**extra):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    kw = dict(dp["kw"])
    kw.update(extra)
    return Engine(**kw), dp


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_ensemble_entry_point_is_exported():
    import acmpc_amd
    from acmpc_amd import _capi
    assert "acmpc_set_dynamics_ensemble" in _capi.SIGNATURES
    assert (acmpc_amd.MAX_VEHICLES, acmpc_amd.ENSEMBLE_MEAN, acmpc_amd.ENSEMBLE_MAX) == (8, 0, 1)
    assert hasattr(acmpc_amd.Engine, "set_dynamics_ensemble")


def test_set_dynamics_ensemble_refusals():
    from acmpc_amd import DynamicBicycleParams, EngineError
    from acmpc_amd import _capi
    good = DynamicBicycleParams.reference()
    eng, dp = _engine()
    eng.set_paths(dp["table"])
    lib, ctx = eng._lib, eng._ctx
    blocks = np.ascontiguousarray(np.stack([good.coefficients()] * 9))
    for K in (0, 9, -1):   # K outside 1 .. 8 (the raw call: the Python wrapper cannot even spell K = 0)
        assert lib.acmpc_set_dynamics_ensemble(ctx, blocks.ctypes.data, K, None, 0) == EINVAL
    for reduce in (2, -1):
        assert lib.acmpc_set_dynamics_ensemble(ctx, blocks.ctypes.data, 2, None, reduce) == EINVAL
    assert lib.acmpc_set_dynamics_ensemble(ctx, None, 2, None, 0) == EINVAL
    with pytest.raises(ValueError):
        eng.set_dynamics_ensemble([good, good], reduce="median")
    with pytest.raises(ValueError):
        eng.set_dynamics_ensemble([good, good], weights=[1.0])
    for w in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(EngineError) as e:
            eng.set_dynamics_ensemble([good, good, good], weights=[1.0, w, 1.0])
        assert e.value.code == EINVAL
    # one bad block among good ones: refused, and nothing kept - the handle still has no vehicle (ESTATE, checked
    # before any device work)
    for field, value in (("mass", 0.0), ("Iz", -1.0), ("Bf", np.nan), ("F_z0", 0.0)):
        bad = good.coefficients()
        bad[ds.FIELDS.index(field)] = value
        with pytest.raises(EngineError) as e:
            eng.set_dynamics_ensemble([good, good, bad, good], reduce="max")
        assert e.value.code == EINVAL
        assert "vehicle 2" in str(e.value)
    with pytest.raises(EngineError) as e:
        eng.solve(dp["x0"][None], dp["U"][None])
    assert e.value.code == ESTATE
    # good ensembles of every size are taken
    for K in range(1, _capi.MAX_VEHICLES + 1):
        eng.set_dynamics_ensemble([good.with_grip(1.0 - 0.05 * k) for k in range(K)], reduce="max")
        eng.set_dynamics_ensemble(np.stack([good.coefficients()] * K), weights=np.arange(1, K + 1))
    eng.close()
    for mode in (0, 1):   # not a mode D handle
        other, _ = _engine(mode=mode)
        with pytest.raises(EngineError) as e:
            other.set_dynamics_ensemble([good, good])
        assert e.value.code == EINVAL
        other.close()


def test_with_grip_scales_only_the_peak_factors():
    from acmpc_amd import DynamicBicycleParams
    from acmpc_amd.dynamic_model import FIELDS
    base = DynamicBicycleParams.reference()
    low = base.with_grip(0.85)
    for name in FIELDS:
        want = getattr(base, name) * 0.85 if name in ("Df", "Dr") else getattr(base, name)
        assert getattr(low, name) == want, name
    assert base.Df == 4.120 and base.Dr == 4.617   # a copy: the original is left as it was
    assert base.with_grip(1.0) == base
    for bad in (0.0, -0.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            base.with_grip(bad)


def _spec_problem(N=64, n=12, seed=3):
    from acmpc_amd import DynamicBicycleParams
    dp = ds.make_dynamic_problem(orc, "monza", n + 1, N, seed)
    coef = orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(np.float32)
    dp["U"][5, n // 2, 1] = np.nan
    return dp, coef, DynamicBicycleParams.reference()


def test_spec_of_one_vehicle_is_rollout_dynamic():
    dp, coef, v = _spec_problem()
    c, V, X = ds.spec_costs(orc, dp, coef, v.coefficients(), return_states=True)
    for reduce in (es.MEAN, es.MAX):
        for weights in (None, [3.0]):
            J, VE, XE = es.spec_ensemble(orc, dp, coef, [v.coefficients()], reduce=reduce, weights=weights,
                                         return_states=True)
            nan = np.isnan(c)
            assert np.array_equal(np.isnan(J), nan) and np.array_equal(_bits(J)[~nan], _bits(c)[~nan])
            assert np.array_equal(_bits(VE), _bits(V))
            assert np.array_equal(_bits(XE), _bits(X))
    # two copies under MEAN (omega = 0.5: fma(0.5, c, 0.5 c) = c) and four under MAX are the single vehicle too
    for blocks, reduce in (([v.coefficients()] * 2, es.MEAN), ([v.coefficients()] * 4, es.MAX)):
        J, VE = es.spec_ensemble(orc, dp, coef, blocks, reduce=reduce)
        nan = np.isnan(c)
        assert np.array_equal(np.isnan(J), nan) and np.array_equal(_bits(J)[~nan], _bits(c)[~nan])
        assert np.array_equal(_bits(VE), _bits(V))


def test_spec_of_a_grip_ensemble_combines_in_order():
    dp, coef, v = _spec_problem()
    vehicles = [v.with_grip(g).coefficients() for g in (1.0, 0.8, 1.1)]
    per = [ds.spec_costs(orc, dp, coef, b) for b in vehicles]
    J, V = es.spec_ensemble(orc, dp, coef, vehicles, weights=[2.0, 1.0, 1.0])
    om = es.omegas(3, [2.0, 1.0, 1.0])
    assert np.array_equal(_bits(om), _bits([0.5, 0.25, 0.25]))
    want = orc.fma32(om[2], per[2][0], orc.fma32(om[1], per[1][0], om[0] * per[0][0]))
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(J)[ok], _bits(want)[ok]) and np.all(np.isnan(J[~ok]))
    assert np.array_equal(_bits(V), _bits(np.maximum(np.maximum(per[0][1], per[1][1]), per[2][1])))
    Jmax, _ = es.spec_ensemble(orc, dp, coef, vehicles, reduce=es.MAX)
    assert np.array_equal(_bits(Jmax)[ok], _bits(np.max([p[0] for p in per], axis=0))[ok])
    assert np.isnan(J[5]) and np.isnan(Jmax[5])   # the NaN pedal


def test_combine_nan_and_inf():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    c = [np.array([1.0, nan, 2.0, inf, 3.0, 0.0], np.float32), np.array([4.0, 1.0, nan, 1.0, inf, 0.0], np.float32),
         np.array([2.0, 1.0, 1.0, 1.0, 1.0, 0.0], np.float32)]
    v = [np.array([0.0, 0.0, 0.0, 0.0, nan, 0.0], np.float32), np.array([0.0, 2.0, 0.0, 0.0, 0.0, 0.0], np.float32),
         np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0], np.float32)]
    J, V = es.combine(c, v, es.MAX)
    assert J[0] == 4.0 and np.isnan(J[1]) and np.isnan(J[2]) and J[3] == inf and J[4] == inf and J[5] == 0.0
    assert V[0] == 1.0 and V[1] == 2.0 and V[2] == 0.0 and np.isnan(V[4]) and V[5] == 0.0
    J, V = es.combine(c, v, es.MEAN)
    third = np.float32(1.0 / 3.0)
    assert J[0] == orc.fma32(third, np.float32(2.0), orc.fma32(third, np.float32(4.0), third * np.float32(1.0)))
    assert np.isnan(J[1]) and np.isnan(J[2]) and J[3] == inf and J[4] == inf
    # candidates non-finite under any vehicle rank last
    assert orc.pick_best(J)[0] == 5 and orc.pick_best(es.combine(c[:2], v[:2], es.MAX)[0][:5])[0] == 0


def test_solver_config_checks():
    from acmpc_amd import DynamicBicycleParams
    from acmpc_amd.dynamic_solver import DynamicSamplingSolver, ensemble_vehicles
    base = DynamicBicycleParams.reference()
    cfg = dict(horizon=20, n_candidates=256)
    with pytest.raises(ValueError, match="mutually exclusive"):
        DynamicSamplingSolver(dict(cfg, vehicle_ensemble=[base, base], grip_ensemble=[0.9, 1.0]))
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(cfg, grip_ensemble=[0.9, 1.0], ensemble_reduce="median"))
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(cfg, grip_ensemble=[0.9, 1.0], ensemble_weights=[1.0]))
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(cfg, grip_ensemble=[1.0] * 9))
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(cfg, ensemble_weights=[1.0, 2.0]))
    assert ensemble_vehicles(cfg, base) is None
    got = ensemble_vehicles(dict(cfg, grip_ensemble=[0.8, 1.0]), base)
    assert got == [base.with_grip(0.8), base.with_grip(1.0)]
    got = ensemble_vehicles(dict(cfg, vehicle_ensemble=[base, base.with_grip(0.9).coefficients()]), base)
    assert got == [base, base.with_grip(0.9)]
    # a solver with an ensemble is built without device work
    solver = DynamicSamplingSolver(dict(cfg, grip_ensemble=[0.85, 1.0, 1.1], ensemble_reduce="max",
                                        ensemble_weights=[1.0, 2.0, 1.0]), base)
    solver.close()
