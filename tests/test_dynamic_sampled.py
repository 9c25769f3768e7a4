"""Mode D's sampled call forms without a GPU: acmpc_rollout_sampled_device exists and refuses what it must before any
device work, and the restatement of its candidates (tests/dynamic_sampled_spec.py) is consistent across shards."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_sampled_spec as dss
import dynamic_spec as ds
from test_support import engine_kwargs, make_problem

FAKE = 0x1000   # a non-null "device pointer": every call below must return before anything reads it


def _rollout_sampled(eng, x0=FAKE, centre=FAKE, stride=None, P=1, N=64, n=19, offset=0):
    eng.rollout_sampled_device(x0, centre, 2 * n if stride is None else stride, 0, P, N, n, offset, (0.05, 0.3), 7, 0, 0, 0)


def test_the_symbol_is_declared_and_bound():
    from acmpc_amd import _capi
    lib = _capi.load_library()
    assert hasattr(lib, "acmpc_rollout_sampled_device")
    assert "acmpc_rollout_sampled_device" in _capi.SIGNATURES
    assert hasattr(_capi.Engine, "rollout_sampled_device")


@pytest.mark.parametrize("mode", [0, 1])
def test_modes_s_and_t_are_refused_before_any_device_work(mode):
    from acmpc_amd import Engine, EngineError, _capi
    prob = make_problem(orc, "monza", 20, 64, seed=0)
    eng = Engine(**engine_kwargs(prob, mode, 1, 64, 19))
    eng.set_paths(prob["table"])
    with pytest.raises(EngineError) as e:
        _rollout_sampled(eng)
    assert e.value.code == _capi.ESTATE
    eng.close()


def test_argument_checks_come_first_on_a_mode_d_handle():
    from acmpc_amd import DynamicBicycleParams, Engine, EngineError, _capi
    dp = ds.make_dynamic_problem(orc, "monza", 20, 64, 0)
    eng = Engine(**dict(dp["kw"], max_problems=1, max_candidates=64, max_steps=19))

    def refused(code, **kw):
        with pytest.raises(EngineError) as e:
            _rollout_sampled(eng, **kw)
        assert e.value.code == code, (kw, str(e.value))

    refused(_capi.EINVAL, x0=0)
    refused(_capi.EINVAL, centre=0)
    refused(_capi.ESTATE)                       # no vehicle yet
    eng.set_dynamics(DynamicBicycleParams.reference())
    refused(_capi.ESTATE)                       # no paths yet
    eng.set_paths(dp["table"])
    refused(_capi.EINVAL, x0=0)
    refused(_capi.EINVAL, stride=2 * 19 - 1)
    refused(_capi.EINVAL, offset=-1)
    refused(_capi.EINVAL, offset=(1 << 32) - 10)   # global indices are 32 bits
    refused(_capi.ECAPACITY, N=65)
    refused(_capi.ECAPACITY, P=2)
    refused(_capi.EINVAL, N=0)
    eng.close()


def test_the_matrix_rounds_switch_is_an_option_of_the_handle():
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 64, 0)
    eng = Engine(**dict(dp["kw"], max_problems=1, max_candidates=64, max_steps=19))
    eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", "1")
    eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", None)
    eng.close()


def test_pack_key_of_the_restatement_is_the_librarys():
    from acmpc_amd import _capi
    for cost in (0.0, -0.0, 1.5, -2.25, 3.0e38, -3.0e38, np.inf, -np.inf, np.nan, 1e-42):
        for index in (0, 1, 7, 3_000_000_013, (1 << 32) - 1):
            assert dss.pack_key(np.float32(cost), index) == _capi.pack_key(float(np.float32(cost)), index), (cost, index)


@pytest.mark.parametrize("with_ref", [False, True])
def test_shards_drawn_with_an_offset_concatenate_to_the_whole(with_ref):
    """Candidate c of a shard at index_offset is global candidate index_offset + c: four slices of a launch, drawn one by
    one, are the launch - candidates 0 (the centre) and 1 (u_ref) only where their global indices fall."""
    n, N, problem, round_, seed, sigma = 19, 1003, 2, 3, 0x123456789ABC, (0.05, 0.3)
    dp = ds.make_dynamic_problem(orc, "monza", n + 1, 8, 4)
    rng = np.random.default_rng(1)
    centre = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.2, 0.6, n)], axis=1).astype(np.float32)
    u_ref = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.2, 0.6, n)], axis=1).astype(np.float32) if with_ref else None
    for base in (0, 3_000_000_013):
        whole = dss.candidates(orc, dp, centre, u_ref, N, base, problem, round_, seed, sigma)
        cuts = [0, 250, 251, 760, N]
        parts = [dss.candidates(orc, dp, centre, u_ref, hi - lo, base + lo, problem, round_, seed, sigma)
                 for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
        box_lo, box_hi = np.float32(dp["kw"]["u_min"]), np.float32(dp["kw"]["u_max"])
        assert np.all(whole >= box_lo) and np.all(whole <= box_hi)
        if base == 0:
            assert np.array_equal(whole[0], np.clip(centre, box_lo, box_hi))
            if with_ref:
                assert np.array_equal(whole[1], np.clip(u_ref, box_lo, box_hi))
        else:   # global candidates 0 and 1 lie outside this launch: every candidate is a draw
            assert not np.any(np.all(whole == np.clip(centre, box_lo, box_hi), axis=(1, 2)))
