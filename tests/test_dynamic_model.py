"""Mode D on the CPU: the float64 host mirror against the reference's own steps (tests/golden/dynamic_bicycle.npz), the
vehicle block, the float32 specification's arctangent and its drift from the mirror, and the C ABI's host-side checks."""
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
import dynamic_spec as ds  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "dynamic_bicycle.npz"))
# the float32 specification rolled 50 steps of 0.05 s against the float64 mirror: largest position gap (measured 5.1e-5 m)
POSITION_BOUND_M = 1.0e-3


def _params():
    from acmpc_amd.dynamic_model import DynamicBicycleParams
    return DynamicBicycleParams


def test_literal_block_is_the_reference_bit_for_bit():
    P = _params()
    assert np.array_equal(P.reference(literal=True).coefficients(), GOLDEN["coef_literal"])
    assert np.array_equal(P.reference().coefficients(), GOLDEN["coef_kn"])
    assert tuple(GOLDEN["fields"]) == ds.FIELDS
    from acmpc_amd.dynamic_model import FIELDS
    assert FIELDS == ds.FIELDS


def test_host_mirror_equals_the_reference_steps():
    P = _params()
    blocks = (P.from_coefficients(GOLDEN["coef_literal"]), P.from_coefficients(GOLDEN["coef_kn"]))
    assert len(GOLDEN["step_state"]) >= 300
    for s, u, dt, b, nxt, xd, f in zip(GOLDEN["step_state"], GOLDEN["step_u"], GOLDEN["step_dt"], GOLDEN["step_block"],
                                       GOLDEN["step_next"], GOLDEN["step_xdot"], GOLDEN["step_forces"]):
        got_next, got_xd, got_f = blocks[int(b)].predict_next_state(s, u, float(dt))
        # a tolerance, not equality: NumPy's SIMD arctan differs between builds
        np.testing.assert_allclose(got_next, nxt, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got_xd, xd, rtol=1e-12, atol=1e-10)
        np.testing.assert_allclose(np.array(got_f), f, rtol=1e-12, atol=1e-10)


def test_host_mirror_rollouts_with_the_clip():
    P = _params()
    p = P.reference()
    for x0, U, S in zip(GOLDEN["roll_x0"], GOLDEN["roll_u"], GOLDEN["roll_states"]):
        np.testing.assert_allclose(p.rollout(x0, U, float(GOLDEN["roll_dt"])), S, rtol=1e-12, atol=1e-9)


def test_literal_block_is_not_unit_consistent_and_the_default_is():
    """DESIGN.md's units finding: the literal maps (N) against kN tyre forces move vx by 125 m/s in one 50 ms step."""
    P = _params()
    lit = P.reference(literal=True).predict_next_state([0, 0, 0, 20.0, 0, 0], [0.0, 0.5], 0.05)[0]
    assert abs(lit[3] - 20.0) > 100.0
    kn = P.reference()
    state = np.array([0, 0, 0, 30.0, 0, 0])
    for _ in range(50):   # 2.5 s of full throttle
        state = kn.predict_next_state(state, [0.0, 1.0], 0.05)[0]
    assert 38.0 < state[3] < 42.0


def test_atan_spec_error_bound_and_special_values():
    x = np.concatenate([np.linspace(-8.0, 8.0, 2000001, dtype=np.float32),
                        np.geomspace(1e-38, 3e38, 400001).astype(np.float32),
                        -np.geomspace(1e-30, 1e30, 100001).astype(np.float32)])
    err = np.abs(ds.atan_spec(x).astype(np.float64) - np.arctan(x.astype(np.float64)))
    assert err.max() <= ds.ATAN_ERROR_BOUND
    special = ds.atan_spec(np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32))
    assert special[0] == 0.0 and not np.signbit(special[0])
    assert special[1] == 0.0 and np.signbit(special[1])
    assert special[2] == np.float32(np.pi / 2) and special[3] == -np.float32(np.pi / 2)
    assert np.isnan(special[4])


def test_float32_spec_tracks_the_float64_mirror():
    P = _params()
    p = P.reference()
    c = ds.constants(p.coefficients(), dt=float(GOLDEN["roll_dt"]))
    for x0, U, S in zip(GOLDEN["roll_x0"], GOLDEN["roll_u"], GOLDEN["roll_states"]):
        st = tuple(np.float32(v) for v in x0)
        traj = [np.array(st, dtype=np.float64)]
        for i, u in enumerate(U):
            one = np.array(ds.dynamic_step(tuple(np.float32(v) for v in S[i]), np.float32(u[0]), np.float32(u[1]), c),
                           dtype=np.float64)
            assert np.all(np.abs(one - S[i + 1]) <= 1e-5 * np.maximum(np.abs(S[i + 1]), 1.0))
            st = ds.dynamic_step(st, np.float32(u[0]), np.float32(u[1]), c)
            traj.append(np.array(st, dtype=np.float64))
        traj = np.array(traj)
        assert np.max(np.hypot(traj[:, 0] - S[:, 0], traj[:, 1] - S[:, 1])) < POSITION_BOUND_M


def _engine(**extra):
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    kw = dict(dp["kw"])
    kw.update(extra)
    return Engine(**kw), dp


def test_set_dynamics_rejects_bad_blocks_and_other_modes():
    from acmpc_amd import EngineError
    P = _params()
    eng, dp = _engine()
    good = P.reference().coefficients()
    eng.set_dynamics(good)
    for bad in (good[:-1], np.append(good, 1.0)):
        with pytest.raises(EngineError) as e:
            eng.set_dynamics(bad)
        assert e.value.code == -1
    for field, value in (("mass", 0.0), ("Iz", -1.0), ("Bf", np.nan), ("Cm1", np.inf), ("mass", -1.0)):
        b = good.copy()
        b[ds.FIELDS.index(field)] = value
        with pytest.raises(EngineError) as e:
            eng.set_dynamics(b)
        assert e.value.code == -1
    eng.close()
    for mode in (0, 1):
        other, _ = _engine(mode=mode)
        with pytest.raises(EngineError) as e:
            other.set_dynamics(good)
        assert e.value.code == -1
        other.close()


def test_mode_d_refuses_lq_and_solves_without_dynamics():
    from acmpc_amd import EngineError
    with pytest.raises(EngineError) as e:
        _engine(lq_candidate=1)
    assert e.value.code == -1
    with pytest.raises(EngineError) as e:
        _engine(max_steps=513)
    assert e.value.code == -1
    eng, dp = _engine()
    eng.set_paths(dp["table"])
    with pytest.raises(EngineError) as e:   # before acmpc_set_dynamics: ESTATE, checked before any device work
        eng.solve(dp["x0"][None], dp["U"][None])
    assert e.value.code == -5
    eng.close()


def test_mode_d_tables_are_mode_t_tables():
    from acmpc_amd import Engine
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    eng = Engine(**dp["kw"])
    eng.set_paths(dp["table"])
    expect = orc.coefficients_temporal(dp["table"], dp["kw"]["margin"]).astype(np.float32)
    assert np.array_equal(eng.coefficients(0), expect)
    eng.close()
