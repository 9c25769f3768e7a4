"""Mode D's grip identification without a GPU: the float32 specification (tests/grip_spec.py) against the float64 mirror on
logs driven at known grips, the windows that carry no information, the derived constants of a hypothesis, every refusal of
acmpc_score_grips (all come before any device work), GripEstimator's bookkeeping with an injected scoring function, and the
solver's config check."""
import numpy as np
import pytest

import dynamic_spec as ds
import grip_spec as gs

GRID = 0.3 + 0.05 * np.arange(25)          # 0.3 .. 1.5, step 0.05
PLANTS = [(0.5, 0.7), (0.9, 0.6), (1.0, 1.0)]
AMPLITUDES = [0.005, 0.02]                 # rad: peak a_y 2.7 m/s^2 and about 10 m/s^2
NOISE = (0.05, 0.02, 0.01)                 # sigma on (vx, vy, r)
# |E32 - E64| <= E_RTOL E64 + E_ATOL over the 25 x 25 grid of the six logs below.  Measured, float32 specification against
# the float64 mirror on these very logs: 1.02e-5 relative at every grid point but the true one, x 4 for other libm builds
# (the mirror's sin / atan are libm's).  At the true grid point both sums are what rounding the log to float32 leaves -
# 2e-11 .. 5e-11 each, neither a reference for the other: they differ by up to 2.4e-11 (measured), x 4.
E_RTOL = 4.1e-5
E_ATOL = 1.0e-10

_logs = {}


def _base():
    from acmpc_amd import DynamicBicycleParams
    return DynamicBicycleParams.reference()


def _split_scales():
    from acmpc_amd.grip_estimator import grip_scales
    return grip_scales(GRID, "split")


def _log(plant, amplitude, noise=None):
    key = (plant, amplitude, noise)
    if key not in _logs:
        _logs[key] = gs.steering_log(_base().with_axle_grip(*plant), amplitude, noise=noise)
    return _logs[key]


@pytest.mark.parametrize("amplitude", AMPLITUDES)
@pytest.mark.parametrize("plant", PLANTS)
def test_specification_finds_the_grid_point_and_its_errors_are_the_mirrors(plant, amplitude):
    base, scales = _base(), _split_scales()
    states, controls = _log(plant, amplitude)
    E, best = gs.score(base.coefficients(), states, controls, 0.05, scales)
    assert tuple(np.round(scales[best], 6)) == plant
    E64 = gs.mirror_score(base, states, controls, 0.05, scales)
    assert int(np.argmin(E64)) == best
    excess = np.abs(E.astype(np.float64) - E64) - (E_RTOL * E64 + E_ATOL)
    assert np.all(excess <= 0.0), "worst: %.3g over the tolerance at hypothesis %d" % (excess.max(), int(np.argmax(excess)))


def test_the_vectorised_mirror_is_predict_next_state():
    """grip_spec.mirror_score is DynamicBicycleParams.predict_next_state hypothesis by hypothesis, to the last bit or two of
    the float64 sum (the array and the scalar forms associate F * dt alike; ** 2 against * may differ in an ulp)."""
    base = _base()
    states, controls = _log((0.5, 0.7), 0.02)
    scales = np.array([[0.5, 0.7], [1.0, 1.0], [0.3, 1.5]])
    E64 = gs.mirror_score(base, states, controls, 0.05, scales, segment=8)
    for (f, r), got in zip(scales, E64):
        v = base.with_axle_grip(f, r)
        want = 0.0
        for j0 in range(0, 40, 8):
            x = np.concatenate([np.zeros(3), states[j0].astype(np.float64)])
            for j in range(j0, j0 + 8):
                x = v.predict_next_state(x, controls[j].astype(np.float64), 0.05)[0]
                x[3] = max(x[3], 0.0)
                want += float(np.sum((x[3:] - states[j + 1]) ** 2))
        assert got == pytest.approx(want, rel=1e-9, abs=1e-20)


def test_a_straight_line_scores_every_hypothesis_equal_and_is_not_accepted():
    from acmpc_amd import GripEstimator
    base, scales = _base(), _split_scales()
    states, controls = gs.steering_log(base.with_grip(0.5), 0.0)
    E, best = gs.score(base.coefficients(), states, controls, 0.05, scales)
    assert best == 0 and np.all(E == E[0])
    est = GripEstimator(lambda x, u, dt, sc, segment=1, weights=(1, 1, 1):
                        gs.score(base.coefficients(), x, u, dt, sc, segment, weights), grid=GRID, axles="split")
    for j in range(41):
        est.push(states[j], controls[j - 1] if j else None)
    got = est.estimate()
    assert not got.accepted and got.front is None and got.rear is None


def test_the_acceptance_defaults_come_from_the_mirror():
    """contrast = 0.25 and floor = 1e-6, re-derived: on the excited logs - clean and with the table's noise - the gap
    median(E) - E_best clears max(contrast E_best, floor) by a wide margin, on the straight it is exactly 0; and 1e-6 sits
    between what rounding leaves at the true hypothesis (< 1e-10) and the gap to its grid neighbour (> 1e-4)."""
    from acmpc_amd.grip_estimator import grip_scales
    base = _base()
    tied = grip_scales(0.3 + 0.025 * np.arange(49), "tied")
    clean = gs.mirror_score(base, *gs.steering_log(base.with_grip(0.5), 0.02), 0.05, tied)
    assert tied[np.argmin(clean), 0] == 0.5 and clean.min() < 1e-10 < 1e-6 < 1e-4 < np.sort(clean)[1]
    assert np.median(clean) - clean.min() > 1.0
    noisy_log = gs.steering_log(base.with_grip(0.5), 0.02, noise=NOISE)
    noisy = gs.mirror_score(base, *noisy_log, 0.05, tied)
    assert abs(tied[np.argmin(noisy), 0] - 0.5) <= 0.025 + 1e-12
    assert (np.median(noisy) - noisy.min()) / noisy.min() > 16 * 0.25       # measured 4.18: sixteen times the bar
    flat = gs.mirror_score(base, *gs.steering_log(base.with_grip(0.5), 0.0), 0.05, tied)
    assert np.median(flat) - flat.min() == 0.0
    for plant in PLANTS:
        E = gs.mirror_score(base, *_log(plant, 0.005), 0.05, _split_scales())
        assert E.min() < 1e-10 and np.sort(E)[1] > 1e-4


def test_a_window_shorter_than_min_window_is_not_accepted():
    from acmpc_amd import GripEstimator
    base = _base()
    states, controls = _log((0.5, 0.7), 0.02)
    est = GripEstimator(lambda x, u, dt, sc, segment=1, weights=(1, 1, 1):
                        gs.score(base.coefficients(), x, u, dt, sc, segment, weights), grid=GRID, axles="split")
    for j in range(10):                      # 9 transitions
        est.push(states[j], controls[j - 1] if j else None)
    got = est.estimate()
    assert est.transitions == 9 and not got.accepted and got.front is None
    assert np.isfinite(got.error) and got.errors.shape == (625,)
    est.push(states[10], controls[9])        # the tenth
    got = est.estimate()
    assert got.accepted and (round(got.front, 6), round(got.rear, 6)) == (0.5, 0.7)


def test_with_noise_an_eight_step_segment_is_within_a_grid_step():
    from acmpc_amd.grip_estimator import grip_scales
    base = _base()
    tied = grip_scales(0.3 + 0.025 * np.arange(49), "tied")
    states, controls = gs.steering_log(base.with_grip(0.5), 0.02, noise=NOISE)
    E, best = gs.score(base.coefficients(), states, controls, 0.05, tied, segment=8)
    assert abs(tied[best, 0] - 0.5) <= 0.025 + 1e-12
    assert np.median(E) - E[best] > max(0.25 * E[best], 1e-6)


def test_hypothesis_one_one_is_vehicle_zero_bit_for_bit():
    base = _base()
    for block in (base.coefficients(), base.with_axle_grip(0.37, 1.21).coefficients()):
        k0 = ds.derived_constants(block)
        k = gs.hypothesis_constants(block, [[1.0, 1.0], [0.5, 0.7]], 0.05).k
        for name, value in k0.items():
            got = k[name][0] if name in ("Pf", "Pr") else k[name]
            assert np.float32(got).tobytes() == np.float32(value).tobytes(), name
        scaled = ds.derived_constants(gs.hypothesis_block(block, 0.5, 0.7))
        assert k["Pf"][1] == scaled["Pf"] and k["Pr"][1] == scaled["Pr"]
    E_a, _ = gs.score(base.coefficients(), *_log((1.0, 1.0), 0.02), 0.05, [[1.0, 1.0]], segment=40)
    # (1, 1) rolls dynamic_spec's own step under vehicle 0: the spec's open-loop states, compared by hand
    c0 = ds.constants(base.coefficients(), dt=0.05)
    states, controls = _log((1.0, 1.0), 0.02)
    st = tuple(np.float32(v) for v in (0, 0, 0, *states[0]))
    e = np.float32(0)
    for j in range(40):
        st = ds.dynamic_step(st, controls[j, 0], controls[j, 1], c0)
        for q in range(3):
            d = st[3 + q] - states[j + 1, q]
            e = gs.fma32(np.float32(1) * d, d, e)
    assert np.float32(e).tobytes() == E_a[0].tobytes()


def test_with_grip_is_with_axle_grip_on_both_axles():
    base = _base()
    for s in (0.3, 0.5, 1.0, 1.37):
        assert np.array_equal(base.with_grip(s).coefficients(), base.with_axle_grip(s, s).coefficients())
    split = base.with_axle_grip(0.5, 0.7)
    assert split.Df == base.Df * 0.5 and split.Dr == base.Dr * 0.7 and split.Bf == base.Bf
    for bad in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            base.with_axle_grip(*bad)


def test_every_refusal_comes_before_any_device_work():
    """acmpc_score_grips refuses a bad call on the host: the codes are the same with or without a GPU, and on a box
    without one a good call is the first to reach the device (ENODEVICE)."""
    import ctypes as C
    import torch
    from acmpc_amd import Engine, EngineError, _capi

    def engine(mode=_capi.MODE_DYNAMIC):
        return Engine(mode=mode, max_problems=1, max_candidates=8, max_steps=4, step_cost=(1, 1, 0), r_term=(1, 1),
                      final_cost=(1, 1, 0), u_min=(-0.3, -1), u_max=(0.3, 1), margin=0.0, wheelbase=2.9)

    x = np.zeros((5, 3), dtype=np.float32)
    x[:, 0] = 20.0
    u = np.zeros((4, 2), dtype=np.float32)
    one = np.ones((1, 2))

    def code(eng, states=x, controls=u, dt=0.05, scales=one, **kw):
        with pytest.raises(EngineError) as refused:
            eng.score_grips(states, controls, dt, scales, **kw)
        return refused.value.code

    assert code(engine(_capi.MODE_TEMPORAL)) == _capi.ESTATE        # not mode D
    eng = engine()
    assert code(eng) == _capi.ESTATE                                # mode D without a vehicle
    eng.set_dynamics(_base())
    for dt in (0.0, -0.05, float("nan"), float("inf")):
        assert code(eng, dt=dt) == _capi.EINVAL
    for segment in (0, -1, 5):
        assert code(eng, segment=segment) == _capi.EINVAL
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for column in (0, 1):
            scales = np.ones((3, 2))
            scales[2, column] = bad
            assert code(eng, scales=scales) == _capi.EINVAL
    for weights in ((0, 0, 0), (1, -1, 1), (1, float("nan"), 1), (float("inf"), 1, 1), (1e39, 1, 1)):
        assert code(eng, weights=weights) == _capi.EINVAL
    assert code(eng, scales=np.ones((0, 2))) == _capi.EINVAL        # K = 0
    long_x = np.zeros((514, 3), dtype=np.float32)
    assert code(eng, states=long_x, controls=np.zeros((513, 2), dtype=np.float32)) == _capi.EINVAL   # W > 512
    assert code(eng, scales=np.ones((65537, 2))) == _capi.ECAPACITY
    wide = np.zeros((513, 3), dtype=np.float32)                     # S K = 512 x 8193 > 2^22
    assert code(eng, states=wide, controls=np.zeros((512, 2), dtype=np.float32), scales=np.ones((8193, 2))) == _capi.ECAPACITY
    # one segment more than fits under the largest K: S K = 2^22 + K; S K = 2^22 itself is a good call
    full = np.ones((65536, 2))
    assert code(eng, states=wide[:66], controls=np.zeros((65, 2), dtype=np.float32), scales=full) == _capi.ECAPACITY
    if not torch.cuda.is_available():
        assert code(eng, states=wide[:65], controls=np.zeros((64, 2), dtype=np.float32), scales=full) == _capi.ENODEVICE
    # null pointers, W = 0 and a null handle: the raw call
    lib = _capi.load_library()
    w3, best = np.ones(3), C.c_int64(0)
    args = dict(states=x.ctypes.data, controls=u.ctypes.data, weights=w3.ctypes.data, scales=one.ctypes.data, best=C.byref(best))
    for name in args:
        a = dict(args, **{name: None})
        assert lib.acmpc_score_grips(eng._ctx, a["states"], a["controls"], 4, 0.05, 1, a["weights"], a["scales"], 1, None,
                                     a["best"]) == _capi.EINVAL, name
    assert lib.acmpc_score_grips(eng._ctx, x.ctypes.data, u.ctypes.data, 0, 0.05, 1, w3.ctypes.data, one.ctypes.data, 1, None,
                                 C.byref(best)) == _capi.EINVAL
    assert lib.acmpc_score_grips(None, x.ctypes.data, u.ctypes.data, 4, 0.05, 1, w3.ctypes.data, one.ctypes.data, 1, None,
                                 C.byref(best)) == _capi.EINVAL
    with pytest.raises(ValueError):
        eng.score_grips(x, u[:3], 0.05, one)                        # states and controls of different logs
    if not torch.cuda.is_available():
        assert code(eng) == _capi.ENODEVICE
    eng.close()


def test_the_grid_of_a_scoring_launch_as_literal_numbers():
    """`acmpc_describe_score_grips` answers from the function the launcher asks (csrc: identify_grid), so these are the sizes at
    which acmpc_score_grips starts to give a workgroup a run of segments, and how ragged the last run is.  Fixed here on
    purpose: whoever changes the rule moves the cases of tests/test_gpu_grip_identification.py, which run them on the
    device, with it."""
    from acmpc_amd import Engine, EngineError, _capi

    def engine(mode=_capi.MODE_DYNAMIC):
        return Engine(mode=mode, max_problems=1, max_candidates=8, max_steps=4, step_cost=(1, 1, 0), r_term=(1, 1),
                      final_cost=(1, 1, 0), u_min=(-0.3, -1), u_max=(0.3, 1), margin=0.0, wheelbase=2.9)

    eng = engine()
    eng.set_dynamics(_base())

    def grid(W, L, K):
        d = eng.describe_score_grips(W, L, K)
        # what the numbers mean: every segment in exactly one run, every run but the last full
        assert d["segments"] == -(-W // L) and d["blocks"] == -(-K // 256) and d["rows"] == min(d["segments"], max(1, 2048 // d["blocks"]))
        assert (d["grid_y"] - 1) * d["run"] + d["last_run"] == d["segments"] and 1 <= d["last_run"] <= d["run"]
        assert (d["segments"] - 1) * L + d["last_segment"] == W and 1 <= d["last_segment"] <= L
        return d["segments"], d["blocks"], d["rows"], d["run"], d["grid_y"], d["last_run"], d["last_segment"]

    # every shape under test before these had run = 1
    for W, L, K in ((1, 1, 1), (5, 1, 3), (7, 3, 65), (33, 8, 257), (12, 12, 64), (40, 1, 625), (512, 512, 2), (512, 1, 2), (40, 8, 625)):
        assert grid(W, L, K)[3:6] == (1, -(-W // L), 1), (W, L, K)
    assert grid(7, 3, 65) == (3, 1, 3, 1, 3, 1, 1) and grid(33, 8, 257) == (5, 2, 5, 1, 5, 1, 1)
    # run = 1 up to 1 024 hypotheses whatever the log; one hypothesis more and 512 segments go in runs of 2
    assert grid(512, 1, 1024) == (512, 4, 512, 1, 512, 1, 1)
    assert grid(512, 1, 1025) == (512, 5, 409, 2, 256, 2, 1)
    assert grid(511, 1, 1025) == (511, 5, 409, 2, 256, 1, 1)          # a last run of one segment
    assert grid(409, 1, 1025) == (409, 5, 409, 1, 409, 1, 1) and grid(410, 1, 1025) == (410, 5, 409, 2, 205, 2, 1)
    # 10 workgroups along the hypotheses: 204 runs aimed at
    assert grid(204, 1, 2305) == (204, 10, 204, 1, 204, 1, 1)
    assert grid(205, 1, 2305) == (205, 10, 204, 2, 103, 1, 1)
    assert grid(409, 2, 2305) == (205, 10, 204, 2, 103, 1, 1)          # ... whose one segment has one step
    assert grid(408, 1, 2305) == (408, 10, 204, 2, 204, 2, 1)
    assert grid(409, 1, 2305) == (409, 10, 204, 3, 137, 1, 1)          # runs of 3, the last ragged
    # 65 and 256 partial keys for identify_best_kernel's 64 lanes; the limits K = 65 536, S K = 2^22
    assert grid(5, 2, 16384) == (3, 64, 3, 1, 3, 1, 1) and grid(5, 2, 16385) == (3, 65, 3, 1, 3, 1, 1)
    assert grid(64, 1, 16384) == (64, 64, 32, 2, 32, 2, 1)
    assert grid(64, 1, 65536) == (64, 256, 8, 8, 8, 8, 1)
    assert grid(64, 1, 1024) == (64, 4, 64, 1, 64, 1, 1)
    assert grid(63, 1, 65536) == (63, 256, 8, 8, 8, 7, 1) and grid(57, 1, 65536) == (57, 256, 8, 8, 8, 1, 1)
    assert grid(512, 1, 8192) == (512, 32, 64, 8, 64, 8, 1)

    # it refuses what acmpc_score_grips refuses of a shape, with its codes
    def code(e, *shape):
        with pytest.raises(EngineError) as refused:
            e.describe_score_grips(*shape)
        return refused.value.code

    assert code(engine(_capi.MODE_TEMPORAL), 4, 1, 1) == _capi.ESTATE
    assert code(engine(), 4, 1, 1) == _capi.ESTATE                        # mode D without a vehicle
    for shape in ((0, 1, 1), (513, 1, 1), (4, 0, 1), (4, -1, 1), (4, 5, 1), (4, 1, 0)):
        assert code(eng, *shape) == _capi.EINVAL, shape
    for shape in ((4, 1, 65537), (512, 1, 8193), (65, 1, 65536)):
        assert code(eng, *shape) == _capi.ECAPACITY, shape
    lib = _capi.load_library()
    assert lib.acmpc_describe_score_grips(eng._ctx, 4, 1, 1, None) == _capi.EINVAL
    assert lib.acmpc_describe_score_grips(None, 4, 1, 1, None) == _capi.EINVAL
    eng.close()


def _table_scorer(table):
    """A scoring function that ignores the log: errors from `table`, a list consumed call by call."""
    calls = []

    def score(states, controls, dt, scales, segment=1, weights=(1.0, 1.0, 1.0)):
        calls.append((np.array(states), np.array(controls), dt, np.array(scales), segment))
        errors = np.asarray(table[min(len(calls), len(table)) - 1], dtype=np.float32)
        keys = [(np.float32(np.inf) if not np.isfinite(e) else e, k) for k, e in enumerate(errors)]
        return errors, min(keys)[1]

    return score, calls


def test_estimator_window_rolls_over():
    from acmpc_amd import GripEstimator
    score, calls = _table_scorer([[3.0, 1.0, 3.0]])
    est = GripEstimator(score, grid=(0.4, 0.5, 0.6), window=4, min_window=2, dt=0.02, segment=3)
    assert est.estimate().errors is None and not calls                  # nothing held: nothing scored
    for j in range(7):
        est.push([0, 0, 0, 10.0 + j, 0.1 * j, 0.01 * j], None if j == 0 else (0.001 * j, 0.2))
    got = est.estimate()
    states, controls, dt, scales, segment = calls[-1]
    assert states.shape == (5, 3) and controls.shape == (4, 2) and dt == 0.02 and segment == 3
    assert states.dtype == np.float32 and list(states[:, 0]) == [12.0, 13.0, 14.0, 15.0, 16.0]      # the last 4 + 1
    np.testing.assert_array_equal(controls[:, 0], np.float32([0.003, 0.004, 0.005, 0.006]))      # control j leads to state j
    assert got.accepted and got.front == got.rear == 0.5 and got.error == 1.0
    est3 = GripEstimator(score, grid=(0.4, 0.5, 0.6), window=4, min_window=1, segment=3)
    est3.push([10.0, 0.0, 0.0])                                         # 3-state input
    est3.push([10.0, 0.0, 0.0], (0.0, 0.0))
    est3.estimate()
    assert calls[-1][4] == 1                                            # a segment never exceeds the held transitions
    with pytest.raises(ValueError):
        est3.push([10.0, 0.0, 0.0])                                     # no control


def test_estimator_ties_go_to_the_lower_index_and_an_unaccepted_call_keeps_the_estimate():
    from acmpc_amd import GripEstimator
    nan = float("nan")
    table = [[5.0, 1.0, 1.0, 5.0, 5.0],        # a tie between 1 and 2: the lower index
             [2.0, 2.0, 2.0, 2.0, 2.0],        # all equal: nothing to tell apart
             [nan, nan, nan, nan, nan],        # a NaN in the log
             [1.0, 1.0, 0.9, 1.0, 1.0],        # a best without contrast: 1.0 - 0.9 < 0.25 * 0.9
             [9.0, 9.0, 9.0, 9.0, 1.0]]
    score, _ = _table_scorer(table)
    est = GripEstimator(score, grid=(0.4, 0.5, 0.6, 0.7, 0.8), min_window=1)
    est.push([10.0, 0.0, 0.0])
    est.push([10.0, 0.0, 0.0], (0.0, 0.0))
    got = est.estimate()
    assert got.accepted and got.front == 0.5
    for _ in range(3):
        got = est.estimate()
        assert not got.accepted and got.front == got.rear == 0.5       # the previous accepted estimate stays
    got = est.estimate()
    assert got.accepted and got.front == 0.8 and got.error == 1.0


def test_estimator_axles():
    from acmpc_amd import GripEstimator
    from acmpc_amd.grip_estimator import grip_scales
    tied = GripEstimator(lambda *a, **k: None, grid=GRID, axles="tied").scales
    assert tied.shape == (25, 2) and np.array_equal(tied[:, 0], tied[:, 1]) and np.array_equal(tied[:, 0], GRID)
    split = grip_scales(GRID, "split")
    assert split.shape == (625, 2) and tuple(split[1]) == (GRID[0], GRID[1]) and tuple(split[25]) == (GRID[1], GRID[0])
    assert GripEstimator(lambda *a, **k: None, grid=GRID).grid_step == pytest.approx(0.05)
    for bad in ((), (0.5, -1.0), (float("nan"),)):
        with pytest.raises(ValueError):
            grip_scales(bad)
    with pytest.raises(ValueError):
        grip_scales(GRID, "both")


def test_grip_adapt_excludes_the_ensemble_keys():
    from acmpc_amd import DynamicSamplingSolver
    for other in (dict(grip_ensemble=(0.4, 0.6)), dict(vehicle_ensemble=[_base()])):
        with pytest.raises(ValueError, match="mutually exclusive"):
            DynamicSamplingSolver(dict(horizon=10, grip_adapt=dict(axles="tied"), **other))
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(horizon=10, grip_adapt=dict(brackets=(0.8, 1.2))))      # an unknown key
    with pytest.raises(ValueError):
        DynamicSamplingSolver(dict(horizon=10, grip_adapt=dict(bracket=(0.8, -1.2))))
    solver = DynamicSamplingSolver(dict(horizon=10, n_candidates=8, grip_adapt=dict(axles="tied")))    # no device work
    assert solver.grip.front is None and not solver.grip.accepted
    solver.close()
