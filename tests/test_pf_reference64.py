"""The float64 statement of the particle filter (tests/pf_reference64.py) against the reference's own vectors
(tests/golden/gen_golden.py: pf/*, xdot/*, est/*) and against the oracle - on the golden map, on a loop with fewer points
than the observation has, and on polylines of 65 536 points and more, where the oracle itself used to give no answer under
NumPy 2.  CPU only: the GPU tests then hold the kernels to this reference."""
import numpy as np
import pytest

import acmpc_oracle as orc
import pf_reference64 as ref64
import pf_scenes

THRESHOLDS = pf_scenes.THRESHOLDS


def test_scoring_equals_the_reference_vectors(golden):
    g = golden
    out = ref64.score_particles(g["pf/states"], g["pf/centre"], g["pf/left"], g["pf/right"], g["pf/obs_left_downsampled"],
                                g["pf/obs_right_downsampled"], 0, 10, THRESHOLDS)
    assert abs(ref64.score_scale(0, 10) - float(g["pf/scale"])) < 1e-17
    np.testing.assert_array_equal(out["track_indices"], g["pf/track_indices"])
    np.testing.assert_allclose(out["minimum_offset"], g["pf/minimum_offset"], rtol=1e-12)
    np.testing.assert_allclose(out["heading_offset"], g["pf/heading_offset"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["observation_error"], g["pf/observation_error"], rtol=1e-5)
    np.testing.assert_allclose(out["score"], g["pf/score"], rtol=1e-5)
    np.testing.assert_array_equal(out["valid"], g["pf/valid_mask"])
    assert not out["wrapped"].any() and out["gap"].min() > 1e-9


def _agrees_with_the_oracle(scene, some, counts):
    left, right = scene.observation(counts)
    track = scene.track
    want = orc.pf_score_particles(scene.states[some], track["centre"], track["left"], track["right"], left, right,
                                  pf_scenes.SCORE_MEAN, pf_scenes.SCORE_SIGMA, THRESHOLDS)
    got = scene.reference(counts)
    np.testing.assert_array_equal(got["track_indices"][some], want["track_indices"])
    # the same float32 placement and the same float64 operations behind it, summed in another order
    np.testing.assert_allclose(got["minimum_offset"][some], want["minimum_offset"], rtol=1e-14)
    np.testing.assert_allclose(got["heading_offset"][some], want["heading_offset"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["observation_error"][some], want["observation_error"], rtol=1e-12)
    np.testing.assert_allclose(got["score"][some], want["score"], rtol=1e-9, atol=1e-300)
    np.testing.assert_array_equal(got["valid"][some], want["valid"])
    return got


@pytest.mark.parametrize("counts", [(120, 110), (0, 120), (300, 333)])
def test_scoring_equals_the_oracle_on_the_golden_map(golden, counts):
    scene = pf_scenes.scene("golden", golden)
    got = _agrees_with_the_oracle(scene, np.arange(600), counts)
    assert np.isnan(scene.states[pf_scenes.NON_FINITE, 0]) and not got["valid"][pf_scenes.NON_FINITE]
    np.testing.assert_array_equal(got["track_indices"][pf_scenes.NON_FINITE], 0)


@pytest.mark.parametrize("counts", [(120, 110), (130, 120), (300, 333)])
def test_scoring_equals_the_oracle_on_the_tiny_map(counts):
    """More observation points than the loop has map points: the indices ahead go round it, up to four times."""
    scene = pf_scenes.scene("tiny")
    got = _agrees_with_the_oracle(scene, np.arange(pf_scenes.N_PARTICLES), counts)
    for t, j in enumerate(scene.duplicates):            # the repeated points: same bits at both places, the lower index
        ties = got["gap"][:, t] == 0
        assert ties.sum() >= 20 and (got["track_indices"][ties, t] == j).all()
        assert not (got["track_indices"][:, t] == j + 3).any()


def test_scoring_equals_the_oracle_on_the_long_map():
    """Polylines of 70 000 and 65 500 points: `np.mod(uint16 indices, 70000)` is an OverflowError under NumPy 2, so the
    oracle takes the uint16 wrap and then the modulo in int64 - NumPy 1's result, and the kernels' statement.  A hundred
    and twenty-eight particles (the oracle's search holds particles x points x 2 doubles at once), half of them with a
    wrapped index."""
    scene = pf_scenes.scene("long")
    ref = scene.reference((120, 110))
    wrapped, plain = np.flatnonzero(ref["wrapped"]), np.flatnonzero(~ref["wrapped"])
    some = np.sort(np.concatenate([wrapped[:64], plain[:64]]))
    _agrees_with_the_oracle(scene, some, (120, 110))
    index = ref["track_indices"]
    assert (index[:, 0] > 65535).sum() > 500 and (index[:, 0] < 400).sum() > 250          # both sides of 65 536 and of the end
    assert ((index[:, 2] + 110 > 65535) & (index[:, 2] < 65500)).any()                    # the shorter polyline wraps too
    assert ref["valid"].sum() > 2500 and ref["wrapped"].sum() > 1000


COUNTS = [(120, 110), (200, 56), (200, 57), (0, 120), (120, 0), (300, 333)]


@pytest.mark.parametrize("name", ["golden", "long", "tiny"])
def test_the_scenes_can_be_held_to_the_reference(golden, name):
    """The preconditions of tests/test_gpu_pf_maps.py, which asserts them again before it runs anything on the device."""
    scene = pf_scenes.scene(name, golden)
    for counts in COUNTS:
        pf_scenes.check_preconditions(scene, counts)
        left, right = scene.observation(counts)
        assert (len(left), len(right)) == counts and (left[:, 1] < 50).all() and (right[:, 1] < 50).all()
    base = scene.reference((120, 110))
    assert base["valid"].sum() > 2500 and (~base["valid"]).sum() > 300


def test_the_step_equals_the_reference_vectors(golden):
    g = golden
    states, delta, velocity = g["xdot/states"], g["xdot/delta"], g["xdot/velocity"]
    wheelbase, dt = float(g["xdot/wheel_base"]), 0.0123
    want = states + g["xdot/out"] * np.float32(dt)
    got = ref64.kinematic_step(states, delta, velocity, dt, wheelbase)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-5)
    # no noise: every particle under the one control
    for i in (0, 1, len(states) - 1):
        quiet = ref64.filter_step(states, float(delta[i]), float(velocity[i]), dt, 0.0, 0.0, wheelbase, 0x123456789A, 1)
        np.testing.assert_allclose(quiet[i], want[i], rtol=2e-6, atol=2e-5)
        np.testing.assert_array_equal(quiet, ref64.kinematic_step(states, np.full(len(states), float(delta[i])),
                                                                  np.full(len(states), abs(float(velocity[i]))), dt, wheelbase))


def test_the_step_and_its_restatement_in_the_oracle():
    """`oracle.pf_step_counter_based` and `pf_reference64.filter_step` are written apart and agree; the draws are standard
    normals that depend on the particle, the step number and BOTH halves of the seed."""
    rng = np.random.default_rng(3)
    n = 4000
    states = rng.normal(0, [100.0, 100.0, 2.0], (n, 3)).astype(np.float32)
    seed = 0x0000123456789ABC
    args = (0.03, 30.0, 0.5, 2.0 * np.pi / 180, 0.25, 2.65)
    a = ref64.filter_step(states, *args, seed, 1)
    np.testing.assert_allclose(orc.pf_step_counter_based(states, *args, seed, 1), a, rtol=1e-14, atol=1e-12)
    z0, z1 = ref64.control_normals(n, seed, 1)
    o0, o1 = orc.pf_control_normals(n, seed, 1)
    np.testing.assert_array_equal(z0, o0)
    np.testing.assert_array_equal(z1, o1)
    assert z0.dtype == np.float32 and not np.array_equal(z0, z1)
    for z in (z0, z1):
        assert abs(z.mean()) < 4 / np.sqrt(n) and abs(z.std() - 1) < 0.05
    assert abs(np.corrcoef(z0, z1)[0, 1]) < 0.06
    for other in (ref64.control_normals(n, seed, 2), ref64.control_normals(n, seed + 2**32, 1),
                  ref64.control_normals(n, seed & 0xFFFFFFFF, 1), ref64.control_normals(n, seed + 1, 1)):
        assert not np.array_equal(other[0], z0) and abs(np.corrcoef(other[0], z0)[0, 1]) < 0.06
    # the noise where it belongs: the yaw moves with z0, the distance covered with |v + sigma_v z1|
    moved = a - states.astype(np.float64)
    np.testing.assert_allclose(np.hypot(moved[:, 0], moved[:, 1]), np.abs(30.0 + 0.25 * z1.astype(np.float64)) * 0.5, rtol=1e-9)
    z0_64, z1_64 = z0.astype(np.float64), z1.astype(np.float64)
    np.testing.assert_allclose(moved[:, 2], np.abs(30.0 + 0.25 * z1_64) * np.tan(0.03 + 2.0 * np.pi / 180 * z0_64) / 2.65 * 0.5,
                               rtol=1e-9, atol=1e-13)
    # a speed whose noise changes its sign: the absolute value
    slow = ref64.filter_step(states, 0.0, -0.1, 0.5, 0.0, 0.25, 2.65, seed, 1) - states.astype(np.float64)
    raw = -0.1 + 0.25 * z1.astype(np.float64)
    assert (raw > 0).sum() > n // 5 and (raw < 0).sum() > n // 5
    along = slow[:, 0] * np.cos(states[:, 2].astype(np.float64)) + slow[:, 1] * np.sin(states[:, 2].astype(np.float64))
    np.testing.assert_allclose(along, np.abs(raw) * 0.5, rtol=1e-9, atol=1e-12)
    assert (along >= 0).all()


def test_the_estimate_equals_the_reference_vectors(golden):
    g = golden
    scores, states = g["est/scores"], g["est/states"]
    est, max_d, max_a = ref64.estimate(scores, states)
    np.testing.assert_allclose(est, g["est/out"], rtol=1e-5)
    want, _ = orc.pf_convergence(scores.astype(np.float64), states.astype(np.float64), 50, np.pi / 2)
    np.testing.assert_allclose(est, want, rtol=1e-12)
    np.testing.assert_allclose(max_d, np.linalg.norm(states[:, :2].astype(np.float64) - want[:2], axis=1).max(), rtol=1e-12)
    np.testing.assert_allclose(max_a, np.abs(states[:, 2].astype(np.float64) - want[2]).max(), rtol=1e-12)
    plain = states.astype(np.float64).mean(axis=0)
    for broken in (np.zeros_like(scores), np.where(np.arange(len(scores)) == 1, np.nan, scores).astype(np.float32)):
        est, max_d, _ = ref64.estimate(broken, states)
        np.testing.assert_allclose(est, g["est/out_nan_fallback"], rtol=1e-5)
        np.testing.assert_allclose(est, plain, rtol=1e-13)
        np.testing.assert_allclose(max_d, np.linalg.norm(states[:, :2].astype(np.float64) - plain[:2], axis=1).max(), rtol=1e-12)
