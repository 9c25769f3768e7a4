"""The device-resident particle filter against its restatements: the step (Philox control noise + kinematic step) against
`oracle.pf_step_counter_based`, every update of consecutive cycles against `oracle.pf_resample_counter_based`, the estimate
against the float64 reference (tests/pf_reference64.py) - with a seed whose high word is not zero, at the counts where the
kernels change path (one workgroup below a capacity of 8 192, tiles of 1 024 particles from there; 4 096 particles in the
host-pointer advance) and through the branches a tracking run never takes: uniform weights, more valid particles than
wanted, more wanted than the capacity, exactly the minimum of valid particles."""
import numpy as np
import pytest

import acmpc_oracle as orc
import pf_reference64 as ref64
from test_gpu_particle_filter import LOCALISATION, _scene

pytestmark = pytest.mark.gpu

SEED = 0x0000_1234_5678_9ABC                       # the high word takes part in the key
WHEELBASE = 2.65
STEP_TOLERANCE = dict(rtol=2e-6, atol=2e-5)       # the project's tolerance of the advance (test_advance_and_estimate_...)
CONTROL = dict(velocity=0.25, yaw=2.0)
SIGMA_YAW, SIGMA_V = 2.0 * np.pi / 180, 0.25


def _config(capacity, n_converged=None, **extra):
    cfg = dict(LOCALISATION, n_particles=capacity, n_converged_particles=capacity if n_converged is None else n_converged,
               sampling_noise=dict(x=1.1, y=1.1, yaw=3.0), control_noise=dict(CONTROL),
               convergence_criteria=dict(maximum_distance=50, maximum_angle=90))
    cfg.update(extra)
    return cfg


def _filter(cfg, track, seed=SEED):
    from acmpc_amd.particle_filter import DeviceParticleFilter
    return DeviceParticleFilter(cfg, track, seed=seed)


def _uniform(n):
    return np.full(n, 1.0 / n, dtype=np.float32)


def _sampling_sigma(cfg):
    noise = cfg["sampling_noise"]
    return (float(noise["x"]), float(noise["y"]), float(noise["yaw"]) * np.pi / 180)


def _check_step(got, before, tyre, velocity, dt, counter, seed=SEED, sigma=(SIGMA_YAW, SIGMA_V), label=""):
    want = orc.pf_step_counter_based(before, tyre, velocity, dt, sigma[0], sigma[1], WHEELBASE, seed, counter)
    print("pf-filter step %s n=%d counter=%d: largest |device - restatement| %.3e (x, y) %.3e (yaw)"
          % (label, len(before), counter, np.abs(got[:, :2] - want[:, :2]).max(), np.abs(got[:, 2] - want[:, 2]).max()))
    np.testing.assert_allclose(got, want, **STEP_TOLERANCE)
    return want


def _check_update(cfg, track, before, obs, out, got, counter, n_desired, seed=SEED):
    """One update of the device against the restatement, exactly: `before` are the particles downloaded in front of it,
    scored through the host-pointer seam (held to the reference elsewhere).  Returns (scoring, picked indices)."""
    from acmpc_amd.particle_filter import ParticleScorer
    scorer = ParticleScorer(cfg, track)
    scored = scorer.update_particles(before, scorer.downsample_observations(obs))
    scorer.close()
    capacity = cfg["n_particles"]
    want = orc.pf_resample_counter_based(before, scored["score"].astype(np.float32), scored["score"], scored["valid_mask"],
                                         min(n_desired, capacity), cfg["thresholds"]["minimum_particles"],
                                         _sampling_sigma(cfg), seed, counter)
    assert want is not None and not out["was_reset"]
    want_states, want_scores, picked = want
    got_states, got_scores = got
    n_valid = int(scored["valid_mask"].sum())
    assert out["n_valid"] == n_valid
    assert out["n_particles"] == want_states.shape[0] == got_states.shape[0] == max(n_valid, min(n_desired, capacity))
    np.testing.assert_array_equal(got_states[:n_valid], want_states[:n_valid])          # kept, in order
    np.testing.assert_array_equal(got_scores, want_scores)                                # the scores follow the picks
    np.testing.assert_array_equal(got_states[n_valid:], want_states[n_valid:])          # fresh particles: picks and noise
    return scored, picked


def _check_estimate(out, got):
    """The update's estimate against the float64 reference on the particles it left behind."""
    states, scores = got
    est, max_d, max_a = ref64.estimate(scores, states)
    np.testing.assert_allclose(out["estimate"], est, rtol=0, atol=1e-10 * np.abs(est).max())
    np.testing.assert_allclose([out["max_distance"], out["max_angle"]], [max_d, max_a], rtol=1e-9)


# ---- 1. the step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,n", [(1, 1), (255, 255), (256, 256), (257, 257), (300, 300), (8192, 2049)])
def test_step_matches_its_restatement(golden, capacity, n):
    """Two steps (counters 1 and 2) with control noise of 2 degrees and 0.25 m/s over dt = 0.5 s at 30 m/s: the noise moves
    a particle by some 0.125 m and 0.2 rad, the tolerance is 5e-4 m - a wrong word, z0 for z1, degrees for radians or a
    seed half left out are hundreds of tolerances."""
    track, states, _, _, _ = _scene(golden, n)
    pf = _filter(_config(capacity), track)
    pf.set_particles(states, _uniform(n))
    tyre, velocity, dt = 0.03, 30.0, 0.5
    pf.step(tyre, velocity, dt)
    first, scores = pf.particles()
    assert first.shape == (n, 3)
    np.testing.assert_array_equal(scores, _uniform(n))
    want = _check_step(first, states, tyre, velocity, dt, 1)
    # (the draws matter at this tolerance: without them the restatement is somewhere else)
    quiet = ref64.filter_step(states, tyre, velocity, dt, 0.0, 0.0, WHEELBASE, SEED, 1)
    assert n == 1 or np.abs(want - quiet).max() > 100 * (STEP_TOLERANCE["atol"] + STEP_TOLERANCE["rtol"] * np.abs(want).max())
    pf.step(tyre, velocity, dt)
    _check_step(pf.particles()[0], first, tyre, velocity, dt, 2)


def test_step_uses_both_halves_of_the_seed(golden):
    track, states, _, _, _ = _scene(golden, 300)
    seen = []
    for seed in (SEED, SEED + 2**32, SEED & 0xFFFFFFFF):
        pf = _filter(_config(300), track, seed=seed)
        pf.set_particles(states, _uniform(300))
        pf.step(0.03, 30.0, 0.5)
        seen.append(pf.particles()[0])
        _check_step(seen[-1], states, 0.03, 30.0, 0.5, 1, seed=seed, label="seed %#x" % seed)
    for a in range(3):
        for b in range(a + 1, 3):
            assert np.abs(seen[a] - seen[b]).max() > 0.05


def test_step_without_noise_is_the_advance(golden):
    """Both sigmas 0: the kinematic step of `ParticleScorer.advance_particles` under one control for all, to one float32
    ulp per component."""
    track, states, _, _, _ = _scene(golden, 300)
    pf = _filter(_config(300, control_noise=dict(velocity=0.0, yaw=0.0)), track)
    pf.set_particles(states, _uniform(300))
    pf.step(0.03, 30.0, 0.5)
    got = pf.particles()[0]
    want = pf.scorer.advance_particles(states, np.full(300, 0.03), np.full(300, 30.0), 0.5)
    assert (np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all()
    _check_step(got, states, 0.03, 30.0, 0.5, 1, sigma=(0.0, 0.0), label="no noise")


def test_step_takes_the_absolute_speed(golden):
    """velocity = -0.1 m/s under noise of 0.25 m/s: velocity + noise comes out on either side of zero, the particle moves
    FORWARD by its magnitude."""
    track, states, _, _, _ = _scene(golden, 300)
    _, z1 = orc.pf_control_normals(300, SEED, 1)
    raw = -0.1 + SIGMA_V * z1.astype(np.float64)
    assert (raw > 0.02).sum() > 60 and (raw < -0.02).sum() > 60
    pf = _filter(_config(300), track)
    pf.set_particles(states, _uniform(300))
    pf.step(0.03, -0.1, 0.5)
    got = pf.particles()[0]
    _check_step(got, states, 0.03, -0.1, 0.5, 1, label="slow")
    moved = got.astype(np.float64) - states
    along = moved[:, 0] * np.cos(states[:, 2].astype(np.float64)) + moved[:, 1] * np.sin(states[:, 2].astype(np.float64))
    assert (along[np.abs(raw) > 0.02] > 0).all()       # (0.02 m/s over 0.5 s: 0.01 m, far above a float32 ulp at 250 m)


# ---- 2. consecutive cycles -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,n_converged", [(300, 295), (8192, 8000)])
def test_three_cycles_match_their_restatements(golden, capacity, n_converged):
    """step, update, step, update, step, update with counters 1, 2, 3: in front of every call the particles are
    downloaded, the step is predicted by its restatement and the update - from the downloaded post-step particles - by
    its own, exactly.  A third of the first particles starts off the track and fresh particles get a yaw noise of 40
    degrees, of which the next step carries a part off the track: every update has valid particles to keep, invalid ones
    to drop and fresh ones to draw.  The desired count is the capacity until the filter has converged, then
    `n_converged_particles`."""
    track, states, _, idx, heading = _scene(golden, capacity)
    states[1::3, :2] += 40.0
    centre, left, right = track["centre"], track["left"], track["right"]
    M = len(centre)
    cfg = _config(capacity, n_converged, sampling_noise=dict(x=1.1, y=1.1, yaw=40.0))
    pf = _filter(cfg, track)
    pf.set_particles(states, _uniform(capacity))
    rng = np.random.default_rng(12)
    spacing = float(np.mean(np.linalg.norm(np.diff(centre, axis=0), axis=1)))
    hop, dt = 36, 0.5
    speed = hop * spacing / dt

    def observe(t, count, at, yaw):
        a = np.pi / 2 - yaw
        rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        return ((t[(at + np.arange(count)) % M] - centre[at]) @ rot.T + rng.normal(0, 0.15, (count, 2))).astype(np.float32)

    assert not pf.is_converged
    for k in (1, 2, 3):
        before = pf.particles()[0]
        yaw_rate = (heading[(idx + hop) % M] - heading[idx]) / dt
        tyre = float(np.arctan(yaw_rate * WHEELBASE / speed))
        pf.step(tyre, speed, dt)
        stepped = pf.particles()[0]
        _check_step(stepped, before, tyre, speed, dt, k, label="cycle")
        idx = (idx + hop) % M
        obs = {"left": observe(left, 230, idx, heading[idx]), "right": observe(right, 210, idx, heading[idx])}
        n_desired = n_converged if pf.is_converged else capacity
        assert n_desired == (capacity if k == 1 else n_converged)
        out = pf.update(obs)
        got = pf.particles()
        scored, picked = _check_update(cfg, track, stepped, obs, out, got, k, n_desired)
        n_valid = int(scored["valid_mask"].sum())
        print("pf-filter cycle %d capacity %d: %d live, %d valid, %d wanted, %d drawn" % (k, capacity, len(stepped), n_valid,
                                                                                        n_desired, len(picked)))
        assert 20 < n_valid < len(stepped) and len(picked) > 0 and len(np.unique(picked)) > 1
        _check_estimate(out, got)
        assert pf.is_converged


# ---- 3. uniform weights ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean,what", [(-10.0, "zero"), (0.0, "nan")])
@pytest.mark.parametrize("capacity", [300, 8192])
def test_uniform_weights_when_no_score_counts(golden, capacity, mean, what):
    """score_distribution.sigma = 0.001: the density of every particle's error underflows to 0.0 while the particles stay
    valid - the weights' total is 0 and the picks are uniform (localiser.py:523-526), in the one-workgroup kernel and in
    the tiled plan.  With the mean at -10 (a point of the normaliser's grid) the scores are 0.0; with the mean at 0 the
    normaliser underflows as well and they are 0 / 0.  Either way every published score is useless as a weight, so the
    estimate is the plain mean of the new particles: the NaN fallback (the tiled one at 8 192)."""
    from acmpc_amd.particle_filter import ParticleScorer
    track, states, obs, _, _ = _scene(golden, capacity)
    cfg = _config(capacity, score_distribution=dict(mean=mean, sigma=0.001))
    scorer = ParticleScorer(cfg, track)
    scored = scorer.update_particles(states, scorer.downsample_observations(obs))
    scorer.close()
    if what == "zero":
        assert (scored["score"] == 0.0).all()
    else:
        assert np.isnan(scored["score"]).all()
    n_valid = int(scored["valid_mask"].sum())
    assert cfg["thresholds"]["minimum_particles"] <= n_valid < capacity
    assert sum(orc.pf_weights_fixed_point(scored["score"][scored["valid_mask"]])) == 0       # the restatement's [1] * n_valid
    pf = _filter(cfg, track)
    pf.set_particles(states, _uniform(capacity))
    out = pf.update(obs)
    got = pf.particles()
    _, picked = _check_update(cfg, track, states, obs, out, got, 1, capacity)
    # uniform picks: (word * n_valid) >> 64 over the kept particles
    assert len(picked) == capacity - n_valid and len(np.unique(picked)) > min(len(picked), n_valid) // 3
    if what == "zero":
        assert (got[1] == 0.0).all()
    else:
        assert np.isnan(got[1]).all()
    plain = got[0].astype(np.float64).mean(axis=0)
    np.testing.assert_allclose(out["estimate"], plain, rtol=0, atol=1e-10 * np.abs(plain).max())
    _check_estimate(out, got)


# ---- 4. counts ---------------------------------------------------------------------------------------------------------------
def test_more_valid_particles_than_wanted(golden):
    """n_converged_particles = 200 at a capacity of 300: once converged, an update that finds more than 200 valid particles
    keeps them all and draws nothing."""
    track, states, obs, _, _ = _scene(golden, 300)
    cfg = _config(300, 200)
    pf = _filter(cfg, track)
    pf.set_particles(states, _uniform(300))
    out = pf.update(obs)
    assert pf.is_converged and out["n_particles"] == 300 and out["n_valid"] < 300
    before = pf.particles()[0]
    out = pf.update(obs)
    got = pf.particles()
    _, picked = _check_update(cfg, track, before, obs, out, got, 2, 200)
    assert len(picked) == 0 and out["n_particles"] == out["n_valid"] > 200
    _check_estimate(out, got)


def test_more_particles_wanted_than_the_capacity(golden):
    """n_converged_particles = 400 at a capacity of 300: capped."""
    track, states, obs, _, _ = _scene(golden, 300)
    cfg = _config(300, 400)
    pf = _filter(cfg, track)
    pf.set_particles(states, _uniform(300))
    pf.update(obs)
    assert pf.is_converged
    pf.set_particles(states, _uniform(300))                 # some off the track again: something to draw
    out = pf.update(obs)
    got = pf.particles()
    _, picked = _check_update(cfg, track, states, obs, out, got, 2, 400)
    assert out["n_particles"] == 300 and len(picked) == 300 - out["n_valid"] > 0


@pytest.mark.parametrize("capacity", [300, 8192])
def test_reset_below_the_minimum_of_valid_particles(golden, capacity):
    """Exactly `minimum_particles` (20) particles near the track and the rest 500 m off: no reset.  With 19: the reset along
    the centre line, the reference's own."""
    from acmpc_amd.particle_filter import ParticleScorer
    track, states, obs, _, _ = _scene(golden, capacity)
    cfg = _config(capacity)
    minimum = cfg["thresholds"]["minimum_particles"]
    scorer = ParticleScorer(cfg, track)
    good = np.flatnonzero(scorer.update_particles(states, scorer.downsample_observations(obs))["valid_mask"])
    for keep in (minimum, minimum - 1):
        far = states.copy()
        far[:, :2] += 500.0
        stay = good[np.linspace(0, len(good) - 1, keep).astype(int)]       # spread over the tiles
        far[stay] = states[stay]
        scored = scorer.update_particles(far, scorer.downsample_observations(obs))
        assert int(scored["valid_mask"].sum()) == keep
        pf = _filter(cfg, track)
        pf.set_particles(far, _uniform(capacity))
        out = pf.update(obs)
        got = pf.particles()
        if keep == minimum:
            _check_update(cfg, track, far, obs, out, got, 1, capacity)
            np.testing.assert_array_equal(got[0][:keep], far[stay])
        else:
            want_states, want_scores = orc.pf_reset(track["centre"], capacity)
            assert out["was_reset"] and out["n_valid"] == keep and out["n_particles"] == capacity
            np.testing.assert_array_equal(got[0], want_states)
            np.testing.assert_array_equal(got[1], want_scores)
        _check_estimate(out, got)
    scorer.close()


# ---- 5. tile edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("live", [1023, 1024, 1025, 2049])
def test_live_counts_on_the_tile_edges(golden, live, monkeypatch):
    """Capacity 8 192 (the tiled kernels: tiles of 1 024 particles) with a live count on, one below and one above a tile's
    edge and two tiles plus one; every seventh particle is invalid, so the ranks of the kept ones cross the borders."""
    track, states, obs, _, _ = _scene(golden, live)
    cfg = _config(8192)
    runs = []
    for narrow in (False, True):
        if narrow:
            monkeypatch.setenv("ACMPC_PF_NARROW_FILTER", "1")
        pf = _filter(cfg, track)
        pf.set_particles(states, _uniform(live))
        out = pf.update(obs)
        got = pf.particles()
        scored, picked = _check_update(cfg, track, states, obs, out, got, 1, 8192)
        assert 0 < int((~scored["valid_mask"]).sum()) and len(picked) == 8192 - out["n_valid"]
        _check_estimate(out, got)
        runs.append((out, got))
    (wide_out, wide), (narrow_out, narrow) = runs
    np.testing.assert_array_equal(wide[0], narrow[0])
    np.testing.assert_array_equal(wide[1], narrow[1])
    assert wide_out["n_particles"] == narrow_out["n_particles"] and wide_out["n_valid"] == narrow_out["n_valid"]
    np.testing.assert_allclose(wide_out["estimate"], narrow_out["estimate"], rtol=1e-10)


# ---- 6. the host-pointer calls -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_scorer(golden):
    from acmpc_amd.particle_filter import ParticleScorer
    g = golden
    scorer = ParticleScorer(dict(LOCALISATION, n_particles=5000), dict(centre=g["pf/centre"], left=g["pf/left"], right=g["pf/right"]))
    yield scorer
    scorer.close()


@pytest.mark.parametrize("P", [1, 255, 256, 257, 4095, 4096, 4097])
def test_advance_at_the_edges_of_its_paths(host_scorer, P):
    """`acmpc_pf_advance` works in the page-locked block below 4 096 particles and through device buffers from there."""
    rng = np.random.default_rng(P)
    states = rng.normal(0, [200.0, 200.0, 2.0], (P, 3)).astype(np.float32)
    delta = rng.normal(0, 0.1, P).astype(np.float32)
    velocity = np.abs(rng.normal(30, 10, P)).astype(np.float32)
    got = host_scorer.advance_particles(states, delta, velocity, 0.05)
    want = ref64.kinematic_step(states, delta, velocity, 0.05, WHEELBASE)
    assert got.shape == (P, 3) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, **STEP_TOLERANCE)
    assert np.abs(want - states).max() > 100 * STEP_TOLERANCE["atol"] or P == 1


@pytest.mark.parametrize("scores", ["weights", "zeros", "one NaN"])
@pytest.mark.parametrize("P", [1, 257, 5000])
def test_estimate_against_the_float64_reference(host_scorer, P, scores):
    rng = np.random.default_rng(P)
    states = (np.array([250.0, -120.0, 1.0]) + rng.normal(0, [3.0, 3.0, 0.2], (P, 3))).astype(np.float32)
    weights = rng.uniform(0.0, 1.0, P).astype(np.float32)
    if scores == "zeros":
        weights[:] = 0.0
    elif scores == "one NaN":
        weights[P // 2] = np.nan
    est, max_d, max_a = host_scorer.estimate_location(weights, states)
    want, want_d, want_a = ref64.estimate(weights, states)
    if scores != "weights":
        np.testing.assert_allclose(want, states.astype(np.float64).mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(est, want, rtol=0, atol=1e-10 * np.abs(want).max())
    np.testing.assert_allclose([max_d, max_a], [want_d, want_a], rtol=1e-9)
