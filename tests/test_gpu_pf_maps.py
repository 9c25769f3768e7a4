"""Particle scoring on maps the golden one does not stand for, every kernel form against the float64 reference
(tests/pf_reference64.py) - not against another form; equality among the forms stays in tests/test_gpu_particle_filter.py.

  golden   3 000 points per polyline
  long     70 000 / 70 000 / 65 500 points on circles of 4.3 km: nearest indices on both sides of 65 536 and of the arrays'
           ends, limits ahead that really wrap in the uint16, more than 2^20 cells of 8 m (the grid doubles its cell)
  tiny     a loop of 150 / 149 / 151 points: more observation points than map points, indices that go round several
           times, the heading's modulo m - 1 at the last index, exact ties between a point and its repeat

Forms: pf_score_kernel<1> with its own grid search (below 4 096 particles); from 4 096 up pf_nearest_kernel in front of
pf_score_given_kernel - <true, true> where no index can wrap, <true, false> where one can and the observation has at most
256 points, <false, false> beyond - or in front of pf_score_kernel<8> (ACMPC_PF_WORKGROUP_SCORE), the exhaustive scan
(ACMPC_PF_NO_GRID) and the first ring row by row (ACMPC_PF_NO_BLOCKS).  A switch is read when a handle is created: one handle
per map and switch, shared by the cases."""
import numpy as np
import pytest

import pf_reference64 as ref64
import pf_scenes

pytestmark = pytest.mark.gpu

MAPS = ("golden", "long", "tiny")
SWITCHES = (None, "ACMPC_PF_WORKGROUP_SCORE", "ACMPC_PF_NO_GRID", "ACMPC_PF_NO_BLOCKS")
BASE = (120, 110)
COUNTS = [(120, 110), (200, 56), (200, 57), (0, 120), (120, 0), (300, 333)]
CONFIG = dict(n_particles=pf_scenes.N_PARTICLES, score_distribution=dict(mean=pf_scenes.SCORE_MEAN, sigma=pf_scenes.SCORE_SIGMA),
              thresholds=dict(offset=10, rotation=90, minimum_particles=20, track_limit=20.0))

_scorers = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_handles():
    yield
    for scorer in _scorers.values():
        scorer.close()
    _scorers.clear()


def _scorer(scene, switch):
    key = (scene.name, switch)
    if key not in _scorers:
        from acmpc_amd.particle_filter import ParticleScorer
        with pytest.MonkeyPatch.context() as patch:
            for name in SWITCHES[1:]:
                patch.delenv(name, raising=False)
            if switch is not None:
                patch.setenv(switch, "1")
            _scorers[key] = ParticleScorer(CONFIG, scene.track)
    return _scorers[key]


def given_form(track, counts):
    """Which pf_score_given_kernel launch_score picks (csrc/acmpc_pf_score.hip): 0 no wrap possible, 1 wrap and K <= 256, 2 K > 256."""
    K = sum(counts)
    lengths = (len(track["left"]), len(track["right"]))
    no_wrap = max(lengths) + K <= 65536 and K <= min(lengths)
    return (0 if no_wrap else 1) if K <= 256 else 2


def test_the_cases_reach_every_form(golden):
    forms = {name: {counts: given_form(pf_scenes.scene(name, golden).track, counts) for counts in COUNTS} for name in MAPS}
    assert forms["golden"][BASE] == 0 and forms["golden"][(200, 56)] == 0 and forms["golden"][(200, 57)] == 2
    assert forms["long"][BASE] == 1 and forms["long"][(200, 56)] == 1 and forms["long"][(200, 57)] == 2
    assert forms["tiny"][BASE] == 1 and forms["tiny"][(0, 120)] == 0 and forms["tiny"][(300, 333)] == 2
    long_map = pf_scenes.scene("long").track
    assert len(long_map["right"]) < 65536                    # below the uint16's range on its own, and still the wrap form
    lo = np.min([t.min(0) for t in long_map.values()], axis=0)
    hi = np.max([t.max(0) for t in long_map.values()], axis=0)
    cells = lambda size: int(np.prod(np.floor((hi - lo) / size) + 1))
    assert cells(8.0) > 2**20 >= cells(16.0)                 # build_grid doubles the cell once


def _score_and_check(scene, counts, P, switch):
    pf_scenes.check_preconditions(scene, counts)             # on the reference alone, before anything runs on the device
    ref = scene.reference(counts)
    states = scene.states[:P]
    out = _scorer(scene, switch).update_particles(states, scene.observation(counts))
    finite = np.isfinite(states).all(axis=1)
    rtol, atol = pf_scenes.error_tolerance(scene)
    deviation = np.abs(out["observation_error"][finite] - ref["observation_error"][:P][finite])
    print("pf-maps %-6s P=%-4d counts=%-10s %-24s |error - reference| max %.3e m, max relative %.3e; valid %d"
          % (scene.name, P, counts, switch or "default", deviation.max(),
             (deviation / ref["observation_error"][:P][finite]).max(), int(out["valid_mask"].sum())))
    np.testing.assert_array_equal(out["track_indices"], ref["track_indices"][:P])
    np.testing.assert_allclose(out["minimum_offset"][finite], ref["minimum_offset"][:P][finite], rtol=1e-12)
    np.testing.assert_allclose(out["heading_offset"][finite], ref["heading_offset"][:P][finite], rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["observation_error"][finite], ref["observation_error"][:P][finite], rtol=rtol, atol=atol)
    # the score's arithmetic at the device's OWN error (the error is judged above): a loose tolerance on the one cannot
    # hide a fault in the other
    np.testing.assert_allclose(out["score"][finite],
                               ref64.score_of_error(out["observation_error"][finite], pf_scenes.SCORE_MEAN, pf_scenes.SCORE_SIGMA),
                               rtol=1e-12, atol=1e-290)
    thresholds = pf_scenes.THRESHOLDS
    with np.errstate(invalid="ignore"):
        own = ((out["heading_offset"] < thresholds["rotation"]) & (out["minimum_offset"] < thresholds["offset"])
               & (out["observation_error"] < thresholds["track_limit"]))
    np.testing.assert_array_equal(out["valid_mask"], own)
    decided = pf_scenes.decided(scene, counts)[:P]
    np.testing.assert_array_equal(out["valid_mask"][decided], ref["valid"][:P][decided])
    if P > pf_scenes.NON_FINITE:                              # the particle without a position: point 0, not valid
        np.testing.assert_array_equal(out["track_indices"][pf_scenes.NON_FINITE], 0)
        assert not out["valid_mask"][pf_scenes.NON_FINITE]
    return out


@pytest.mark.parametrize("P", [1, 7, 500])
@pytest.mark.parametrize("name", MAPS)
def test_a_workgroup_per_particle(golden, name, P):
    """pf_score_kernel<1>: a wavefront per polyline searches the grid."""
    _score_and_check(pf_scenes.scene(name, golden), BASE, P, None)


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: s or "default")
@pytest.mark.parametrize("P", [4096, 4099])
@pytest.mark.parametrize("name", MAPS)
def test_the_forms_from_4096_particles_up(golden, name, P, switch):
    """4 099: a ragged last wave of pf_score_given_kernel, 3 of 8 particles in pf_score_kernel<8>'s last workgroup."""
    scene = pf_scenes.scene(name, golden)
    out = _score_and_check(scene, BASE, P, switch)
    if name == "long":                                        # the scene is what it is meant to be
        ref = scene.reference(BASE)
        assert ref["wrapped"][:P].sum() > 1000 and out["valid_mask"].sum() > 2500
        assert (out["track_indices"][:, 0] > 65535).sum() > 500 and (out["track_indices"][:, 0] < 400).sum() > 250


@pytest.mark.parametrize("switch", SWITCHES[:2], ids=lambda s: s or "default")
@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "%dx%d" % c)
@pytest.mark.parametrize("name", MAPS)
def test_observation_counts(golden, name, counts, switch):
    """256 points exactly (a point per lane and slot) and 257, an empty side, more points than the tiny map has."""
    _score_and_check(pf_scenes.scene(name, golden), counts, pf_scenes.N_PARTICLES, switch)
