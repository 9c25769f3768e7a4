"""Maps, particles and observations of the particle-filter tests that the golden map alone does not stand for
(tests/test_pf_reference64.py, tests/test_gpu_pf_maps.py).  Everything is built from closed forms and seeded draws; the
float64 reference of a scene (tests/pf_reference64.py) is computed once per process and shared.  A helper, not a test file.

  golden   3 000 points per polyline: the map every other particle-filter test uses
  long     circles round the origin, 70 000 / 70 000 / 65 500 points at radius 4 300 / 4 295.25 / 4 304.75 m: indices
           beyond 65 535 (the limits ahead are taken through a uint16), a box of more than 2^20 cells of 8 m
  tiny     a closed loop of 150 / 149 / 151 points about 1.25 m apart: more observation points than map points, indices
           that go round the loop several times, and one point of every polyline repeated three places further on"""
from __future__ import annotations

import numpy as np

import pf_reference64 as ref64

N_PARTICLES = 4099
THRESHOLDS = dict(rotation=np.pi / 2, offset=10.0, track_limit=20.0)      # configs/monza.yaml:43-66, the angle in radians
SCORE_MEAN, SCORE_SIGMA = 0.0, 10.0
DUPLICATE_AT = {"tiny": (40, 97, 120)}     # per polyline: point j + 3 is point j again
NON_FINITE = 3                             # the particle without a position


def long_map():
    def circle(m, radius):
        theta = 2.0 * np.pi * np.arange(m) / m
        return np.stack([radius * np.cos(theta), radius * np.sin(theta)], axis=1)
    return dict(centre=circle(70000, 4300.0), left=circle(70000, 4295.25), right=circle(65500, 4304.75))


def tiny_map():
    def loop(m, shift):
        theta = 2.0 * np.pi * np.arange(m) / m
        radius = 29.8 * (1.0 + 0.08 * np.cos(3.0 * theta)) + shift
        return np.stack([radius * np.cos(theta), radius * np.sin(theta)], axis=1)
    track = dict(centre=loop(150, 0.0), left=loop(149, -4.75), right=loop(151, 4.75))
    for name, j in zip(("centre", "left", "right"), DUPLICATE_AT["tiny"]):
        # float32 coordinates, so that a (float32) particle can sit exactly on the point
        track[name][j] = track[name][j].astype(np.float32).astype(np.float64)
        track[name][j + 3] = track[name][j]
    return track


def golden_map(golden):
    return dict(centre=np.asarray(golden["pf/centre"], dtype=np.float64), left=np.asarray(golden["pf/left"], dtype=np.float64),
                right=np.asarray(golden["pf/right"], dtype=np.float64))


def heading_along(centre):
    tangent = np.roll(centre, -1, axis=0) - np.roll(centre, 1, axis=0)
    return np.arctan2(tangent[:, 1], tangent[:, 0])


def _round(track, heading, rng, indices, sd_xy, sd_yaw):
    """Particles round the given centre-line points."""
    n = len(indices)
    return np.concatenate([track["centre"][indices] + rng.normal(0, sd_xy, (n, 2)),
                           (heading[indices] + rng.normal(0, sd_yaw, n))[:, None]], axis=1)


def _particles(name, track, heading, pose_idx, rng):
    M = len(track["centre"])
    at_pose = np.full(N_PARTICLES, pose_idx)
    if name == "long":
        parts = [_round(track, heading, rng, at_pose[:2498], 1.5, 0.08),
                 _round(track, heading, rng, rng.integers(64900, 70000, 1200), 1.5, 0.08),   # both sides of 65 536 and of the end
                 _round(track, heading, rng, rng.integers(0, 400, 300), 1.5, 0.08)]
    elif name == "tiny":
        parts = [_round(track, heading, rng, at_pose[:1500], 1.5, 0.08),
                 _round(track, heading, rng, rng.integers(0, M, 2318), 2.0, 0.3)]
        near = []
        for key, j in zip(("centre", "left", "right"), DUPLICATE_AT[name]):
            spot = np.concatenate([track[key][j], [heading[round(j * M / len(track[key])) % M]]])
            on = np.tile(spot, (20, 1))
            on[:, 2] += rng.normal(0, 0.3, 20)                                             # exactly on the repeated point
            close = np.tile(spot, (40, 1)) + rng.normal(0, [0.4, 0.4, 0.3], (40, 3))       # and within a metre of it
            near += [on, close]
        parts += near
    else:
        parts = [_round(track, heading, rng, at_pose[:2000], 1.5, 0.08),
                 _round(track, heading, rng, rng.integers(0, M, 1968), 4.0, 0.5)]
        lo, hi = track["centre"].min(0), track["centre"].max(0)
        outside = np.concatenate([rng.uniform(lo - 3000.0, hi + 3000.0, (30, 2)), rng.uniform(-np.pi, np.pi, (30, 1))], axis=1)
        parts.append(outside)                                                              # far outside the map's box
    off = _round(track, heading, rng, at_pose[:100], 1.5, 0.08)
    off[:, :2] += 40.0                                                                     # 40 m off the track
    states = np.concatenate(parts + [off])
    assert states.shape[0] == N_PARTICLES - 1, states.shape
    states = states[rng.permutation(states.shape[0])]
    first = _round(track, heading, rng, at_pose[:1], 1.5, 0.08)                            # particle 0: one of the cluster
    states = np.concatenate([first, states]).astype(np.float32)
    states[NON_FINITE, 0] = np.nan
    return states


class Scene:
    """One map with its 4 099 particles; observations and references by (k_left, k_right), each computed once."""

    def __init__(self, name, track, pose_idx, seed):
        self.name, self.track, self.pose_idx, self.seed = name, track, pose_idx, seed
        self.heading = heading_along(track["centre"])
        self.states = _particles(name, track, self.heading, pose_idx, np.random.default_rng(seed))
        pose = track["centre"][pose_idx][None]
        self._ahead = {k: int(ref64.nearest_points(pose, track[k])[0][0]) for k in ("left", "right")}
        self._nearest = None
        self._observations, self._references = {}, {}
        self.largest_coordinate = float(max(np.abs(t).max() for t in track.values()))
        self.duplicates = DUPLICATE_AT.get(name)

    def observation(self, counts):
        """[left, right] float32 in the vehicle frame: `counts` consecutive points of the map's own limits from the pose on,
        plus noise of sd 0.15 m.  A point 50 m ahead or further is no part of an observation (the scorer drops it), so the
        cut is held at 49.5 m: the counts stay what a case names; such points fit the map badly, which changes nothing in
        a comparison with the reference."""
        if counts not in self._observations:
            rng = np.random.default_rng([self.seed, counts[0], counts[1]])
            a = np.pi / 2 - self.heading[self.pose_idx]
            rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            out = []
            for key, count in zip(("left", "right"), counts):
                t = self.track[key]
                cut = (t[(self._ahead[key] + np.arange(count)) % len(t)] - self.track["centre"][self.pose_idx]) @ rot.T
                cut = cut + rng.normal(0, 0.15, (count, 2))
                cut[:, 1] = np.minimum(cut[:, 1], 49.5)
                out.append(cut.astype(np.float32).reshape(count, 2))
            self._observations[counts] = out
        return self._observations[counts]

    def nearest(self):
        if self._nearest is None:
            self._nearest = ref64.nearest_of_scene(self.states, self.track["centre"], self.track["left"], self.track["right"])
        return self._nearest

    def reference(self, counts):
        """pf_reference64.score_particles of all 4 099 particles (particles are scored one by one: the reference of the
        first P is its first P rows).  Read only."""
        if counts not in self._references:
            left, right = self.observation(counts)
            out = ref64.score_particles(self.states, self.track["centre"], self.track["left"], self.track["right"], left, right,
                                        SCORE_MEAN, SCORE_SIGMA, THRESHOLDS, nearest=self.nearest())
            for value in out.values():
                value.setflags(write=False)
            self._references[counts] = out
        return self._references[counts]


_SCENES = {}


def scene(name, golden=None):
    if name not in _SCENES:
        if name == "long":
            _SCENES[name] = Scene(name, long_map(), 65400, 31)
        elif name == "tiny":
            _SCENES[name] = Scene(name, tiny_map(), 20, 32)
        else:
            _SCENES[name] = Scene(name, golden_map(golden), 700, 33)
    return _SCENES[name]


def error_tolerance(scn):
    """(rtol, atol) of `observation_error`: the project's 1e-5 plus one float32 ulp of the scene's largest |coordinate|.
    Both sides place the observation in float32; a last-bit difference of cosf / sinf flips the rounding of a placed
    coordinate by one ulp on a few of the K points, and their mean cannot move by more than that."""
    return 1e-5, float(np.spacing(np.float32(scn.largest_coordinate)))


def decided(scn, counts):
    """Particles whose reference heading, offset and error lie further from their thresholds than the tolerances the
    device's values are held to: their validity is the reference's, whatever the rounding."""
    ref = scn.reference(counts)
    rtol, atol = error_tolerance(scn)
    with np.errstate(invalid="ignore"):
        return ((np.abs(ref["heading_offset"] - THRESHOLDS["rotation"]) > 1e-9)
                & (np.abs(ref["minimum_offset"] - THRESHOLDS["offset"]) > 1e-12 * ref["minimum_offset"])
                & (np.abs(ref["observation_error"] - THRESHOLDS["track_limit"]) > rtol * ref["observation_error"] + atol))


def check_preconditions(scn, counts):
    """What a comparison with the reference rests on, asserted on the reference alone: no nearest point is a near-tie that
    rounding could decide (the planted repeats are exact ties, and go to the lower index), and all but a few particles are
    far enough from every threshold for their validity to be the reference's."""
    ref = scn.reference(counts)
    finite = np.isfinite(scn.states).all(axis=1)
    assert (~finite).sum() == 1 and not finite[NON_FINITE]
    gap, index = ref["gap"], ref["track_indices"]
    for t in range(3):
        tie = gap[:, t] == 0
        if scn.duplicates is None:
            assert not tie.any()
        else:
            assert tie.sum() >= 20 and (index[tie, t] == scn.duplicates[t]).all()
            assert not (index[:, t] == scn.duplicates[t] + 3).any()
        assert (gap[finite & ~tie, t] > 1e-9).all(), gap[finite & ~tie, t].min()
    left_out = int((~decided(scn, counts)).sum())
    assert left_out <= 0.005 * N_PARTICLES, left_out
    np.testing.assert_array_equal(index[NON_FINITE], 0)
    assert not ref["valid"][NON_FINITE]
