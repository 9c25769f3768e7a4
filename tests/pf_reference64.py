"""The particle filter's arithmetic in plain float64 and Python / int64 integers, written from the definitions
(localiser.py:41-95,255-410,561-579) - NOT from the kernels' operation order: brute-force nearest
points, every index as a whole number that cannot overflow, library cos / sin / tan / arctan2 / exp, plain sums.
tests/test_pf_reference64.py holds it to the reference's own vectors and to the oracle; the GPU tests
(tests/test_gpu_pf_maps.py, tests/test_gpu_pf_filter.py) hold every kernel form to it.  A helper of the tests, not a test file.

Two things are float32 because they are the specification and not an accuracy choice: the particle states and the
observation are float32 data, and the observation is PLACED in a particle's frame in float32 (the reference does so,
localiser.py:330-353; csrc/acmpc_pf_score.hip says the same where it places).  Everything behind the placement is float64.
The normals of the control noise are specified bit for bit (oracle `box_muller_spec`), so they are taken from there.

Nothing here calls `oracle.pf_score_particles`."""
from __future__ import annotations

import numpy as np

import acmpc_oracle as orc

TAG_CONTROL = 0x4354524C   # "CTRL"


def nearest_points(points, track, chunk=256):
    """First minimum of dx*dx + dy*dy over the whole polyline for every point [P, 2] (float64): (index int64 [P],
    squared distance [P], relative gap [P] between the best and the second-best squared distance).  A point whose
    distances are all NaN or all infinite is nearest to point 0 (np.argmin), its gap is NaN."""
    points = np.asarray(points, dtype=np.float64)
    track = np.asarray(track, dtype=np.float64)
    P = points.shape[0]
    index = np.empty(P, dtype=np.int64)
    best = np.empty(P)
    gap = np.empty(P)
    with np.errstate(all="ignore"):
        for lo in range(0, P, chunk):
            q = points[lo:lo + chunk]
            dx = q[:, 0, None] - track[None, :, 0]
            dy = q[:, 1, None] - track[None, :, 1]
            d2 = dx * dx + dy * dy
            i = np.argmin(d2, axis=1)
            rows = np.arange(q.shape[0])
            b = d2[rows, i].copy()
            d2[rows, i] = np.inf
            second = d2.min(axis=1) if track.shape[0] > 1 else np.full(q.shape[0], np.inf)
            index[lo:lo + chunk], best[lo:lo + chunk] = i, b
            gap[lo:lo + chunk] = np.where(second == b, 0.0, (second - b) / second)      # (a point ON a repeated one: 0, not 0 / 0)
    return index, best, gap


def nearest_of_scene(states, centre, left, right):
    """The three queries of every particle: dict(index [P, 3] int64, d2 [P, 3], gap [P, 3]) - the expensive part of
    `score_particles`, which takes it back through `nearest=` so that a scene pays for it once."""
    xy = np.asarray(states, dtype=np.float32)[:, :2].astype(np.float64)
    parts = [nearest_points(xy, t) for t in (centre, left, right)]
    return dict(index=np.stack([p[0] for p in parts], 1), d2=np.stack([p[1] for p in parts], 1),
                gap=np.stack([p[2] for p in parts], 1))


def score_scale(mean, sigma):
    """Largest value of the normal density over 100 evenly spaced errors in [-10, 10] (localiser.py:655-661)."""
    x = (np.linspace(-10.0, 10.0, 100) - float(mean)) / float(sigma)
    return float(np.max(np.exp(-x * x / 2.0) / np.sqrt(2.0 * np.pi) / float(sigma)))


def score_of_error(error, mean, sigma):
    z = (np.asarray(error, dtype=np.float64) - float(mean)) / float(sigma)
    with np.errstate(under="ignore"):
        return np.exp(-z * z / 2.0) / np.sqrt(2.0 * np.pi) / float(sigma) / score_scale(mean, sigma)


def limit_indices(closest, count, m):
    """Indices [P, count] of the `count` limit points ahead of `closest` [P] on a polyline of m points: closest + i, the
    last entry closest + count when count > 1 (np.linspace(closest, closest + count, count) truncated), wrapped the way a
    uint16 wraps, THEN taken modulo m.  Also the unwrapped sums."""
    closest = np.asarray(closest, dtype=np.int64)
    off = np.arange(count, dtype=np.int64)
    if count > 1:
        off[-1] = count
    raw = closest[:, None] + off[None, :]
    return (raw & 0xFFFF) % int(m), raw


def score_particles(states, centre, left, right, obs_left, obs_right, mean, sigma, thresholds, nearest=None):
    """Scoring and validity of P particles.  states [P, 3] float32; centre / left / right [m, 2] float64; obs_* [k, 2]
    float32 in the vehicle frame (x right, y forward), either may be empty; thresholds = dict(rotation [rad], offset,
    track_limit).  Returns track_indices [P, 3], minimum_offset, heading_offset, observation_error, score, valid, gap
    [P, 3] (see nearest_points) and wrapped [P]: whether an index ahead of the particle went past 65 535."""
    states = np.asarray(states, dtype=np.float32)
    centre, left, right = (np.asarray(t, dtype=np.float64) for t in (centre, left, right))
    P = states.shape[0]
    if nearest is None:
        nearest = nearest_of_scene(states, centre, left, right)
    index, d2, gap = nearest["index"][:P], nearest["d2"][:P], nearest["gap"][:P]
    with np.errstate(all="ignore"):
        offset = np.sqrt(d2[:, 0])
        # heading of the centre line at the nearest point, both indices modulo m - 1
        m1 = centre.shape[0] - 1
        here, ahead = centre[index[:, 0] % m1], centre[(index[:, 0] + 1) % m1]
        track_heading = np.arctan2(ahead[:, 1] - here[:, 1], ahead[:, 0] - here[:, 0])
        yaw = states[:, 2].astype(np.float64)
        heading = np.abs(np.mod(track_heading - yaw + np.pi, 2.0 * np.pi) - np.pi)
        # the observation in every particle's frame: float32, the transpose of [[cos, -sin], [sin, cos]] of pi/2 - yaw
        obs_left = np.asarray(obs_left, dtype=np.float32).reshape(-1, 2)
        obs_right = np.asarray(obs_right, dtype=np.float32).reshape(-1, 2)
        obs_left, obs_right = obs_left[obs_left[:, 1] < 50], obs_right[obs_right[:, 1] < 50]
        obs = np.concatenate([obs_left, obs_right])
        angle = (-states[:, 2] + np.float32(np.pi / 2)).astype(np.float32)
        ca, sa = np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)
        ox, oy = obs[None, :, 0], obs[None, :, 1]
        placed_x = ((ca[:, None] * ox + sa[:, None] * oy) + states[:, 0, None]).astype(np.float32)
        placed_y = ((-sa[:, None] * ox + ca[:, None] * oy) + states[:, 1, None]).astype(np.float32)
        # the map's limits ahead of the nearest left and right points
        i_left, raw_left = limit_indices(index[:, 1], obs_left.shape[0], left.shape[0])
        i_right, raw_right = limit_indices(index[:, 2], obs_right.shape[0], right.shape[0])
        expected = np.concatenate([left[i_left], right[i_right]], axis=1)          # [P, K, 2]
        dx = placed_x.astype(np.float64) - expected[:, :, 0]
        dy = placed_y.astype(np.float64) - expected[:, :, 1]
        error = np.sqrt(dx * dx + dy * dy).sum(axis=1) / float(obs.shape[0])
        score = score_of_error(error, mean, sigma)
        valid = (heading < thresholds["rotation"]) & (offset < thresholds["offset"]) & (error < thresholds["track_limit"])
    wrapped = (np.concatenate([raw_left, raw_right], axis=1) > 0xFFFF).any(axis=1)
    return dict(track_indices=index.copy(), minimum_offset=offset, heading_offset=heading, observation_error=error,
                score=score, valid=valid, gap=gap.copy(), wrapped=wrapped)


def control_normals(n, seed, counter):
    """(z0, z1) [n] float32 of particle p = 0 ... n - 1: Philox4x32-10 at counter (p, counter, "CTRL", 0) under the key
    (seed & 0xffffffff, seed >> 32), words 0 and 1 to uniforms in (0, 1], one Box-Muller pair."""
    p = np.arange(n, dtype=np.uint32)
    ctr = np.stack([p, np.full_like(p, counter), np.full_like(p, TAG_CONTROL), np.zeros_like(p)], axis=1)
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    r = orc.philox4x32_10(ctr, np.broadcast_to(key, (n, 2)))
    return orc.box_muller_spec(orc.uniform_open(r[:, 0]), orc.uniform_open(r[:, 1]))


def kinematic_step(states, delta, velocity, dt, wheelbase):
    """states + (v cos yaw, v sin yaw, v tan delta / L) dt in float64 on float32 states; delta, velocity per particle."""
    s = np.asarray(states, dtype=np.float32).astype(np.float64)
    delta, velocity = np.asarray(delta, dtype=np.float64), np.asarray(velocity, dtype=np.float64)
    out = s.copy()
    out[:, 0] += velocity * np.cos(s[:, 2]) * dt
    out[:, 1] += velocity * np.sin(s[:, 2]) * dt
    out[:, 2] += velocity * np.tan(delta) / wheelbase * dt
    return out


def filter_step(states, tyre_angle, velocity, dt, sigma_yaw, sigma_v, wheelbase, seed, counter):
    """One step of the device-resident filter: every particle with its own noisy control, delta = tyre + sigma_yaw z0,
    v = |velocity + sigma_v z1|.  Returns the new states [n, 3] float64."""
    n = np.asarray(states).shape[0]
    z0, z1 = control_normals(n, seed, counter)
    delta = float(tyre_angle) + float(sigma_yaw) * z0.astype(np.float64)
    v = np.abs(float(velocity) + float(sigma_v) * z1.astype(np.float64))
    return kinematic_step(states, delta, v, float(dt), float(wheelbase))


def estimate(scores, states):
    """(estimate [3], largest distance to it, largest |yaw difference| to it): the score-weighted mean of the states, the
    plain mean where that is not a number (all scores zero, a NaN score)."""
    w = np.asarray(scores, dtype=np.float32).astype(np.float64)
    s = np.asarray(states, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        est = (s * w[:, None]).sum(axis=0) / w.sum()
    if np.isnan(est).any():
        est = s.sum(axis=0) / s.shape[0]
    distance = np.sqrt((s[:, 0] - est[0]) ** 2 + (s[:, 1] - est[1]) ** 2)
    return est, float(distance.max()), float(np.abs(s[:, 2] - est[2]).max())
