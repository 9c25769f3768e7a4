"""`GripEstimator`: which grip is the car on?  It keeps the last second or two of logged (vx, vy, r) and (delta, pedal),
scores a grid of hypothetical vehicles - the engine's vehicle 0 with its front and rear Pacejka peaks scaled - against the
log on the GPU (`Engine.score_grips`, csrc/acmpc_identify.hip) and answers only when the log can tell them apart.

    est = GripEstimator(engine, grid=np.arange(0.3, 1.5001, 0.05), axles="tied", dt=0.05)
    est.push(state, control)          # every tick: the state now and the control applied SINCE the previous push
    g = est.estimate()                # g.front, g.rear, g.error, g.accepted, g.errors

Acceptance rule: at least `min_window` transitions are held, the best error E_best is finite, and

    median(finite E) - E_best > max(contrast * E_best, floor)

A window without lateral excitation (a straight: every hypothesis predicts it equally well) carries no information and is
never accepted; `front` / `rear` then stay at the last accepted estimate (None before there is one).  The defaults
contrast = 0.25 and floor = 1e-6 come from the float64 mirror ("Mode D, grip identification";
tests/test_grip_identification.py re-derives them): on a noise-free, float32-rounded log the true hypothesis scores about
2e-11 and its grid neighbour 3e-4, so 1e-6 separates rounding from information; with sensor noise of (0.05, 0.02, 0.01) on
(vx, vy, r) the best hypothesis scores 0.31 against a median of 1.6 - a contrast of 4, sixteen times the bar."""
from __future__ import annotations

from collections import deque
from types import SimpleNamespace
from typing import Optional

import numpy as np

AXLES = ("tied", "split")


def grip_scales(grid, axles: str = "tied") -> np.ndarray:
    """The hypotheses [K, 2] = (front, rear) of a grid of scales: "tied" - both axles on the same scale, K = len(grid);
    "split" - every pair, front-major, K = len(grid)^2."""
    g = np.asarray(grid, dtype=np.float64).ravel()
    if g.size == 0 or not np.all(np.isfinite(g)) or not np.all(g > 0.0):
        raise ValueError("a grip grid is a non-empty list of finite, positive scales")
    if axles == "tied":
        return np.ascontiguousarray(np.stack([g, g], axis=1))
    if axles == "split":
        front, rear = np.meshgrid(g, g, indexing="ij")
        return np.ascontiguousarray(np.stack([front.ravel(), rear.ravel()], axis=1))
    raise ValueError("axles is 'tied' or 'split', not %r" % (axles,))


class GripEstimator:
    def __init__(self, engine, grid=None, axles: str = "tied", window: int = 40, min_window: int = 10, segment: int = 1,
                 weights=(1.0, 1.0, 1.0), contrast: float = 0.25, floor: float = 1e-6, dt: float = 0.05):
        """`engine`: a mode D `Engine` with a vehicle set, or any callable with `Engine.score_grips`' signature
        `(states, controls, dt, scales, segment=, weights=) -> (errors, best_index)`.  `dt`: the log's period."""
        self._score = engine.score_grips if hasattr(engine, "score_grips") else engine
        self._scales = grip_scales(np.arange(0.3, 1.5001, 0.05) if grid is None else grid, axles)
        grid_values = np.unique(self._scales[:, 0])
        self.grid_step = float(np.min(np.diff(grid_values))) if grid_values.size > 1 else 0.0
        self._window, self._min_window, self._segment = int(window), int(min_window), int(segment)
        if not 1 <= self._min_window <= self._window:
            raise ValueError("1 <= min_window <= window")
        if self._segment < 1:
            raise ValueError("segment must be positive")
        self._weights = tuple(float(w) for w in weights)
        self._contrast, self._floor, self._dt = float(contrast), float(floor), float(dt)
        self._states = deque(maxlen=self._window + 1)
        self._controls = deque(maxlen=self._window)
        self._accepted: Optional[tuple] = None   # (front, rear) of the last accepted estimate

    @property
    def scales(self) -> np.ndarray:
        return self._scales

    @property
    def transitions(self) -> int:
        return len(self._controls)

    def reset(self):
        self._states.clear()
        self._controls.clear()

    def push(self, state, control=None):
        """The state now - (X, Y, yaw, vx, vy, r) or (vx, vy, r) - and the control (delta, pedal) applied since the previous
        push.  The first push of a log has no control before it (None, or ignored)."""
        x = np.asarray(state, dtype=np.float32).ravel()
        if x.size == 6:
            x = x[3:]
        if x.size != 3:
            raise ValueError("a state is (X, Y, yaw, vx, vy, r) or (vx, vy, r)")
        if self._states:
            if control is None:
                raise ValueError("every push after the first needs the control applied since the previous one")
            self._controls.append(np.asarray(control, dtype=np.float32).ravel()[:2].copy())
        self._states.append(x.copy())

    def estimate(self) -> SimpleNamespace:
        """Scores the grid against the held window: `front`, `rear` = the last ACCEPTED estimate (None before one), `error`
        = this window's best error, `accepted` = whether this window's argmin was accepted, `errors` [K] (None while no
        transition is held)."""
        W = len(self._controls)
        accepted, error, errors = False, float("nan"), None
        if W >= 1:
            errors, best = self._score(np.stack(self._states), np.stack(self._controls), self._dt, self._scales,
                                       segment=min(self._segment, W), weights=self._weights)
            errors = np.asarray(errors)
            error = float(errors[best])
            finite = errors[np.isfinite(errors)]
            if W >= self._min_window and np.isfinite(error) and finite.size:
                accepted = bool(float(np.median(finite.astype(np.float64))) - error > max(self._contrast * error, self._floor))
            if accepted:
                self._accepted = (float(self._scales[best, 0]), float(self._scales[best, 1]))
        front, rear = self._accepted if self._accepted is not None else (None, None)
        return SimpleNamespace(front=front, rear=rear, error=error, accepted=accepted, errors=errors)
