#!/usr/bin/env python3
"""Golden vectors of mode D's vehicle, computed by IMPORTING the reference's DynamicBicycleModel
(src/acmpc/control/dynamic_bicycle_model.py; never copied).  The module imports matplotlib at the top, so it is loaded
under the Agg backend.

    python tests/golden/gen_dynamic_golden.py <the reference's src directory>    # rewrites tests/golden/dynamic_bicycle.npz

Recorded (numbers only):
  coef_literal     [26]  the reference's block as it holds it (curve_fit output included), ABI order
  coef_kn          [26]  the same with the nine longitudinal coefficients times 1e-3 (the default vehicle)
  step_*           ~300 single steps (state, u, dt) -> (next_state, x_dot, forces) of predict_next_state, half with
                   each block: random states, vx near 0, large yaw, full lock, full brake
  roll_*           20 fifty-step rollouts with the reference loop's clip vx >= 0 (dynamic_bicycle_model.py:180), kN block
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "ac-mpc_amd"))
from acmpc_amd.dynamic_model import FIELDS, LONGITUDINAL  # noqa: E402


def load_reference(src):
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, src)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from acmpc.control.dynamic_bicycle_model import DynamicBicycleModel
        return DynamicBicycleModel()


def block(model):
    return np.array([float(getattr(model, k)) for k in FIELDS])


def set_block(model, coef):
    for k, v in zip(FIELDS, coef):
        setattr(model, k, float(v))
    model.F_zf = model.mass * model.g * model.lr / (model.lr + model.lf)
    model.F_zr = model.mass * model.g * model.lf / (model.lr + model.lf)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    model = load_reference(sys.argv[1])
    literal = block(model)
    kn = literal.copy()
    for k in LONGITUDINAL:
        kn[FIELDS.index(k)] *= 1e-3
    rng = np.random.default_rng(20261016)
    states, us, dts, tags = [], [], [], []
    for i in range(300):
        s = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-np.pi, np.pi), rng.uniform(0, 60),
                      rng.uniform(-2, 2), rng.uniform(-1, 1)])
        u = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-1, 1)])
        kind = i % 6
        if kind == 1:
            s[3] = rng.choice([0.0, 1e-4, 1e-3, 0.05])          # vx near 0
        elif kind == 2:
            s[2] = rng.uniform(-40, 40)                          # large yaw
        elif kind == 3:
            u[0] = rng.choice([-0.3, 0.3])                       # full lock
        elif kind == 4:
            u[1] = -1.0                                          # full brake
        states.append(s)
        us.append(u)
        dts.append(rng.choice([0.05, 0.02, 0.1]))
        tags.append(i % 2)                                       # 0 = literal block, 1 = kN block
    nxt, xdot, forces = [], [], []
    for s, u, dt, tag in zip(states, us, dts, tags):
        set_block(model, literal if tag == 0 else kn)
        a, b, c = model.predict_next_state(s.copy(), u.copy(), dt)
        nxt.append(np.asarray(a, dtype=np.float64))
        xdot.append(np.asarray(b, dtype=np.float64))
        forces.append(np.asarray(c, dtype=np.float64))
    set_block(model, kn)
    r_x0, r_u, r_states = [], [], []
    for i in range(20):
        s = np.array([rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-np.pi, np.pi), rng.uniform(5, 50),
                      rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2)])
        t = np.arange(50)
        U = np.stack([0.08 * rng.uniform(-1, 1) * np.sin(t / rng.uniform(4, 12) + rng.uniform(0, 6)),
                      np.clip(rng.uniform(-0.6, 0.8) + 0.3 * np.sin(t / rng.uniform(5, 15)), -1, 1)], axis=1)
        traj = [s.copy()]
        state = s.copy()
        for u in U:
            state, _, _ = model.predict_next_state(state, u, 0.05)
            state = np.asarray(state, dtype=np.float64)
            state[3] = np.clip(state[3], 0, np.inf)
            traj.append(state.copy())
        r_x0.append(s)
        r_u.append(U)
        r_states.append(np.stack(traj))
    out = os.path.join(HERE, "dynamic_bicycle.npz")
    np.savez_compressed(out, fields=np.array(FIELDS), coef_literal=literal, coef_kn=kn, step_state=np.array(states),
                        step_u=np.array(us), step_dt=np.array(dts), step_block=np.array(tags), step_next=np.array(nxt),
                        step_xdot=np.array(xdot), step_forces=np.array(forces), roll_x0=np.array(r_x0),
                        roll_u=np.array(r_u), roll_states=np.array(r_states), roll_dt=np.float64(0.05))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
