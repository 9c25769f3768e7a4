"""Mode D behind the drop-in entry point on the MI355X: `rollout_mode: "D"` in the control config -> `build_mpc` /
`SpatialMPC.get_control(..., motion=)` score with a DynamicSamplingSolver, and the reference's read-after-call attributes carry
the plan ("Mode D, plan trace").  Tick for tick against the solver called directly, and test_gpu_dynamic's
closed loop driven through `published_plan` + `TemporalCommandSelector`."""
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_dynamic as tgd

pytestmark = pytest.mark.gpu

# The speed profile of get_control's host path is the reference's: the ceiling min(v_max, sqrt(ay_max / |kappa|)) PLUS 2 m/s
# (speed_profile.py: velocity_ceiling), under acceleration limits.  test_gpu_dynamic's loop drives min(34, sqrt(8 / |kappa|)),
# which is 34 m/s all the way round (its tightest corner allows 36.9): ay_max 8 and v_max 34 - 2 give that very profile, with
# acceleration limits that do not bind, no end velocity and no curvature threshold.
CONSTRAINTS = dict(v_min=8.0, v_max=tgd.LOOP_V_MAX - 2.0, a_min=-20.0, a_max=20.0, ay_max=tgd.LOOP_AY, ki_min=0.0, end_velocity=None)


def _mpc():
    from acmpc_amd import workloads
    from acmpc_amd.mpc import build_mpc
    cfg = dict(tgd.LOOP_CONFIG, rollout_mode="D", speed_profile_constraints=dict(CONSTRAINTS))
    mpc = build_mpc(cfg, workloads.PlaceholderVehicle())
    assert mpc.model.margin == tgd.LOOP_CONFIG["margin"]
    return mpc


def _window(centre, state):
    """The H x 3 path window ahead of the car in the VEHICLE frame: the car at the origin, heading +y."""
    i0 = int(np.argmin(((centre - state[:2]) ** 2).sum(axis=1)))
    idx = (i0 + tgd.LOOP_STRIDE * np.arange(tgd.LOOP_H)) % len(centre)
    rot = np.pi / 2 - state[2]
    c, s = np.cos(rot), np.sin(rot)
    local = (centre[idx] - state[:2]) @ np.array([[c, s], [-s, c]])
    return np.column_stack([local, np.full(tgd.LOOP_H, tgd.LOOP_WIDTH)])


def _command(mpc):
    """What the agent applies at the moment the plan is published: (steering, pedal) of the selected step."""
    from acmpc_amd.command_selection import TemporalCommandSelector
    from acmpc_amd.mpc import published_plan
    plan = published_plan(mpc)
    steering = float(TemporalCommandSelector(plan)(0.0)[1])
    pedals = SimpleNamespace(control_inputs=mpc.projected_pedal[:, None], control_cumtime=plan.control_cumtime)
    return steering, float(TemporalCommandSelector(pedals)(0.0)[0]), plan


def _start():
    centre, v_profile, heading, start = tgd.loop_track()
    state = np.array([centre[start, 0], centre[start, 1], heading[start], v_profile[start] - 4.0, 0.0, 0.0])
    return centre, v_profile, heading, state


def test_get_control_is_the_solver_called_directly():
    """20 consecutive ticks along the circuit: the plan of get_control is the plan of a DynamicSamplingSolver of the same
    config and seed on the same table from the same state, bit for bit, and the attributes are that plan's."""
    from acmpc_amd import DynamicBicycleParams, DynamicSamplingSolver
    plant = DynamicBicycleParams.reference()
    mpc = _mpc()
    direct = DynamicSamplingSolver(dict(tgd.LOOP_CONFIG, plan_states=True), plant)
    centre, v_profile, heading, state = _start()
    n = tgd.LOOP_H - 1
    for tick in range(20):
        mpc.get_control(_window(centre, state), motion=state[3:])
        assert mpc.infeasibility_counter == 0, tick
        np.testing.assert_array_equal(mpc.reference_path.velocities, np.full(n, tgd.LOOP_V_MAX))   # the loop's profile
        obj = direct.solve(np.array([0.0, 0.0, np.pi / 2, *state[3:]]), mpc.reference_path.table)
        u = obj.x[3 * (n + 1):].reshape(n, 2)
        np.testing.assert_array_equal(mpc.projected_control[1], u[:, 0])
        np.testing.assert_array_equal(mpc.projected_pedal, u[:, 1])
        np.testing.assert_array_equal(mpc.plan_states, obj.states)
        np.testing.assert_array_equal(mpc.projected_control[0], mpc.plan_states[1:, 3])
        np.testing.assert_array_equal(mpc.current_prediction, mpc.plan_states[:n, :2])
        np.testing.assert_array_equal(mpc.plan_states[:, :3], obj.x[:3 * (n + 1)].reshape(n + 1, 3))
        np.testing.assert_array_equal(mpc.plan_states[0], np.array([0.0, 0.0, np.pi / 2, *state[3:]], dtype=np.float32))
        assert mpc.plan_violation == obj.violation and mpc.cum_time[1] == tgd.LOOP_DT
        steering, pedal, plan = _command(mpc)
        assert steering == u[0, 0] and pedal == u[0, 1] and plan.control_inputs.shape == (n, 2)
        state = plant.predict_next_state(state, (steering, pedal), tgd.LOOP_DT)[0]
        state[3] = max(state[3], 0.0)
    trace = mpc._control_solver.dynamic_solver.trace()
    np.testing.assert_array_equal(trace["states"][0], mpc.plan_states.astype(np.float32))
    assert trace["violation"][0] == np.float32(mpc.plan_violation)
    direct.close()


def test_closed_loop_through_the_published_plan():
    """test_gpu_dynamic's loop - 400 ticks against the float64 plant - with the controller behind get_control and the command
    read the way the agent reads it; held to that loop's own bounds (test_gpu_dynamic.check_loop)."""
    from acmpc_amd import DynamicBicycleParams
    plant = DynamicBicycleParams.reference()
    mpc = _mpc()
    centre, v_profile, heading, state = _start()
    log = []
    for tick in range(tgd.LOOP_TICKS):
        mpc.get_control(_window(centre, state), motion=state[3:], elapsed=tgd.LOOP_DT)
        assert mpc.infeasibility_counter == 0, "tick %d was not solved" % tick
        steering, pedal, _ = _command(mpc)
        state = plant.predict_next_state(state, (steering, pedal), tgd.LOOP_DT)[0]
        state[3] = max(state[3], 0.0)
        ey, i = tgd.loop_frenet(centre, heading, state)
        log.append((ey, abs(state[4]) / max(state[3], 1.0), state[3] - v_profile[i], i))
    log = np.array(log)
    ey, slip, dv, _ = log.T
    print("mode D behind get_control, 400 ticks: max |e_y| %.3f m, mean |e_y| %.3f m, sideslip %.4f, speed error %.3f m/s, %d "
          "waypoints" % (np.abs(ey).max(), np.abs(ey).mean(), slip.max(), np.abs(dv[40:]).max(), (log[-1, 3] - log[0, 3]) % 11586))
    tgd.check_loop(log)
