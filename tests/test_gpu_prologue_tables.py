"""Every table the tick's prologue kernel (csrc/acmpc_prologue.hip) builds, against the reference of tests/prologue_cases.py
(the oracle and NumPy alone - never the library's host path, never the kernel's own output handed back to it): the 7 x n
waypoint table, the speed profile, the start state, the packed float32 rows, `u_ref` and the centre sequence; at the horizons
on both sides of every lane and input-route edge (H = 3, 4, 64 | 65, 66, 128, 129 and the workload's 50), in modes S, T with
the exhaustive search (the frames workgroup runs beside) and T with a window, by every route the inputs can take (kernel
arguments, pinned memory, a replayed graph's header pointer, the bound map), with and without a previous plan.

Ticks run one candidate and one round with sigma = 0: candidate 0 of a round is the clipped centre (`orc.sample_candidates`),
so the winner's controls ARE the centre sequence the prologue wrote, every index of both lane slots.

PSI_ULPS: the device's double atan2 against the long double heading, largest error measured on the MI355X:
0.934 ulp(pi) over the whole case list (H128_wiggly_0), 0.771 over the map windows; in units of the heading's own
last place 1.32 and 0.94 - more than the "last float64 bit" once claimed for it.  The ROCm tree states no bound for double
atan2, so the bound asserted is the measured figure rounded up to the next whole ulp(pi): 1.  kappa's bound follows from it
(`prologue_cases.kappa_bound`).  Every test prints its figures before it asserts."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import acmpc_oracle as orc
import prologue_cases as pc
from test_support import RACING

pytestmark = pytest.mark.gpu

PSI_ULPS = 1.0
KEYS = ("table", "x0", "u_ref", "coef", "record", "info6")
ROUTES = ((), ("ACMPC_TICK_NO_INLINE_PATH",), ("ACMPC_TICK_GRAPH",), ("ACMPC_TICK_NO_FLAG",))


def _engine(mode, n, switches=()):
    from acmpc_amd import Engine
    number, window = pc.MODES[mode]
    cfg = RACING["monza"]
    eng = Engine(mode=number, max_problems=1, max_candidates=1, max_steps=n, step_cost=cfg["step_cost"], r_term=cfg["r_term"],
                 final_cost=cfg["final_cost"], u_min=pc.BOX[0], u_max=pc.BOX[1], margin=pc.LIMITS.margin,
                 wheelbase=pc.LIMITS.length, dt=0.05, nn_window=window)
    for name in switches:
        eng.set_option(name, "1")
    return eng


def _tick(case, centre_is_reference=1, qp_method=0, seed=5):
    from acmpc_amd import _capi
    t = _capi.Tick()
    t.struct_size = _capi.C.sizeof(_capi.Tick)
    t.horizon, t.localised, t.has_end_velocity = case.H, case.localised, case.has_end_velocity
    t.n_candidates, t.rounds, t.centre_is_reference = 1, 1, centre_is_reference
    t.qp_max_iter, t.qp_check_every, t.qp_method = 4000, 10, qp_method
    t.offset = case.offset
    cons = pc.CONS
    t.v_min, t.v_max, t.a_min, t.a_max = cons["v_min"], cons["v_max"], cons["a_min"], cons["a_max"]
    t.ay_max, t.ki_min, t.end_velocity = cons["ay_max"], cons["ki_min"], cons["end_velocity"]
    t.sigma[0], t.sigma[1], t.shrink = 0.0, 0.0, 0.5
    t.qp_eps_abs = t.qp_eps_rel = 1e-3
    t.seed = seed
    return t


def _random_centre(n, seed):
    """A previous plan no tick would make: float32, a different value at every index, some outside the input box."""
    rng = np.random.default_rng(seed)
    lo, hi = pc.BOX
    centre = np.stack([rng.uniform(lo[0] - 4.0, hi[0] + 4.0, n), rng.uniform(1.5 * lo[1], 1.5 * hi[1], n)], axis=1)
    centre[0, 0], centre[n - 1, 1] = hi[0] + rng.uniform(1.0, 3.0), lo[1] * rng.uniform(1.1, 1.4)   # (also at n = 2)
    centre = centre.astype(np.float32)
    assert np.unique(centre).size == 2 * n and centre[0, 0] > hi[0] and centre[n - 1, 1] < lo[1]
    return centre


def _run(eng, case, tick, coords, centre):
    """One tick and everything it left: the caller's outputs and the device's tables."""
    out = eng.control_tick(tick, coords, centre)
    x0, u_ref, coef = eng.tick_device_tables(case.n)
    got = dict(out, x0=x0, u_ref=u_ref, coef=coef, info6=out["info"][:6].copy())
    if eng.describe_rounds(1, 1, case.n)["tick_frames"]:
        got["frames"] = eng.tick_device_frames(case.n)
    return got


def _controls(got, n):
    from acmpc_amd import _capi
    return got["record"][_capi.REC_HEADER:_capi.REC_HEADER + 2 * n].reshape(n, 2)


def _check(case, mode, got, what, coords=None):
    from acmpc_amd import _capi
    path = case.coords if coords is None else coords
    error = pc.heading_error(path, got["table"][orc.ROW_PSI])
    print("%s %s %s: heading error %.4f ulp(pi), %.4f of its own last place"
          % (case.name, mode, what, error, pc.heading_error_in_own_ulps(path, got["table"][orc.ROW_PSI])))
    pc.check_tables(case, mode, got["table"], PSI_ULPS, coef=got["coef"], x0=got["x0"], u_ref=got["u_ref"], info=got["info"],
                    coords=coords, what=what)
    if "frames" in got:     # the second workgroup read the same path: its frames are the host's of these rows
        pc.assert_bits(got["frames"], _capi.search_frames(got["coef"][None])[0], "%s %s %s frames" % (case.name, mode, what))
    return error


def _same(want, got, what):
    for key in KEYS + (("frames",) if "frames" in want else ()):
        pc.assert_bits(got[key], want[key], "%s: %s" % (what, key))


@pytest.mark.parametrize("H", pc.HORIZONS)
@pytest.mark.parametrize("mode", list(pc.MODES))
def test_prologue_tables_by_every_route(mode, H):
    """Per case: a tick without a previous plan (the record's controls are `u_ref`, bit for bit) and one with a random plan
    (they are `clip32(centre)` at every step: at n = 65 and 128 the second lane slot's last element), each by the inline route
    (H <= 64; beyond it the default IS the pinned route), with ACMPC_TICK_NO_INLINE_PATH (H <= 64), by a replayed graph and
    with the stream synchronised instead of the flag polled.  Every route's tables are held to the reference, and all routes
    give the same bits."""
    n = H - 1
    routes = [r for r in ROUTES if H <= 64 or r != ("ACMPC_TICK_NO_INLINE_PATH",)]
    engines = [(route, _engine(mode, n, route)) for route in routes]
    worst = 0.0
    for case in pc.cases_at(H):
        centre = _random_centre(n, 7 * H + case.index)
        first, second = None, None
        for route, eng in engines:
            label = "+".join(route) or "default"
            cold = _run(eng, case, _tick(case, 1), case.coords, None)
            worst = max(worst, _check(case, mode, cold, label))
            pc.assert_bits(_controls(cold, n), cold["u_ref"], "%s %s %s: controls == u_ref" % (case.name, mode, label))
            warm = _run(eng, case, _tick(case, 0, seed=6), case.coords, centre)
            _check(case, mode, warm, label + " with a previous plan")
            pc.assert_bits(_controls(warm, n), pc.clip32(centre), "%s %s %s: controls == clip32(centre)" % (case.name, mode, label))
            pc.assert_bits(cold["coords"], case.coords, case.name + " coords")
            if first is None:
                first, second = cold, warm
            else:
                _same(first, cold, "%s %s %s against the default route" % (case.name, mode, label))
                _same(second, warm, "%s %s %s against the default route, with a previous plan" % (case.name, mode, label))
    print("H %d mode %s: largest heading error %.4f ulp(pi)" % (H, mode, worst))
    for _, eng in engines:
        eng.close()


@pytest.mark.parametrize("H", [4, 50, 100, 125])
@pytest.mark.parametrize("mode", list(pc.MODES))
def test_prologue_tables_from_the_bound_map(mode, H):
    """The prologue's own lanes cut the path out of the bound map (`map_path_row`; in mode T its second workgroup cuts the same
    window for the frames): a map index, one whose window wraps past the end of the map, and a pose.  The path it reports is
    the window kernel's bit for bit, and every table is held to the reference evaluated on that path."""
    from acmpc_amd import workloads
    track = workloads.synthetic_track("monza")
    M = len(track["centre"])
    n = H - 1
    engines = [(route, _engine(mode, n, route)) for route in ((), ("ACMPC_TICK_GRAPH",))]
    for _, eng in engines:
        eng.bind_map(track["centre"], track["spacing"])
    pose_index = M // 3
    pose = track["centre"][pose_index] + np.array([0.3, -0.2])
    for i, (map_index, lateral) in enumerate(((17, 0.2), (M - 40, -0.2), (-1, 0.1), (M // 2, 0.0))):
        case = SimpleNamespace(name="map_H%d_at_%d" % (H, map_index), H=H, n=n, index=i, localised=int(i == 3),
                               has_end_velocity=int(i % 2 == 0), offset=lateral, coords=None)
        first = None
        for route, eng in engines:
            label = "+".join(route) or "default"
            want_coords, want_first = eng.map_reference_path(H, map_index=map_index, pose=pose, lateral_offset=lateral)
            tick = _tick(case, 1)
            tick.map_index, tick.centreline_points, tick.lateral_offset = map_index, 500, lateral
            tick.pose_x, tick.pose_y = pose[0], pose[1]
            got = _run(eng, case, tick, None, None)
            pc.assert_bits(got["coords"], want_coords, "%s %s: the window" % (case.name, label))
            assert int(got["info"][6]) == want_first == (map_index % M if map_index >= 0 else want_first)
            _check(case, mode, got, label, coords=got["coords"])
            pc.assert_bits(_controls(got, n), got["u_ref"], "%s %s %s: controls == u_ref" % (case.name, mode, label))
            if first is None:
                first = got
            else:
                _same(first, got, "%s %s %s against the default route" % (case.name, mode, label))
                pc.assert_bits(got["coords"], first["coords"], case.name + " coords")
    for _, eng in engines:
        eng.close()


@pytest.mark.parametrize("mode", list(pc.MODES))
def test_one_handle_through_changing_horizons(mode):
    """Ticks at H = 129, 3, 65, 64, 129 on ONE handle of 128 steps, first with the splitting (qp_method 1: the warm state's
    `warm_n` must keep an iterate of another horizon out), then with the exact profile, a localised tick (the second solver
    slot) in between, a previous plan on every other tick: each equals the same tick on a fresh handle bit for bit - nothing
    of a longer horizon's LDS, staging block or warm state shows."""
    def at(H, name="arc_r25_left"):
        return [c for c in pc.cases_at(H) if c.name.endswith(name)][0]

    def localised(H):
        return [c for c in pc.cases_at(H) if c.localised][0]

    sequence = [(at(129), 1), (at(3), 1), (at(65), 1), (localised(65), 1), (at(64), 1), (at(129), 1),
                (at(129), 0), (at(3), 0), (at(65), 0), (localised(64), 0), (at(64), 0), (at(129, "rotated_to_minus_pi"), 0)]
    eng = _engine(mode, 128)
    for step, (case, qp_method) in enumerate(sequence):
        centre = _random_centre(case.n, 100 + step) if step % 2 else None
        got = _run(eng, case, _tick(case, int(centre is None), qp_method, seed=step), case.coords, centre)
        fresh_engine = _engine(mode, 128)
        fresh = _run(fresh_engine, case, _tick(case, int(centre is None), qp_method, seed=step), case.coords, centre)
        fresh_engine.close()
        what = "step %d %s qp_method %d" % (step, case.name, qp_method)
        _same(fresh, got, what)
        assert got["info"][4] == 0 and (got["info"][5] == 0) == (qp_method == 0), what
        if qp_method == 0:
            _check(case, mode, got, what)
        want = got["u_ref"] if centre is None else pc.clip32(centre)
        pc.assert_bits(_controls(got, case.n), want, what + ": controls")
    eng.close()
