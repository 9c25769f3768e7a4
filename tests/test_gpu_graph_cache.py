"""The captured-graph caches of `acmpc_optimize` and `acmpc_control_tick` (four slots each, least recently used slot
re-captured): more shapes than slots on ONE handle, so that eviction, re-capture and a hit after both run; every part
of the key that selects a graph; `acmpc_set_option` and a map re-bind dropping what was captured.

Oracle: the library itself by another route - a fresh handle per call (its first capture), the eager path
(ACMPC_NO_GRAPH) and the tick's direct launches - whose bits the other GPU tests pin to the oracle.  Everything is
compared bit for bit.
"""
import numpy as np
import pytest

import acmpc_oracle as orc
from test_support import RACING, engine_kwargs, make_problem

pytestmark = pytest.mark.gpu

P, H = 2, 13
n = H - 1
KEYS = [(N, rounds) for N in (128, 256) for rounds in (1, 2, 3)]   # six keys for four slots
VISITS = list(range(6)) + [0, 5]                                    # k0 .. k5, k0 again (evicted by then), k5 (a hit)
SIGMA = (3.0, 0.01)


@pytest.fixture(scope="module")
def problems():
    probs = [make_problem(orc, "silverstone", H, 4, seed=700 + p) for p in range(P)]
    u_ref = np.stack([np.stack([p["table"][orc.ROW_V], p["table"][orc.ROW_KAPPA]], axis=1) for p in probs]).astype(np.float32)
    return dict(probs=probs, tables=np.stack([p["table"] for p in probs]), u_ref=u_ref,
                x0={0: np.stack([p["x0"] for p in probs]), 1: np.stack([p["pose0"] for p in probs])})


def _handle(problems, mode, options=(), paths=True, **extra):
    from acmpc_amd import Engine
    eng = Engine(**engine_kwargs(problems["probs"][0], mode, P, 256, n, **extra))
    for name in options:
        eng.set_option(name, "1")
    if paths:
        eng.set_paths(problems["tables"])
    return eng


def _optimize(eng, problems, mode, key, with_ref=True, sigma=SIGMA):
    N, rounds = KEYS[key]
    u_ref = problems["u_ref"]
    return eng.optimize(problems["x0"][mode], u_ref, u_ref if with_ref else None, N, rounds, sigma, shrink=0.5,
                        seed=100 + key)["records"].copy()


@pytest.mark.parametrize("mode", [0, 1])
def test_optimize_through_more_keys_than_slots(problems, mode):
    """Six (N, rounds) keys on one handle, then the first again - its slot has been re-used since - then the last, a hit:
    every record block equals the same call on a fresh handle and on a handle on the eager path; two calls that differ
    only in u_ref given / None (part of the key) each equal their fresh handle's."""
    want = []
    for key in range(6):
        fresh = _handle(problems, mode)
        want.append(_optimize(fresh, problems, mode, key))
        fresh.close()
        assert np.isfinite(want[-1][:, 0]).all()
    eager = _handle(problems, mode, options=("ACMPC_NO_GRAPH",))
    cached = _handle(problems, mode)
    for key in VISITS:
        np.testing.assert_array_equal(_optimize(cached, problems, mode, key), want[key], err_msg="cached, key %d" % key)
        np.testing.assert_array_equal(_optimize(eager, problems, mode, key), want[key], err_msg="eager, key %d" % key)
    # has_uref: the last key again without u_ref, then with it (both graphs are in the cache by then)
    fresh = _handle(problems, mode)
    bare = _optimize(fresh, problems, mode, 5, with_ref=False)
    fresh.close()
    for with_ref, expect in ((False, bare), (True, want[5]), (False, bare)):
        np.testing.assert_array_equal(_optimize(cached, problems, mode, 5, with_ref=with_ref), expect)
        np.testing.assert_array_equal(_optimize(eager, problems, mode, 5, with_ref=with_ref), expect)
    cached.close()
    eager.close()


def test_optimize_key_holds_the_plan_bit(problems):
    """lq_candidate = 1: a graph captured with the LQ plan as candidate 2 of its last round is not the graph of the same
    shape without one.  The plan needs the float64 tables of acmpc_set_paths; packed coefficients handed in for another
    shape drop them, so the same coefficients handed back leave the handle with the same device table and no plan."""
    sigma = (0.05, 1e-4)   # a narrow spread round the reference controls: the plan is what differs
    planned = _handle(problems, 0, lq_candidate=True)
    with_plan = _optimize(planned, problems, 0, 0, sigma=sigma)
    coef = np.stack([planned.coefficients(p) for p in range(P)])
    fresh = _handle(problems, 0, lq_candidate=True)
    np.testing.assert_array_equal(with_plan, _optimize(fresh, problems, 0, 0, sigma=sigma))
    fresh.close()
    plain = _handle(problems, 0)
    without = _optimize(plain, problems, 0, 0, sigma=sigma)
    plain.close()
    planned.set_coefficients(coef[:1])   # P = 1: the float64 tables of P = 2 go
    planned.set_coefficients(coef)       # the same packed tables again, now without float64 tables behind them
    np.testing.assert_array_equal(_optimize(planned, problems, 0, 0, sigma=sigma), without)
    planned.set_paths(problems["tables"])
    np.testing.assert_array_equal(_optimize(planned, problems, 0, 0, sigma=sigma), with_plan)
    assert not np.array_equal(with_plan, without), "the LQ plan changes nothing here: the pair shows nothing"
    planned.close()


def test_set_option_drops_the_captured_graphs(problems):
    """A captured graph holds the launch forms it was captured with: after a hit, ACMPC_NO_FUSED_FINALIZE=1 and the same
    shape give what a fresh handle with the option set gives, and the option taken back gives the first result again."""
    eng = _handle(problems, 0)
    first = _optimize(eng, problems, 0, 4)
    np.testing.assert_array_equal(_optimize(eng, problems, 0, 4), first)   # the hit
    eng.set_option("ACMPC_NO_FUSED_FINALIZE", "1")
    fresh = _handle(problems, 0, options=("ACMPC_NO_FUSED_FINALIZE",))
    np.testing.assert_array_equal(_optimize(eng, problems, 0, 4), _optimize(fresh, problems, 0, 4))
    fresh.close()
    eng.set_option("ACMPC_NO_FUSED_FINALIZE", None)
    np.testing.assert_array_equal(_optimize(eng, problems, 0, 4), first)
    eng.close()


# ---- acmpc_control_tick: P = 1, horizon 13

TICK_KEYS = [(N, rounds) for N in (256, 512) for rounds in (1, 2, 3)]


def _tick_engine(graph):
    from acmpc_amd import MODE_SPATIAL, Engine
    cfg = RACING["monza"]
    lim = orc.vehicle_limits(2.65, 1.94, 0.30, 8.0, 28.0)
    lo, hi = orc.input_box(lim)
    eng = Engine(mode=MODE_SPATIAL, max_problems=1, max_candidates=512, max_steps=n, step_cost=cfg["step_cost"],
                 r_term=cfg["r_term"], final_cost=cfg["final_cost"], u_min=lo, u_max=hi, margin=lim.margin,
                 wheelbase=lim.length, lq_candidate=0)
    if graph:
        eng.set_option("ACMPC_TICK_GRAPH", "1")
    return eng


def _tick(key, seed, map_index=None):
    from acmpc_amd import _capi
    cons = dict(RACING["monza"]["speed_profile_constraints"], v_max=28.0)
    t = _capi.Tick()
    t.struct_size = _capi.C.sizeof(_capi.Tick)
    t.horizon, t.localised, t.has_end_velocity = H, 0, 1
    t.n_candidates, t.rounds = TICK_KEYS[key]
    t.centre_is_reference = 1
    t.qp_max_iter, t.qp_check_every, t.qp_method = 4000, 10, 0
    t.offset = 0.05 * key
    t.v_min, t.v_max, t.a_min, t.a_max = cons["v_min"], cons["v_max"], cons["a_min"], cons["a_max"]
    t.ay_max, t.ki_min, t.end_velocity = cons["ay_max"], cons["ki_min"], cons["end_velocity"]
    t.sigma[0], t.sigma[1], t.shrink = 0.5, 1e-3, 0.5
    t.qp_eps_abs = t.qp_eps_rel = 1e-3
    t.seed = seed
    if map_index is not None:
        t.map_index, t.centreline_points = map_index, H * 38
    return t


def _same_tick(got, want, what):
    for field in ("record", "table", "info"):
        np.testing.assert_array_equal(got[field], want[field], err_msg="%s: %s" % (what, field))


def test_tick_graphs_through_more_keys_than_slots(golden):
    """ACMPC_TICK_GRAPH=1: six (n_candidates, rounds) keys on one handle, the first again (re-captured), the last (a
    hit) - record, table and info equal those of a handle without the switch (direct launches) fed the same ticks."""
    coords = np.ascontiguousarray(golden["monza_H20_hairpin_10/coords"][:H], dtype=np.float64)
    graphed, direct = _tick_engine(True), _tick_engine(False)
    for visit, key in enumerate(VISITS):
        got = graphed.control_tick(_tick(key, 40 + visit), coords, None)
        want = direct.control_tick(_tick(key, 40 + visit), coords, None)
        assert want["info"][4] == 0 and want["info"][7] == 0
        _same_tick(got, want, "visit %d (key %d)" % (visit, key))
    graphed.close()
    direct.close()


def test_rebinding_a_map_drops_every_captured_tick_graph():
    """A tick graph holds the map's address, length and window size: with two keys captured, binding another map and
    running both keys again gives what a fresh handle bound to that map gives."""
    from acmpc_amd import workloads
    first, second = workloads.synthetic_track("silverstone"), workloads.synthetic_track("monza")
    assert len(first["centre"]) != len(second["centre"])
    eng = _tick_engine(True)
    eng.bind_map(first["centre"], first["spacing"])
    for key in (0, 4):
        eng.control_tick(_tick(key, 60 + key, map_index=25), None, None)
    eng.bind_map(second["centre"], second["spacing"])
    fresh = _tick_engine(True)
    fresh.bind_map(second["centre"], second["spacing"])
    for key in (0, 4):
        got = eng.control_tick(_tick(key, 70 + key, map_index=25), None, None)
        want = fresh.control_tick(_tick(key, 70 + key, map_index=25), None, None)
        assert want["info"][6] == 25
        _same_tick(got, want, "key %d after the re-bind" % key)
        np.testing.assert_array_equal(got["coords"], want["coords"])
    eng.close()
    fresh.close()
