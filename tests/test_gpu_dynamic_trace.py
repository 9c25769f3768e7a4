"""Mode D's plan trace on the MI355X ("Mode D, plan trace"; csrc/acmpc_dynamic_trace.hip):
Engine.trace_plans bit for bit against the float32 restatement (tests/dynamic_spec.py's trace_plans) - states, totals and terms - at
the smallest shapes the kernel can go wrong at and once per step family; against the engine itself (the record of
Engine.optimize's winner, the costs of acmpc_rollout_device); the hinge replay; the scratch that regrows; and the plan built to
break one limit at one step."""
import numpy as np
import pytest

import acmpc_oracle as orc
import dynamic_fuzz_cases as fz
import dynamic_spec as ds
from dynamic_spec import Settings

pytestmark = pytest.mark.gpu

T = np.float32
INF = float("inf")
K_F, K_R = 7.35e-4, 1.1025e-3              # test_gpu_dynamic_downforce's: C_L A = 3.0 m^2, 40 % front, kN per (m/s)^2
RATE_SLIP = dict(rate_weight=(0.3, 0.02), rate_max=(1.5, 6.0), slip_weight=40.0, slip_max=0.08)
OBJECTIVE = dict(progress_weight=3.0, speed_ceiling=(0.98, 0.0))   # (below the start speed: the ceiling binds)
FAR = 3                                    # dynamic_fuzz_cases.KIND[3]: the path 3 km from the origin


def _case(n, P=1, K=1, window=None, seed=61000, **settings):
    """A case of tests/dynamic_fuzz_cases.py's kind: four candidates per problem to take plans from, the LAST problem's path
    far from the origin, everything off unless `settings` says so."""
    c = fz._longest("trace", window, "monza", 0, 4, seed=seed)
    c.update(H=n + 1, P=P, kinds=[p % 3 for p in range(P - 1)] + [FAR if P > 1 else 0], K=K, vehicles=list(range(K)),
             index="n%d" % n, aero=None, clearance=(0.0, 0.0))
    c.update(settings)
    return c


def _engine(c, dps):
    from acmpc_amd import Engine
    eng = Engine(**dict(dps[0]["kw"], max_problems=c["P"], max_candidates=64, max_steps=c["H"] - 1, nn_window=c["window"]))
    fz.apply(eng, c)
    eng.set_dynamics_downforce(c["aero"])
    eng.set_dynamics_clearance(*c["clearance"])
    eng.set_paths(np.stack([d["table"] for d in dps]))
    return eng


def _settings(c):
    return Settings.of_case(c, downforce=c["aero"], clearance_weight=c["clearance"][0], clearance_margin=c["clearance"][1])


def _plans(dps, M):
    """M plans per problem: candidates 1 .. 3 of the problem's four (2 and 3 leave the input box), or candidate 0 alone."""
    return np.stack([d["U"][1:4] if M == 3 else d["U"][:M] for d in dps])


def _want(c, eng, dps, U, discs=None):
    u_prev = fz.previous(c)
    vehicles = [fz.blocks()[v] for v in c["vehicles"]]
    per = [ds.trace_plans(dp, eng.coefficients(p), U[p], vehicles, _settings(c), c["window"],
                           None if u_prev is None else u_prev[p], None if discs is None else discs[p])
           for p, dp in enumerate(dps)]
    return {name: np.stack([t[name] for t in per]) for name in ("states", "totals", "terms")}


def _same(got, want, label):
    for name in ("states", "terms"):
        assert got[name].shape == want[name].shape, (label, name)
        diff = np.argwhere(ds.bits(got[name]) != ds.bits(want[name]))
        assert diff.size == 0, "%s: %s differs first at %s: %r != %r" % (label, name, diff[0], got[name][tuple(diff[0])],
                                                                        want[name][tuple(diff[0])])
    totals = np.stack([got["cost"], got["violation"]], axis=-1)
    assert np.array_equal(ds.bits(totals), ds.bits(want["totals"])), (label, totals, want["totals"])


def _replays(out, label):
    """V = fma(h, h, V) over slots 5 .. 19 from the previous step's V gives every step's V, and the last step's is V_k."""
    assert np.array_equal(ds.bits(ds.replay(out["terms"])), ds.bits(out["V"])), label
    assert np.array_equal(ds.bits(out["V"][..., -1]), ds.bits(out["violation"])), label


def run(c, M, K_obs=0, nans=None, narrow=False):
    dps = fz.problems(c, orc)
    if narrow:
        dps[0]["table"][orc.ROW_WIDTH] = 1.0   # metres: problem 0's plans leave the corridor
    eng = _engine(c, dps)
    try:
        discs = None
        if K_obs:
            n = c["H"] - 1
            discs = [ds.make_obstacles(d, n, K_obs, c["seed"] + 7 * p, nan=(nans or ["none"] * c["P"])[p]) for p, d in enumerate(dps)]
            eng.set_obstacles(np.stack([d[0] for d in discs]), np.stack([d[1] for d in discs]))
        U = _plans(dps, M)
        x0 = np.stack([d["x0"] for d in dps])
        got = eng.trace_plans(x0, U)
        label = "M %d K_obs %d | %s" % (M, K_obs, fz.label(c))
        want = _want(c, eng, dps, U, discs)
        _same(got, want, label)
        _replays(got, label)
        return got
    finally:
        eng.close()


# n: two steps is the least a table has; the lane-strided search wraps at 64; 512 is the LDS limit.  (2, 5) at n = 2: a window
# wider than the path.
SHAPES = [(2, 3, 3, 8, None), (2, 1, 1, 1, (2, 5)), (63, 1, 3, 2, (2, 5)), (64, 3, 1, 1, None), (65, 3, 3, 2, None),
          (65, 1, 1, 8, (2, 5)), (512, 1, 1, 1, None), (512, 1, 3, 1, (2, 5))]


@pytest.mark.parametrize("n,P,M,K,window", SHAPES)
def test_shapes_of_the_default_step(n, P, M, K, window):
    got = run(_case(n, P=P, K=K, window=window, seed=61000 + n), M)
    assert got["states"].shape == (P, M, K, n + 1, 6) and got["terms"].shape == (P, M, K, n, 22)
    if M == 3:
        assert np.any(got["box"] != 0), "plans 2 and 3 leave the input box"


FAMILIES = {
    "default": dict(),
    "fine": dict(M=4, blend=(3.0, 5.0)),
    "terms": dict(terms=RATE_SLIP, previous="finite"),
    "objective": dict(objective=OBJECTIVE),
    "coupled": dict(ratio=(INF, 0.9), terms=RATE_SLIP, objective=OBJECTIVE),
    "loaded": dict(load=(0.35, 0.9), M=2, blend=(3.0, 5.0), terms=RATE_SLIP, previous="finite"),
    "aero": dict(aero=(K_F, K_R, 100.0), ratio=(0.9, 1.1), load=(0.35, 0.9), objective=OBJECTIVE),
}


@pytest.mark.parametrize("window", [None, (2, 5)], ids=["all", "window"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_each_step_family(family, window):
    """Three problems (a narrow corridor, a standstill, a path far from the origin), three plans, two vehicles."""
    got = run(_case(9, P=3, K=2, window=window, seed=62000, **FAMILIES[family]), 3, narrow=True)
    on = FAMILIES[family]
    assert np.any(got["corridor"] != 0) and np.any(got["box"] != 0)
    if "terms" in on:
        assert np.any(got["rate"] != 0) or np.any(got["slip"] != 0)
        assert np.any(got["E"] != 0)
    else:
        assert not np.any(got["rate"]) and not np.any(got["slip"])
    assert np.any(got["ceiling"] != 0) == ("objective" in on)
    assert not np.any(got["obstacles"])


@pytest.mark.parametrize("base,K_obs", [("default", 1), ("aero", 8)])
def test_obstacles_over_a_step(base, K_obs):
    """Over the default step (the general step's kernels) and over the aero step; one disc with NaN coordinates at some steps;
    the soft part on."""
    c = _case(9, P=2, K=2, window=(2, 5), seed=63001, clearance=(40.0, 1.0), **FAMILIES[base])
    got = run(c, 3, K_obs=K_obs, nans=["some", "none"])
    assert np.any(got["obstacles"][..., :K_obs] != 0), "a plan enters a disc"
    assert not np.any(got["obstacles"][..., K_obs:])
    assert np.any(got["E"] != 0), "the soft part adds to E"


def test_the_scratch_regrows():
    """A small call, a larger one, the small one again on one handle: each is the specification."""
    c = _case(9, P=1, K=2, seed=64000)
    dps = fz.problems(c, orc)
    eng = _engine(c, dps)
    try:
        x0 = np.stack([d["x0"] for d in dps])
        small, large = _plans(dps, 1), np.tile(_plans(dps, 3), (1, 40, 1, 1))
        first = eng.trace_plans(x0, small)
        _same(first, _want(c, eng, dps, small), "small")
        big = eng.trace_plans(x0, large)
        _same({k: v[:, :3] for k, v in big.items()}, _want(c, eng, dps, large[:, :3]), "large")
        assert np.array_equal(ds.bits(big["terms"][:, :3]), ds.bits(big["terms"][:, 117:]))
        again = eng.trace_plans(x0, small)
        for name in ("states", "terms", "cost", "violation"):
            assert np.array_equal(ds.bits(again[name]), ds.bits(first[name])), name
        only = eng.trace_plans(x0, small, want=("totals",))
        assert only["states"] is None and only["terms"] is None
        assert np.array_equal(ds.bits(only["cost"]), ds.bits(first["cost"]))
    finally:
        eng.close()


@pytest.mark.parametrize("K,reduce", [(1, "mean"), (2, "max")])
@pytest.mark.parametrize("family", ["default", "coupled"])
def test_the_winner_of_optimize_is_its_record(family, K, reduce):
    """trace_plans on the u block of Engine.optimize's record: vehicle 0's (X, Y, yaw) is the record's x, and the totals are its
    cost and violation (K = 2 under the max: the larger of the two vehicles')."""
    c = _case(9, P=2, K=K, window=(2, 5), seed=65000, reduce=reduce, **FAMILIES[family])
    dps = fz.problems(c, orc)
    eng = _engine(c, dps)
    try:
        n = c["H"] - 1
        x0 = np.stack([d["x0"] for d in dps])
        centre = np.stack([d["U"][0] for d in dps])
        rec = eng.optimize(x0, centre, None, 64, 2, (0.05, 0.3), seed=7)
        u = np.ascontiguousarray(rec["u"], dtype=T).reshape(2, n, 2)
        got = eng.trace_plans(x0, u)
        assert np.array_equal(ds.bits(got["states"][:, 0, 0, :, :3]), ds.bits(np.asarray(rec["x"], dtype=T).reshape(2, n + 1, 3)))
        assert np.array_equal(ds.bits(got["cost"][:, 0].max(axis=1)), ds.bits(rec["cost"]))
        assert np.array_equal(ds.bits(got["violation"][:, 0].max(axis=1)), ds.bits(rec["violation"]))
    finally:
        eng.close()


@pytest.mark.parametrize("family", ["default", "terms", "aero"])
def test_totals_are_the_rollout_costs(family):
    """K = 1: the M candidates of a control matrix cost what acmpc_rollout_device says."""
    import torch
    c = _case(9, P=2, K=1, seed=66000, **FAMILIES[family])
    dps = fz.problems(c, orc)
    eng = _engine(c, dps)
    try:
        n = c["H"] - 1
        x0 = np.stack([d["x0"] for d in dps])
        U = np.stack([d["U"] for d in dps])
        got = eng.trace_plans(x0, U, want=("totals",))
        dev = torch.device("cuda:0")
        d_x0, d_U = torch.tensor(x0, device=dev), torch.tensor(U, device=dev)
        costs = torch.empty(2, 4, device=dev)
        eng.rollout_device(d_x0.data_ptr(), d_U.data_ptr(), 2, 4, n, 0, 0, costs.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(ds.bits(got["cost"][:, :, 0]), ds.bits(costs.cpu().numpy()))
    finally:
        eng.close()


def test_one_broken_limit_is_named():
    """A plan that breaks exactly one limit at one known step - the pedal outside the box at step 3: among slots 5 .. 19 of
    the whole trace only slot 6 of step 3 is not 0, and V is its square."""
    from acmpc_amd import _capi
    c = _case(12, seed=67000, terms=dict(rate_weight=(0.0, 0.0), rate_max=(50.0, 200.0), slip_weight=0.0, slip_max=5.0),
              objective=dict(progress_weight=0.0, speed_ceiling=(3.0, 0.0)))
    dps = fz.problems(c, orc)
    eng = _engine(c, dps)
    try:
        n = c["H"] - 1
        d_ref = np.arctan(float(dps[0]["kw"]["wheelbase"]) * dps[0]["table"][orc.ROW_KAPPA])[:n]
        u = np.stack([d_ref, np.full(n, 0.1)], axis=1).astype(T)
        u[3, 1] = T(1.25)                                   # the box is +-1
        got = eng.trace_plans(dps[0]["x0"][None], u[None])
        hinges = got["terms"][0, 0, 0][:, _capi.TRACE_HINGES]
        nonzero = np.argwhere(hinges != 0)
        assert nonzero.tolist() == [[3, 1]], nonzero
        excess = T(1.25) - T(1.0)
        assert got["box"][0, 0, 0, 3, 1] == excess
        assert got["violation"][0, 0, 0] == excess * excess
        assert np.array_equal(got["V"][0, 0, 0], np.where(np.arange(n) >= 3, excess * excess, 0).astype(T))
    finally:
        eng.close()
