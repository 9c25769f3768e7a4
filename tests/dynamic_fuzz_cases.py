"""The cases of tests/test_gpu_fuzz_dynamic_settings.py: test_gpu_fuzz_dynamic._case's draw - layout, horizon, candidates,
problems, window, track, problem kinds, ensemble, reduce, weights - with every mode D setting of the handle and the call
form drawn beside it.  A helper of the tests, not a test file; it runs no device code (the test modules it borrows lists and
vehicles from import theirs only inside their tests).  tests/test_dynamic_fuzz_cases.py holds what keeps the fuzz from
passing vacuously: the coverage of the committed seed, that every part that is on changes something, and that every setting
is one the handle takes.

A case names a target FAMILY, the kernels the dispatch of csrc/acmpc_dynamic.hip (launch_rollout_dynamic and its two
siblings) picks from the handle's state, highest rank first:

    loaded      load transfer on                            TermsLoaded     csrc/acmpc_dynamic_loaded.hip
    coupled     coupling on                                 TermsCoupled    csrc/acmpc_dynamic_coupled.hip
    objective   progress or ceiling on                      TermsObjective  csrc/acmpc_dynamic_terms.hip
    terms       a rate or slip part on                      Terms           csrc/acmpc_dynamic_terms.hip
    fine        set_dynamics_integration != (1, None)       FINE = true     csrc/acmpc_dynamic.hip

The family's own setting is on, every setting that outranks it is off, and the settings ranked below it are drawn freely
(`family_of` restates the dispatch).  Under `coupled` and `loaded` the four parts of the cost - rate, slip, progress,
ceiling - follow PATTERNS by the case's slot, so that each is on alone, all are off, the limits run without the weights and
the rate part runs with no previous control at least once per family, and each one-sided ratio appears under both.

A case is `case(family, form, index)`: seeded by (SEED, family, form, index, attempt), where `attempt` counts the re-draws
REDRAWN lists - cases whose first draw had a part that changed nothing on its first 32 candidates (a slip limit no candidate
reaches, a ceiling above every speed).  tests/test_dynamic_fuzz_cases.py checks that table.

The NumPy restatement costs about  P K n (0.3 ms + 2.8 ms M + N (2.3 us + 2.8 us M + 80 ns W))  on one core (measured with
the loaded step, the coupled and the plain one are within a tenth of it; W waypoints searched per step): test_gpu_fuzz_
dynamic's estimate with the step taken M times.  A case above BUDGET_S gives up problems first, then vehicles, then
sub-steps, then candidates - never its horizon, window, layout, family or which parts are on."""
from __future__ import annotations

import numpy as np

import dynamic_sampled_spec as dss
import dynamic_spec as ds
from dynamic_spec import Settings

T = np.float32
INF = float("inf")
SEED = 20261019
DEFAULT_CASES = 6                       # per family and form; ACMPC_FUZZ_CASES scales it
BUDGET_S = 1.0
FAMILIES = ("fine", "terms", "objective", "coupled", "loaded")
FORMS = ("matrix", "sampled")

# test_gpu_fuzz_dynamic's lists (kept equal to them by tests/test_dynamic_fuzz_cases.py)
HORIZONS = [3, 4, 9, 17, 33, 50, 65, 66, 100, 130, 257, 513]
CANDIDATES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1000, 2049]
WINDOWS = [None, (2, 5), (1, 2), (0, 2), (3, 12), (20, 43)]
TRACKS = ["monza", "spa", "nordschleife", "silverstone"]
ENSEMBLE_SIZES = [1, 1, 2, 3, 5, 8]
BIG_OFFSET = 3_000_000_013              # test_gpu_dynamic_sampled.BIG_OFFSET
SAMPLED_MIN_N = 63                      # the smallest N the sampled forms have been launched with
BLENDS = [None, (3.0, 5.0), (0.0, 8.0)]
SUBSTEPS_P = np.array([4.0] * 5 + [1.0] * 11) / 31.0          # 1 .. 16, weighted towards 1 .. 5
# test_gpu_dynamic_terms.SETTINGS' values: a weight scaled by one of SCALES, a limit by one of LIMIT_SCALES - downwards, to
# where the candidates of most cases reach it (a limit nothing reaches is a part that runs and changes nothing)
RATE_WEIGHT, RATE_MAX, SLIP_WEIGHT, SLIP_MAX = (0.3, 0.02), (1.5, 6.0), 40.0, 0.08
SCALES = (0.5, 1.0, 2.0)
LIMIT_SCALES = (0.1, 0.25, 1.0)
PROGRESS = (0.0, 3.0, 400.0)
CEILINGS = (None, 0.9, (1.05, 0.0), (1.0, 0.3))
SIGMAS = ((0.04, 0.35), (0.05, 0.6))
SETTERS = ("vehicles", "integration", "terms", "previous", "objective", "coupling", "load")

# Under `coupled` and `loaded`, slot = 2 index + (form == "sampled"), modulo 12: which of (rate weight, rate limit, slip
# weight, slip limit, progress, ceiling) are on (None: drawn), the previous control (None: drawn) and the coupling's ratio
# ("front": (inf, rho), "rear": (rho, inf), None: drawn).
PATTERNS = {
    0: ((1, 0, 0, 0, 0, 0), "finite", None),        # rate alone
    1: ((0, 0, 1, 0, 0, 0), None, "front"),         # slip alone
    2: ((0, 0, 0, 0, 1, 0), None, "rear"),          # progress alone: the finish that skips E
    3: ((0, 0, 0, 0, 0, 1), None, "front"),         # ceiling alone
    4: ((0, 0, 0, 0, 0, 0), None, None),            # all off
    5: ((0, 1, 0, 1, 0, 0), "finite", "rear"),      # the limits without the weights
    6: ((1, 0, 0, 0, 0, 0), "none", None),          # rate with no previous control
    7: ((0, 0, 0, 1, 1, 0), None, None),            # the slip limit and the progress
}


def fleet():
    """The vehicles a case's `vehicles` index: test_gpu_dynamic_ensemble._vehicles() (0 .. 7), then the three members of
    test_gpu_dynamic_load_transfer._geometry_vehicles() that are not vehicle 0 (8 .. 10)."""
    import test_gpu_dynamic_ensemble as tge
    import test_gpu_dynamic_load_transfer as tgl
    return tge._vehicles() + tgl._geometry_vehicles()[1:]


_blocks = []


def blocks():
    if not _blocks:
        _blocks.extend(v.coefficients() for v in fleet())
    return _blocks


def accepts(block, ratio, load):
    """What acmpc_set_dynamics_coupling / _load_transfer ask of a vehicle: finite positive float32 peaks while either is on,
    and under the load transfer N_a != 0 and a peak factor phi_a > 0 at x = +-w_max and at its vertex inside."""
    if ratio is None and load is None:
        return True
    k = ds.derived_constants(block)
    if not all(np.isfinite(k[p]) and k[p] > 0 for p in ("Pf", "Pr")):
        return False
    if load is None:
        return True
    c = ds.constants64(block, load)
    if not (np.isfinite(c["c_h"]) and np.isfinite(c["w_max"])):
        return False
    for a in "fr":
        a1, a2 = c["a1_" + a], c["a2_" + a]
        if not (np.isfinite(a1) and np.isfinite(a2)):
            return False
        probes = [-c["w_max"], c["w_max"]]
        if a2 > 0.0 and -c["w_max"] < -a1 / (2 * a2) < c["w_max"]:
            probes.append(-a1 / (2 * a2))
        if not all(1 + x * (a1 + a2 * x) > 0.0 for x in probes):
            return False
    return True


def spec_seconds(c):
    n = c["H"] - 1
    W = n if c["window"] is None else min(c["window"][0] + c["window"][1] + 1, n)
    M = c["M"]
    return c["P"] * c["K"] * n * (0.3e-3 + 2.8e-3 * M + c["N"] * (2.3e-6 + 2.8e-6 * M + 8.0e-8 * W))


def parts(c):
    """Which parts of the cost are on, as the kernels' switches see them."""
    t = ds.constants(None, Settings(**c["terms"]))
    return dict(rate=t.rate, slip=t.slip, progress=float(c["objective"]["progress_weight"]) != 0.0,
                ceiling=c["objective"]["speed_ceiling"] is not None)


def integration_on(c):
    return c["M"] != 1 or c["blend"] is not None


def family_of(c):
    """The dispatch of csrc/acmpc_dynamic.hip restated: the kernel family the handle's state selects."""
    on = parts(c)
    if c["load"] is not None:
        return "loaded"
    if c["ratio"] is not None:
        return "coupled"
    if on["progress"] or on["ceiling"]:
        return "objective"
    if on["rate"] or on["slip"]:
        return "terms"
    return "fine" if integration_on(c) else "plain"


def _scaled(rng, value, scales=SCALES):
    return float(value) * scales[int(rng.integers(0, 3))]


def _limit_pair(rng):
    """(rd_max, rp_max): each None, inf or a value - one of them at least a value."""
    pair = [[None, INF, _scaled(rng, v, LIMIT_SCALES), _scaled(rng, v, LIMIT_SCALES)][int(rng.integers(0, 4))] for v in RATE_MAX]
    if not any(v is not None and np.isfinite(v) for v in pair):
        q = int(rng.integers(0, 2))
        pair[q] = _scaled(rng, RATE_MAX[q], LIMIT_SCALES)
    return tuple(pair)


def _terms(rng, switches):
    rw, rl, sw, sl = switches
    return dict(rate_weight=(_scaled(rng, RATE_WEIGHT[0]), _scaled(rng, RATE_WEIGHT[1])) if rw else (0.0, 0.0),
                rate_max=_limit_pair(rng) if rl else (None, (INF, INF), (None, None))[int(rng.integers(0, 3))],
                slip_weight=_scaled(rng, SLIP_WEIGHT) if sw else 0.0,
                slip_max=_scaled(rng, SLIP_MAX, LIMIT_SCALES) if sl else (None, INF)[int(rng.integers(0, 2))])


def _ratio(rng, choice):
    rho = float(rng.uniform(0.7, 1.2))
    if choice == "front":
        return (INF, rho)
    if choice == "rear":
        return (rho, INF)
    return [rho, (0.9, 1.1), (INF, rho), (rho, INF), (INF, INF)][int(choice)]


def _load(rng):
    h, w = float(rng.uniform(0.2, 0.6)), float(rng.uniform(0.3, 0.95))
    return [h, (h, w), (h, 0.9), (0.0, w)][int(rng.integers(0, 4))]


def _settings(rng, family, slot):
    """The handle's settings of one case: everything that outranks `family` off, its own on, the rest drawn."""
    rank = FAMILIES.index(family)
    c = {}
    pattern = PATTERNS.get(slot % 12) if rank >= 3 else None
    # integration
    c["M"] = int(rng.choice(np.arange(1, 17), p=SUBSTEPS_P))
    c["blend"] = BLENDS[int(rng.integers(0, 3))]
    if family == "fine" and c["M"] == 1 and c["blend"] is None:
        c["blend"] = BLENDS[1 + int(rng.integers(0, 2))]
    if slot % 12 == 4:                                  # (index 2 of the matrix form: M > 1 with the blend, for certain)
        c["M"] = int(rng.integers(2, 6))
        c["blend"] = BLENDS[1 + int(rng.integers(0, 2))]
    # terms and objective
    switches = [int(v) for v in rng.integers(0, 2, 4)]
    progress = PROGRESS[int(rng.integers(0, 3))]
    ceiling = CEILINGS[int(rng.integers(0, 4))]
    if pattern is not None:
        switches = list(pattern[0][:4])
        progress = PROGRESS[1 + int(rng.integers(0, 2))] if pattern[0][4] else 0.0
        ceiling = CEILINGS[1 + int(rng.integers(0, 3))] if pattern[0][5] else None
    if rank < 1:
        switches = [0, 0, 0, 0]
    if rank < 2:
        progress, ceiling = 0.0, None
    if family == "terms" and not any(switches):
        switches[int(rng.integers(0, 4))] = 1
    if family == "objective" and progress == 0.0 and ceiling is None:
        if rng.integers(0, 2):
            progress = PROGRESS[1 + int(rng.integers(0, 2))]
        else:
            ceiling = CEILINGS[1 + int(rng.integers(0, 3))]
    c["terms"] = _terms(rng, switches)
    c["objective"] = dict(progress_weight=progress, speed_ceiling=ceiling)
    # the previous control: none set, finite, or (where the existing tests show it legal: the terms' own kernels, the rate
    # part off beside a slip part, or both rate weights on) a NaN steering in one problem
    t = ds.constants(None, Settings(**c["terms"]))
    choices = ["none", "finite"]
    if family == "terms" and ((not t.rate and t.slip) or (t.hwd != 0 and t.hwp != 0)):
        choices.append("nan")
    c["previous"] = choices[int(rng.integers(0, len(choices)))]
    if pattern is not None and pattern[1] is not None:
        c["previous"] = pattern[1]
    # coupling and load transfer
    c["ratio"] = c["load"] = None
    if rank >= 3:
        choice = int(rng.integers(0, 5))
        if family == "loaded" and rng.integers(0, 4) == 0:
            choice = None
        if pattern is not None and pattern[2] is not None:
            choice = pattern[2]
        c["ratio"] = None if choice is None else _ratio(rng, choice)
    if family == "loaded":
        c["load"] = _load(rng)
    return c


def _vehicles(rng, c, K):
    """K vehicles the settings accept (the eight of test_gpu_dynamic_ensemble; under the load transfer the geometry members
    too, so that the six scalars differ per vehicle)."""
    pool = range(11) if c["load"] is not None else range(8)
    pool = [v for v in pool if accepts(blocks()[v], c["ratio"], c["load"])]
    picked = [int(pool[i]) for i in rng.permutation(len(pool))]
    return picked[:min(K, len(picked))]


def case(family, form, index, attempt=None):
    """Case `index` of (family, form) as a plain dict."""
    if attempt is None:
        attempt = REDRAWN.get((family, form, index), 0)
    rng = np.random.default_rng([SEED, FAMILIES.index(family), FORMS.index(form), index, attempt])
    slot = 2 * index + FORMS.index(form)
    c = dict(family=family, form=form, index=index, attempt=attempt, layout=int(rng.integers(0, 2)))
    H = int(rng.choice(HORIZONS))
    if index % DEFAULT_CASES in (1, 2):                 # the cases that keep K > 1 and M > 1 whatever the budget says
        H = int(rng.choice([h for h in HORIZONS if h <= (50 if index % DEFAULT_CASES == 1 else 66)]))
    N = int(rng.choice(CANDIDATES if H <= 130 else [v for v in CANDIDATES if v <= 257]))
    if form == "sampled":
        N = max(N, SAMPLED_MIN_N)
    P = int(rng.integers(1, 5))
    window = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
    track = TRACKS[int(rng.integers(0, 4))]
    kinds = [int(k) for k in rng.integers(0, 4, 4)]
    K = int(rng.choice(ENSEMBLE_SIZES))
    if index % DEFAULT_CASES == 0:
        K = 1
    elif index % DEFAULT_CASES == 1:
        K = int(rng.choice([2, 3, 5]))
    reduce = ["mean", "max"][int(rng.integers(0, 2))]
    weights = [float(x) for x in rng.uniform(0.2, 3.0, 8)] if rng.integers(0, 2) else None
    c.update(H=H, N=N, P=P, window=window, track=track, K=K, reduce=reduce)
    c.update(_settings(rng, family, slot))
    if index % DEFAULT_CASES == 1:
        c["M"] = min(c["M"], 2)
    vehicles = _vehicles(rng, c, 8)
    c["K"] = K = min(K, len(vehicles))
    while spec_seconds(c) > BUDGET_S:
        if c["P"] > 1:
            c["P"] -= 1
        elif c["K"] > 1:
            c["K"] = max(k for k in ENSEMBLE_SIZES if k < c["K"])
        elif c["M"] > 1 + (c["blend"] is None and family == "fine"):
            c["M"] -= 1
        elif c["N"] > (SAMPLED_MIN_N if form == "sampled" else 1):
            c["N"] = max(v for v in CANDIDATES if v < c["N"])
        else:
            break
    c["kinds"] = kinds[:c["P"]]
    c["vehicles"] = vehicles[:c["K"]]
    c["weights"] = None if weights is None else weights[:c["K"]]
    c["order"] = [SETTERS[i] for i in rng.permutation(len(SETTERS))]
    c["seed"] = 30000 + 1000 * FAMILIES.index(family) + 100 * FORMS.index(form) + 10 * index
    c["plant"] = form == "matrix" and index % 3 == 1
    if form == "sampled":
        c.update(round=int(rng.integers(0, 6)), with_ref=bool(rng.integers(0, 2)),
                 index_offset=(0, BIG_OFFSET)[int(rng.integers(0, 2))], sigma=SIGMAS[int(rng.integers(0, 2))],
                 sample_seed=int(rng.integers(1, 1 << 40)))
    return c


def cases(family, form, count=DEFAULT_CASES):
    return [case(family, form, index) for index in range(count)]


def previous(c):
    """The [P, 2] previous controls of a case (test_gpu_dynamic_terms._previous), or None."""
    if c["previous"] == "none":
        return None
    rng = np.random.default_rng(8800 + c["seed"])
    u = np.column_stack([rng.uniform(-0.1, 0.1, c["P"]), rng.uniform(-0.3, 0.5, c["P"])]).astype(T)
    if c["previous"] == "nan":
        u[c["P"] - 1, 0] = np.nan
    return u


def apply(eng, c, order=None):
    """The case's settings through the handle's public setters, in the drawn order (or `order`)."""
    vehicles = [fleet()[v] for v in c["vehicles"]]
    calls = dict(
        vehicles=lambda: eng.set_dynamics(vehicles[0]) if c["K"] == 1 else
        eng.set_dynamics_ensemble(vehicles, weights=c["weights"], reduce=c["reduce"]),
        integration=lambda: eng.set_dynamics_integration(c["M"], c["blend"]),
        terms=lambda: eng.set_dynamics_terms(**c["terms"]),
        previous=lambda: eng.set_previous_control(previous(c)),
        objective=lambda: eng.set_dynamics_objective(**c["objective"]),
        coupling=lambda: eng.set_dynamics_coupling(c["ratio"]),
        load=lambda: eng.set_dynamics_load_transfer(c["load"]))
    for name in (c["order"] if order is None else order):
        calls[name]()


def label(c):
    return ("%s %s %s: layout %d H %d N %d P %d window %s %s kinds %s K %d vehicles %s %s weights %s | M %d blend %s terms %s "
            "previous %s objective %s ratio %s load %s order %s" % (
                c["family"], c["form"], c["index"], c["layout"], c["H"], c["N"], c["P"], c["window"], c["track"], c["kinds"],
                c["K"], c["vehicles"], c["reduce"], c["weights"], c["M"], c["blend"], c["terms"], c["previous"], c["objective"],
                c["ratio"], c["load"], c["order"])
            + (" | round %d ref %s offset %d sigma %s" % (c["round"], c["with_ref"], c["index_offset"], c["sigma"])
               if c["form"] == "sampled" else ""))


def _longest(family, window, track, kind, N, **settings):
    c = dict(family=family, form="matrix", index="longest", attempt=0, layout=0, H=513, N=N, P=1, window=window, track=track,
             kinds=[kind], K=1, vehicles=[0], reduce="mean", weights=None, M=1, blend=None,
             terms=dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=None), previous="none",
             objective=dict(progress_weight=0.0, speed_ceiling=None), ratio=None, load=None, order=list(SETTERS), plant=False)
    c.update(settings)
    return c


# the longest horizon the kernels accept (kDynamicMaxSteps = 512 steps), one restatement for both layouts
LONGEST = [
    _longest("objective", None, "monza", 0, 17, seed=39000, previous="finite",
             terms=dict(rate_weight=(0.3, 0.02), rate_max=(1.5, None), slip_weight=40.0, slip_max=None),
             objective=dict(progress_weight=3.0, speed_ceiling=(1.05, 0.0))),
    _longest("coupled", (20, 43), "silverstone", 3, 33, seed=39010, ratio=(INF, 0.9),
             terms=dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=0.08),
             objective=dict(progress_weight=400.0, speed_ceiling=None)),
    _longest("loaded", None, "silverstone", 2, 9, seed=39020, ratio=(0.9, 1.1), load=(0.35, 0.9), previous="finite",
             terms=dict(rate_weight=(0.3, 0.02), rate_max=None, slip_weight=0.0, slip_max=None),
             objective=dict(progress_weight=0.0, speed_ceiling=(1.0, 0.3))),
    _longest("loaded", (20, 43), "monza", 0, 65, seed=39030, ratio=None, load=(0.5, 0.6),
             objective=dict(progress_weight=3.0, speed_ceiling=None)),
]


def packed_cases():
    """Two cases per family of (terms, coupled, loaded) for the two-candidates-per-lane launch of test_gpu_dynamic_packed
    (N = 4099, n = 4): the drawn settings, K in (1, 3), a layout and a window.  P follows from N and K there."""
    out = []
    for family in ("terms", "coupled", "loaded"):
        for q in range(2):
            rng = np.random.default_rng([SEED, FAMILIES.index(family), 7, q])
            c = dict(family=family, form="packed", index=q, K=(1, 3)[q], layout=int(rng.integers(0, 2)),
                     window=(None, (2, 5))[int(rng.integers(0, 2))])
            c.update(_settings(rng, family, (5, 7, 1, 2, 3, 0)[2 * (FAMILIES.index(family) % 3) + q]))
            c["M"] = min(c["M"], 4)
            if c["previous"] == "nan":
                c["previous"] = "finite"
            out.append(c)
    return out


def identification_cases():
    """Four (ratio, load, integration, L, K) cases of acmpc_score_grips: a one-sided ratio each way and a zero height first,
    two drawn ones after them.  K is 25 (tied scales) or 625 (split)."""
    rng = np.random.default_rng([SEED, 99])
    out = [dict(ratio=(INF, 1.1), load=(0.35, 0.9), integration=(1, None), L=8, K=625),
           dict(ratio=(0.8, INF), load=(0.0, 0.7), integration=(4, (3.0, 5.0)), L=1, K=25)]
    for _ in range(2):
        out.append(dict(ratio=_ratio(rng, int(rng.integers(0, 4))), load=_load(rng),
                        integration=(int(rng.integers(1, 6)), BLENDS[int(rng.integers(0, 3))]),
                        L=int(rng.choice([1, 5, 8, 40])), K=int(rng.choice([25, 625]))))
    return out


# ---- the composed restatement of a case ------------------------------------------------------------------------------------
KIND = [dict(), dict(vx0=0.0), dict(yaw_turns=-1), dict(origin=(3000.0, 2700.0))]   # test_gpu_dynamic._problems' four


def problems(c, orc, limit=None):
    """The case's problems: for the matrix form test_gpu_fuzz_dynamic._problems' (N candidates each, or the first `limit`;
    with non-finite candidates planted where the case says so), for the sampled form test_gpu_dynamic_sampled.Rig's (whose
    own four candidates are not used)."""
    N = 4 if c["form"] == "sampled" else c["N"]
    out = [ds.make_dynamic_problem(orc, c["track"], c["H"], N, c["seed"] + p, **KIND[kind]) for p, kind in enumerate(c["kinds"])]
    if c["form"] == "matrix":
        if c["plant"] and c["N"] > 8:
            n = c["H"] - 1
            out[0]["U"][5, n // 2, 0] = np.nan
            out[0]["U"][7, 0, 1] = np.inf
        if limit is not None:
            for d in out:
                d["U"] = d["U"][:limit]
    return out


def centres(c, orc, dps):
    """(centre [P, n, 2], u_ref [P, n, 2] or None) of a sampled case: test_gpu_dynamic_sampled.Rig's construction."""
    n = c["H"] - 1
    rng = np.random.default_rng(777 + c["seed"])
    L = float(dps[0]["kw"]["wheelbase"])
    centre, ref = np.empty((c["P"], n, 2), dtype=T), np.empty((c["P"], n, 2), dtype=T)
    for p, d in enumerate(dps):
        d_ref = np.arctan(L * d["table"][orc.ROW_KAPPA])[:n]
        centre[p, :, 0] = d_ref + rng.normal(0.0, 0.01, n)
        centre[p, :, 1] = rng.uniform(-0.1, 0.4)
        ref[p, :, 0] = d_ref
        ref[p, :, 1] = 0.15
    return centre, (ref if c["with_ref"] else None)


def specification(c, orc, dps, coefs, centre=None, ref=None, limit=None, without=(), only=None, obstacles=None,
                  clearance=(0.0, 0.0)):
    """What the kernels must give for case `c`, per problem.  Matrix form: (cost, V, states).  Sampled form: dynamic_sampled_
    spec.rollout_sampled's dict.  `limit`: the first candidates only; `without`: Settings.without's parts; `only`: these
    problems only; `obstacles`: per problem (positions [n, K, 2], radii [K]) or None, under `clearance` = (weight, margin)."""
    vehicles = [blocks()[v] for v in c["vehicles"]]
    u_prev = previous(c)
    settings = Settings.of_case(c, clearance_weight=clearance[0], clearance_margin=clearance[1]).without(*without)
    N = c["N"] if limit is None else min(c["N"], limit)
    out = []
    for p in (range(len(dps)) if only is None else only):
        dp, coef = dps[p], coefs[p]
        kwargs = dict(settings=settings, u_prev=None if u_prev is None else u_prev[p],
                      obstacles=None if obstacles is None else obstacles[p])
        if c["form"] == "sampled":
            out.append(dss.rollout_sampled(orc, dp, coef, vehicles, centre[p], None if ref is None else ref[p], N,
                                           c["index_offset"], p, c["round"], c["sample_seed"], c["sigma"], reduce=c["reduce"],
                                           weights=c["weights"], nn_window=c["window"], return_states=True, **kwargs))
        else:
            out.append(dss.costs(orc, dp, coef, vehicles, dp["U"][:N], c["reduce"], c["weights"], c["window"],
                                 return_states=True, **kwargs))
    return out


# (family, form, index) -> attempt of the cases whose first draw did not pass "every switch bites": 9 of the committed seed's
# 60 cases, 15 % (tests/test_dynamic_fuzz_cases.py's __main__ finds them; its tests hold the table and the 25 % cap).  Every
# one was a slip limit, a rate limit or a ceiling no candidate of the problem looked at reached, or a progress reward on a
# problem that starts at a standstill.
REDRAWN = {("terms", "matrix", 2): 1, ("terms", "matrix", 4): 1, ("terms", "matrix", 5): 1, ("terms", "sampled", 0): 1,
           ("terms", "sampled", 4): 1, ("objective", "matrix", 2): 2, ("objective", "matrix", 4): 1,
           ("objective", "sampled", 2): 4, ("objective", "sampled", 5): 1}
