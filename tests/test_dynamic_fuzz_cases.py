"""The generator of tests/test_gpu_fuzz_dynamic_settings.py's cases (tests/dynamic_fuzz_cases.py) on the CPU: what keeps that
fuzz from passing vacuously, for the committed seed and the default case count.

  coverage    every family with both forms and with K = 1 and K > 1; under `coupled` and again under `loaded` each of rate,
              slip, progress and ceiling on alone, all four off, each one-sided ratio; M > 1 with the blend in every family;
              and the dispatch restated in Python names the target family for every case.
  bites       on the first 32 candidates of one problem (the one with the NaN previous control where a case has one, else
              problem 0) every part that is on changes a cost or a violation against the same case without it, and the
              coupling or load transfer changes a cost - where it can: (inf, inf) and a height of 0 are identities (test_gpu_
              dynamic_coupling / _load_transfer hold them) and are not asked to.  dynamic_fuzz_cases.REDRAWN lists the cases
              that needed another draw; the share is capped at 25 %.
              Measured on the committed seed: 9 of 60 cases re-drawn, 15 % (`python tests/test_dynamic_fuzz_cases.py` finds
              the table and prints it with the coverage counts).
  legality    every case's restatement runs (the bites test calls it), and a handle takes every drawn setting in the drawn
              order: the argument checks run without a device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "ac-mpc_amd"), os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acmpc_oracle as orc  # noqa: E402
import dynamic_fuzz_cases as fz  # noqa: E402

T = np.float32
BITES_CANDIDATES = 32
REDRAWN_CAP = 0.25
PAIRS = [(family, form) for family in fz.FAMILIES for form in fz.FORMS]


def _all_cases():
    return [c for family, form in PAIRS for c in fz.cases(family, form)]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=T)).view(np.uint32)


def test_the_lists_are_the_parent_fuzz_lists():
    import test_gpu_dynamic_sampled as tsm
    import test_gpu_fuzz_dynamic as tfd
    for name in ("HORIZONS", "CANDIDATES", "WINDOWS", "TRACKS", "ENSEMBLE_SIZES", "KIND"):
        assert getattr(fz, name) == getattr(tfd, name), name
    assert fz.BIG_OFFSET == tsm.BIG_OFFSET


def coverage():
    """The counts the summary quotes: per family and form, and per part under the coupled and loaded families."""
    rows = {}
    for c in _all_cases():
        on = fz.parts(c)
        alone = [name for name in on if on[name]]
        row = rows.setdefault(c["family"], dict(matrix=0, sampled=0, K1=0, Kmany=0, fine_blend=0, all_off=0, front_inf=0,
                                                rear_inf=0, both_inf=0, rate_alone=0, slip_alone=0, progress_alone=0,
                                                ceiling_alone=0, rate=0, slip=0, progress=0, ceiling=0, no_previous_rate=0,
                                                limits_only=0, zero_height=0, H513=0))
        row[c["form"]] += 1
        row["K1" if c["K"] == 1 else "Kmany"] += 1
        row["fine_blend"] += c["M"] > 1 and c["blend"] is not None
        row["all_off"] += not alone
        row["H513"] += c["H"] == 513
        for name in alone:
            row[name] += 1
        if len(alone) == 1:
            row[alone[0] + "_alone"] += 1
        t = fz.ds.constants(None, fz.Settings(**c["terms"]))
        row["no_previous_rate"] += t.rate and c["previous"] == "none"
        row["limits_only"] += (t.rate or t.slip) and t.hwd == 0 and t.hwp == 0 and t.hws == 0
        if c["ratio"] is not None and np.ndim(c["ratio"]) == 1:
            f, r = (np.isinf(v) for v in c["ratio"])
            row["front_inf"] += f and not r
            row["rear_inf"] += r and not f
            row["both_inf"] += f and r
        row["zero_height"] += c["load"] is not None and np.ndim(c["load"]) == 1 and c["load"][0] == 0.0
    return rows


def test_coverage_of_the_committed_seed():
    rows = coverage()
    for family, row in rows.items():
        print(family, row)
    assert set(rows) == set(fz.FAMILIES)
    for family, form in PAIRS:
        cs = fz.cases(family, form)
        assert len(cs) == fz.DEFAULT_CASES
        assert any(c["K"] == 1 for c in cs) and any(c["K"] > 1 for c in cs), (family, form)
        for c in cs:
            assert fz.family_of(c) == family, fz.label(c)
            assert fz.spec_seconds(c) <= fz.BUDGET_S or (c["P"], c["K"]) == (1, 1), fz.label(c)
            assert len(c["vehicles"]) == c["K"] and len(c["kinds"]) == c["P"]
    for family, row in rows.items():
        assert row["fine_blend"] >= 1, family
    for family in ("coupled", "loaded"):
        row = rows[family]
        for key in ("rate_alone", "slip_alone", "progress_alone", "ceiling_alone", "all_off", "front_inf", "rear_inf",
                    "no_previous_rate", "limits_only"):
            assert row[key] >= 1, (family, key)
    for c in fz.LONGEST:
        assert c["H"] == 513 and (c["P"], c["M"], c["K"]) == (1, 1, 1) and c["window"] in (None, (20, 43))
        assert fz.family_of(c) == c["family"]
    assert {c["family"] for c in fz.LONGEST} == {"objective", "coupled", "loaded"}
    for c in fz.packed_cases():
        assert fz.family_of(c) == c["family"], c
    ident = fz.identification_cases()
    assert len(ident) == 4 and ident[0]["ratio"][0] == fz.INF and ident[1]["ratio"][1] == fz.INF and ident[1]["load"][0] == 0.0


def _inputs(c):
    dps = fz.problems(c, orc, limit=BITES_CANDIDATES)
    coefs = [orc.coefficients_temporal(d["table"], d["kw"]["margin"]).astype(T) for d in dps]
    centre, ref = fz.centres(c, orc, dps) if c["form"] == "sampled" else (None, None)
    return dps, coefs, centre, ref


def _outcome(c, inputs, without=()):
    p = c["P"] - 1 if c["previous"] == "nan" else 0
    out = fz.specification(c, orc, *inputs, limit=BITES_CANDIDATES, without=without, only=[p])[0]
    return (out["cost"], out["violation"]) if c["form"] == "sampled" else (out[0], out[1])


def idle_parts(c):
    """The parts of case `c` that are on and change nothing (an empty list: every switch bites)."""
    inputs = _inputs(c)
    base = _outcome(c, inputs)
    names = [name for name, on in fz.parts(c).items() if on]
    acts = (c["ratio"] is not None and np.isfinite(np.asarray(c["ratio"], dtype=float)).any()) or \
        (c["load"] is not None and float(np.ravel(c["load"])[0]) > 0.0)
    idle = []
    for name in names + (["step"] if acts else []):
        other = _outcome(c, inputs, without=(name,))
        same_cost = np.array_equal(_bits(base[0]), _bits(other[0]))
        if same_cost and (name == "step" or np.array_equal(_bits(base[1]), _bits(other[1]))):
            idle.append(name)
    return idle


@pytest.mark.parametrize("family,form", PAIRS)
def test_every_switch_bites(family, form):
    for c in fz.cases(family, form):
        assert idle_parts(c) == [], fz.label(c)


def test_the_share_of_redrawn_cases():
    total = len(PAIRS) * fz.DEFAULT_CASES
    for (family, form, index), attempt in fz.REDRAWN.items():
        assert family in fz.FAMILIES and form in fz.FORMS and 0 <= index < fz.DEFAULT_CASES and attempt >= 1
    print("re-drawn: %d of %d cases" % (len(fz.REDRAWN), total))
    assert len(fz.REDRAWN) <= REDRAWN_CAP * total


def test_a_handle_takes_every_drawn_setting_in_the_drawn_order():
    from acmpc_amd import Engine
    import dynamic_spec as ds
    dp = ds.make_dynamic_problem(orc, "monza", 20, 8, 0)
    todo = _all_cases() + fz.LONGEST
    for c in todo:
        eng = Engine(**dict(dp["kw"], max_problems=c["P"]))
        try:
            fz.apply(eng, c)
            fz.apply(eng, c, order=list(reversed(c["order"])))
        finally:
            eng.close()
        for v in c["vehicles"]:
            assert fz.accepts(fz.blocks()[v], c["ratio"], c["load"])
    eng = Engine(**dp["kw"])
    try:
        eng.set_dynamics(fz.fleet()[0])
        for c in fz.packed_cases():
            fz.apply(eng, dict(c, vehicles=[0]), order=[s for s in fz.SETTERS if s not in ("vehicles", "previous")])
        for c in fz.identification_cases():
            eng.set_dynamics_integration(*c["integration"])
            eng.set_dynamics_coupling(c["ratio"])
            eng.set_dynamics_load_transfer(c["load"])
    finally:
        eng.close()
    # accepts() agrees with the handle on every vehicle of the fleet, for a mild and a severe setting
    for load in ((0.35, 0.9), (0.6, 0.95), (5.0, 0.99)):
        for v, vehicle in enumerate(fz.fleet()):
            eng = Engine(**dp["kw"])
            try:
                eng.set_dynamics(vehicle)
                try:
                    eng.set_dynamics_load_transfer(load)
                    taken = True
                except Exception:
                    taken = False
                assert taken == fz.accepts(fz.blocks()[v], None, load), (v, load)
            finally:
                eng.close()


def test_the_comparison_fails_on_a_broken_restatement(monkeypatch):
    """The fuzz can fail: test_gpu_fuzz_dynamic_settings.check_solve on a stored solve (built here from the restatement, which
    the kernels equal) passes against the restatement and fails against one that drops E - the finish that a wrong
    `if (!kObjective || rate || slip)` would take with the progress on beside the rate weights - and against one that takes
    the progress with the wrong sign."""
    from acmpc_amd import _capi
    import dynamic_spec as ds
    import test_gpu_fuzz_dynamic_settings as tfs
    c = dict(fz.LONGEST[0], H=9, N=24, seed=39100)          # rate weights, a slip weight, progress 3 and a ceiling
    n = c["H"] - 1
    dps, coefs, _, _ = _inputs(c)
    want = fz.specification(c, orc, dps, coefs)
    U = np.stack([d["U"] for d in dps])
    records = np.zeros((1, _capi.record_floats(n)), dtype=T)
    cost, V, X = want[0]
    best = orc.pick_best(cost)[0]
    records[0, :4] = cost[best], V[best], np.count_nonzero(V == 0), 1.0
    records[0, 4:4 + 2 * n] = U[0][best].ravel()
    records[0, 4 + 2 * n:] = X[best].ravel()
    stored = dict(costs=cost[None], best_idx=np.array([best]), n_feasible=np.array([np.count_nonzero(V == 0)]), records=records)
    tfs.check_solve(stored, U, want, n, "stored")
    step_terms = ds.step_terms
    with monkeypatch.context() as m:
        m.setattr(ds, "step_terms", lambda c_, st, d, p, pd, pp, E, V_, row=None: (E, step_terms(c_, st, d, p, pd, pp, E, V_, row)[1]))
        dropped = fz.specification(c, orc, dps, coefs)
    assert np.array_equal(_bits(dropped[0][1]), _bits(V))    # (V is untouched: only the cost can tell)
    with pytest.raises(AssertionError, match="costs"):
        tfs.check_solve(stored, U, dropped, n, "stored")
    constants = ds.constants
    with monkeypatch.context() as m:
        m.setattr(ds, "constants", lambda *a: (lambda o: setattr(o, "nwp", -o.nwp) or o)(constants(*a)))
        flipped = fz.specification(c, orc, dps, coefs)
    with pytest.raises(AssertionError, match="costs"):
        tfs.check_solve(stored, U, flipped, n, "stored")
    assert tfs.check_solve(stored, U, fz.specification(c, orc, dps, coefs), n, "stored") is None   # (and everything is put back)


if __name__ == "__main__":
    redrawn = {}
    for family, form in PAIRS:
        for index in range(fz.DEFAULT_CASES):
            attempt = 0
            while True:
                idle = idle_parts(fz.case(family, form, index, attempt))
                if not idle:
                    break
                print("%s %s %d attempt %d: idle %s" % (family, form, index, attempt, idle))
                attempt += 1
            if attempt:
                redrawn[family, form, index] = attempt
    print("REDRAWN = %r" % redrawn)
    print("re-drawn share: %d / %d" % (len(redrawn), len(PAIRS) * fz.DEFAULT_CASES))
    for family, row in coverage().items():
        print(family, row)
