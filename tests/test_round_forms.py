"""Which form a sampled round takes, as literal numbers (no GPU): `acmpc_describe_rounds` answers from the two host functions
the launches themselves ask (csrc: choose_sampled_form, plan_rounds), so the horizons and workgroup counts below are those at
which `acmpc_optimize` and `acmpc_control_tick` change kernels.  They follow from the LDS layouts (160 KiB per workgroup, 64
KiB for the re-rolling tail) and are fixed here on purpose: a change of layout fails this file, and whoever updates it moves
the cases of tests/test_gpu_round_forms.py, which sit on either side of every number, with it."""
import os
import re
import subprocess
import sys
import textwrap

import pytest

from acmpc_amd import MODE_SPATIAL, MODE_TEMPORAL, Engine, _capi
from acmpc_amd._capi import ROUND_PAIR, ROUND_QUAD, ROUND_SINGLE, ROUND_TRIO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("ACMPC_NO_QUAD_ROUNDS", "ACMPC_NO_PAIR_ROUNDS", "ACMPC_NO_TRIO_ROUNDS", "ACMPC_NO_CHAINED_ROUNDS",
            "ACMPC_NO_TRACED_FINALIZE", "ACMPC_NO_FUSED_FINALIZE", "ACMPC_NO_FUSED_SAMPLING", "ACMPC_NO_VERIFIED_SEARCH",
            "ACMPC_CONFORMANT_SYNC")


def _engine(mode, window=None, **extra):
    kw = dict(mode=mode, max_problems=8, max_candidates=70000, max_steps=1024, step_cost=[1.0, 1.0, 0.0], r_term=[1.0, 1.0],
              final_cost=[1.0, 0.0, 0.0], u_min=[0.0, -1.0], u_max=[30.0, 1.0], margin=0.5, wheelbase=2.65, nn_window=window)
    kw.update(extra)
    return Engine(**kw)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in SWITCHES:   # (a handle reads them when it is created)
        monkeypatch.delenv(name, raising=False)


def _last_and_first(eng, field, value, last, P=1, N=130):
    """`field` has `value` at n = last and no longer at last + 1."""
    assert eng.describe_rounds(P, N, last)[field] == value, "%s at n = %d" % (field, last)
    assert eng.describe_rounds(P, N, last + 1)[field] != value, "%s at n = %d" % (field, last + 1)


def test_mode_s_changes_form_at_117_120_and_682():
    eng = _engine(MODE_SPATIAL)
    _last_and_first(eng, "kernel", ROUND_QUAD, 117)
    _last_and_first(eng, "traced", True, 120)
    _last_and_first(eng, "fused_finalize", True, 682)
    for n in (1, 2, 49, 117):
        assert eng.describe_rounds(1, 130, n) == dict(kernel=ROUND_QUAD, fused_finalize=True, traced=True, chained=True,
                                                       frames_in_lds=False, frames_tabulated=False, tick_accepted=n >= 2,
                                                       tick_frames=False)
    for n, traced, fused in ((118, True, True), (120, True, True), (121, False, True), (682, False, True),
                             (683, False, False), (1024, False, False)):
        d = eng.describe_rounds(1, 130, n)
        assert (d["kernel"], d["traced"], d["chained"], d["fused_finalize"]) == (ROUND_SINGLE, traced, traced, fused), n
        assert not d["frames_in_lds"] and not d["frames_tabulated"] and not d["tick_frames"]
    eng.close()


def test_mode_t_with_the_exhaustive_search_changes_form_at_7_106_108_119_256_and_372():
    eng = _engine(MODE_TEMPORAL)
    _last_and_first(eng, "frames_in_lds", False, 7)
    _last_and_first(eng, "frames_tabulated", False, 7)
    _last_and_first(eng, "tick_frames", False, 7)
    _last_and_first(eng, "frames_in_lds", True, 106)
    _last_and_first(eng, "tick_frames", True, 106)
    _last_and_first(eng, "kernel", ROUND_TRIO, 108)
    _last_and_first(eng, "traced", True, 119)
    _last_and_first(eng, "chained", True, 119)
    _last_and_first(eng, "frames_tabulated", True, 256)
    _last_and_first(eng, "fused_finalize", True, 372)
    want = {7: (ROUND_TRIO, True, True, False, False), 8: (ROUND_TRIO, True, True, True, True),
            106: (ROUND_TRIO, True, True, True, True), 107: (ROUND_TRIO, True, True, False, True),
            108: (ROUND_TRIO, True, True, False, True), 109: (ROUND_SINGLE, True, True, False, True),
            119: (ROUND_SINGLE, True, True, False, True), 120: (ROUND_SINGLE, True, False, False, True),
            256: (ROUND_SINGLE, True, False, False, True), 257: (ROUND_SINGLE, True, False, False, False),
            372: (ROUND_SINGLE, True, False, False, False), 373: (ROUND_SINGLE, False, False, False, False)}
    for n, (kernel, fused, traced, in_lds, tabulated) in want.items():
        d = eng.describe_rounds(2, 130, n)
        assert (d["kernel"], d["fused_finalize"], d["traced"], d["frames_in_lds"], d["frames_tabulated"]) == \
            (kernel, fused, traced, in_lds, tabulated), n
        assert d["chained"] == traced and d["tick_frames"] == (in_lds and n <= 128)
    eng.close()


def test_mode_t_with_a_window_has_no_frames_and_changes_form_at_108_119_and_372():
    eng = _engine(MODE_TEMPORAL, (2, 5))
    _last_and_first(eng, "kernel", ROUND_TRIO, 108)
    _last_and_first(eng, "traced", True, 119)
    _last_and_first(eng, "fused_finalize", True, 372)
    for n in (2, 7, 8, 50, 106, 107, 108, 109, 119, 120, 128, 256, 257, 372, 373, 1024):
        d = eng.describe_rounds(1, 130, n)
        assert not d["frames_in_lds"] and not d["frames_tabulated"] and not d["tick_frames"], n
        assert d["kernel"] == (ROUND_TRIO if n <= 108 else ROUND_SINGLE), n
    eng.close()


@pytest.mark.parametrize("mode,window", [(MODE_SPATIAL, None), (MODE_TEMPORAL, None), (MODE_TEMPORAL, (2, 5))])
def test_the_tick_takes_2_to_128_steps(mode, window):
    eng = _engine(mode, window)
    _last_and_first(eng, "tick_accepted", False, 1)
    _last_and_first(eng, "tick_accepted", True, 128)
    eng.close()
    small = _engine(mode, window, max_steps=100, max_candidates=1000)   # ... within the handle's capacity
    assert small.describe_rounds(1, 1000, 100)["tick_accepted"]
    for shape in ((1, 1000, 101), (1, 1001, 50), (9, 1000, 50)):
        with pytest.raises(_capi.EngineError) as e:
            small.describe_rounds(*shape)
        assert e.value.code == _capi.ECAPACITY
    with pytest.raises(_capi.EngineError) as e:
        small.describe_rounds(1, 0, 50)
    assert e.value.code == _capi.EINVAL
    small.close()
    softmin = _engine(mode, window, centre_update="softmin")            # rounds through the control matrix, and no tick
    assert softmin.describe_rounds(1, 130, 50) == dict(kernel=-1, fused_finalize=False, traced=False, chained=False,
                                                        frames_in_lds=False, frames_tabulated=mode == 1 and window is None,
                                                        tick_accepted=False, tick_frames=False)
    softmin.close()


@pytest.mark.parametrize("mode,window,multi", [(MODE_SPATIAL, None, ROUND_QUAD), (MODE_TEMPORAL, None, ROUND_TRIO),
                                               (MODE_TEMPORAL, (2, 5), ROUND_TRIO)])
def test_workgroup_count_limits(mode, window, multi):
    """Chained while a problem has at most 256 workgroups, traced while the launch has at most 1024."""
    eng = _engine(mode, window)
    n = 20
    for P, N, traced, chained in ((1, 16384, True, True), (1, 16385, True, False), (1, 16448, True, False),
                                  (4, 16384, True, True), (4, 16385, False, False), (8, 8192, True, True),
                                  (8, 8193, False, False), (1, 65536, True, False), (1, 65537, False, False)):
        d = eng.describe_rounds(P, N, n)
        assert (d["traced"], d["chained"], d["fused_finalize"]) == (traced, chained, True), (P, N)
        assert d["kernel"] == (multi if traced else ROUND_SINGLE), (P, N)   # the multi-wave rounds are traced rounds
        assert d["frames_in_lds"] == (traced and mode == 1 and window is None), (P, N)
    eng.close()


def test_mode_d_has_no_such_rounds():
    eng = _engine(_capi.MODE_DYNAMIC, max_steps=512)
    with pytest.raises(_capi.EngineError) as e:
        eng.describe_rounds(1, 130, 50)
    assert e.value.code == _capi.ESTATE
    eng.close()


def test_mode_s_switches(monkeypatch):
    """As launch_rollout_sampled reads them: without the quad form the pair form up to 115 steps and - there being no
    third multi-wave form - the single wave at 116 and 117, where the quad form would have fitted; the pair switch takes both."""
    monkeypatch.setenv("ACMPC_NO_QUAD_ROUNDS", "1")
    eng = _engine(MODE_SPATIAL)
    _last_and_first(eng, "kernel", ROUND_PAIR, 115)
    for n, kernel in ((2, ROUND_PAIR), (115, ROUND_PAIR), (116, ROUND_SINGLE), (117, ROUND_SINGLE), (118, ROUND_SINGLE)):
        d = eng.describe_rounds(1, 1000, n)
        assert (d["kernel"], d["traced"], d["chained"]) == (kernel, True, True), n
    eng.close()
    monkeypatch.delenv("ACMPC_NO_QUAD_ROUNDS")
    monkeypatch.setenv("ACMPC_NO_PAIR_ROUNDS", "1")
    eng = _engine(MODE_SPATIAL)
    for n in (2, 50, 115, 117, 120):
        d = eng.describe_rounds(1, 1000, n)
        assert (d["kernel"], d["traced"], d["chained"]) == (ROUND_SINGLE, True, True), n
    eng.close()
    monkeypatch.delenv("ACMPC_NO_PAIR_ROUNDS")
    eng = _engine(MODE_SPATIAL)   # ... and set_option moves a live handle the same way
    assert eng.describe_rounds(1, 1000, 115)["kernel"] == ROUND_QUAD
    eng.set_option("ACMPC_NO_QUAD_ROUNDS", 1)
    assert eng.describe_rounds(1, 1000, 115)["kernel"] == ROUND_PAIR
    assert eng.describe_rounds(1, 1000, 116)["kernel"] == ROUND_SINGLE
    eng.set_option("ACMPC_NO_QUAD_ROUNDS", None)
    assert eng.describe_rounds(1, 1000, 116)["kernel"] == ROUND_QUAD
    eng.close()


def test_mode_t_switches(monkeypatch):
    monkeypatch.setenv("ACMPC_NO_TRIO_ROUNDS", "1")
    eng = _engine(MODE_TEMPORAL)
    for n in (7, 8, 106, 108, 119):   # one wave, which takes no frames: the tick tabulates none
        d = eng.describe_rounds(1, 1000, n)
        assert (d["kernel"], d["traced"], d["frames_in_lds"], d["tick_frames"]) == (ROUND_SINGLE, True, False, False), n
        assert d["frames_tabulated"] == (n >= 8)
    eng.close()
    monkeypatch.delenv("ACMPC_NO_TRIO_ROUNDS")
    monkeypatch.setenv("ACMPC_NO_VERIFIED_SEARCH", "1")
    eng = _engine(MODE_TEMPORAL)
    for n in (8, 106, 107, 108):      # three waves that scan every waypoint
        d = eng.describe_rounds(1, 1000, n)
        assert (d["kernel"], d["frames_in_lds"], d["frames_tabulated"], d["tick_frames"]) == (ROUND_TRIO, False, True, False), n
    assert eng.describe_rounds(1, 1000, 109)["kernel"] == ROUND_SINGLE
    eng.close()


@pytest.mark.parametrize("mode,multi", [(MODE_SPATIAL, ROUND_QUAD), (MODE_TEMPORAL, ROUND_TRIO)])
def test_finalize_switches(mode, multi, monkeypatch):
    def describe(n=50, P=1, N=1000):
        eng = _engine(mode)
        out = eng.describe_rounds(P, N, n)
        eng.close()
        return out["kernel"], out["fused_finalize"], out["traced"], out["chained"]

    assert describe() == (multi, True, True, True)
    monkeypatch.setenv("ACMPC_NO_CHAINED_ROUNDS", "1")
    assert describe() == (multi, True, True, False)
    monkeypatch.setenv("ACMPC_NO_TRACED_FINALIZE", "1")      # the multi-wave forms are traced forms
    assert describe() == (ROUND_SINGLE, True, False, False)
    monkeypatch.delenv("ACMPC_NO_CHAINED_ROUNDS")
    assert describe() == (ROUND_SINGLE, True, False, False)
    monkeypatch.delenv("ACMPC_NO_TRACED_FINALIZE")
    monkeypatch.setenv("ACMPC_NO_FUSED_FINALIZE", "1")       # a finalize launch behind every round
    assert describe() == (ROUND_SINGLE, False, False, False)
    monkeypatch.delenv("ACMPC_NO_FUSED_FINALIZE")
    monkeypatch.setenv("ACMPC_CONFORMANT_SYNC", "1")         # ... which the conformant forms are
    assert describe() == (ROUND_SINGLE, False, False, False)
    monkeypatch.delenv("ACMPC_CONFORMANT_SYNC")
    monkeypatch.setenv("ACMPC_NO_FUSED_SAMPLING", "1")       # sample -> rollout -> finalize through the matrix
    assert describe() == (-1, False, False, False)


def test_the_query_does_not_open_the_device():
    """With the HIP runtime logging its API calls (AMD_LOG_LEVEL), a process that creates handles of both modes, asks for
    their round forms and destroys them logs nothing: no HIP call was made, so the runtime was never initialised.  The
    same process then makes a compute call, whose first HIP call shows up - the log does see one when there is one."""
    script = textwrap.dedent("""
        import sys
        sys.path[:0] = [%r, %r]
        import numpy as np
        from acmpc_amd import Engine, _capi
        kw = dict(max_problems=2, max_candidates=1000, max_steps=128, step_cost=[1.0, 1.0, 0.0], r_term=[1.0, 1.0],
                  final_cost=[1.0, 0.0, 0.0], u_min=[0.0, -1.0], u_max=[30.0, 1.0], margin=0.5, wheelbase=2.65)
        for mode, n in ((0, 117), (0, 121), (1, 106), (1, 109), (1, 128)):
            eng = Engine(mode=mode, **kw)
            assert eng.describe_rounds(2, 130, n)["tick_accepted"]
            eng.close()
        sys.stderr.write("== queried ==\\n")
        sys.stderr.flush()
        eng = Engine(mode=0, **kw)
        eng.set_paths(np.ones((1, 7, 10)))
        try:
            eng.optimize(np.zeros((1, 3)), np.ones((1, 10, 2)), None, 64, 1, (1.0, 0.01))
        except _capi.EngineError as e:
            assert e.code == _capi.ENODEVICE
        sys.stderr.write("== computed ==\\n")
    """) % (os.path.join(ROOT, "ac-mpc_amd"), os.path.join(ROOT, "oracle"))
    env = dict(os.environ, AMD_LOG_LEVEL="4")
    proc = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-2000:]
    before, mark, after = proc.stderr.partition("== queried ==\n")
    assert mark and "== computed ==" in after, proc.stderr[-2000:]
    assert not re.search(r"^:\d:", before, re.M) and "hipGetDeviceCount" not in before, before[-2000:]
    assert "hipGetDeviceCount" in after, after[-2000:]
