"""Which launch a rollout over a caller's control matrix takes, as literal numbers (no GPU): `acmpc_describe_rollout` answers
from the host functions the launches themselves ask (csrc: choose_shape, tailed_rollout_fits, chained_rollout_fits,
tile_rows_table_in_lds, solo_fits), so the sizes below are those at which `acmpc_rollout_device`, `acmpc_solve_device`, the
sampled solve and the stream of batches change kernels.  They are fixed here on purpose: a changed heuristic or LDS layout
fails this file first, and whoever updates it moves the cases of tests/test_gpu_rollout_shapes.py, which run either side of
every number on the device, with it."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from acmpc_amd import MODE_SPATIAL, MODE_TEMPORAL, Engine, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("ACMPC_SHAPE", "ACMPC_T_PACK", "ACMPC_NO_TILE", "ACMPC_TILE_ROWS", "ACMPC_TILE_TABLE", "ACMPC_NO_SOLO",
            "ACMPC_TAILED_ROLLOUT", "ACMPC_NO_CHAINED_STREAM", "ACMPC_CONFORMANT_SYNC")
CM, SM = 0, 1
S, T = MODE_SPATIAL, MODE_TEMPORAL


def _engine(mode, window=None, **extra):
    kw = dict(mode=mode, max_problems=65535, max_candidates=1 << 21, max_steps=256, step_cost=[1.0, 1.0, 0.0],
              r_term=[1.0, 1.0], final_cost=[1.0, 0.0, 0.0], u_min=[0.0, -1.0], u_max=[30.0, 1.0], margin=0.5,
              wheelbase=2.65, nn_window=window)
    kw.update(extra)
    return Engine(**kw)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in SWITCHES:   # (a handle reads them when it is created)
        monkeypatch.delenv(name, raising=False)


def _form(eng, P, N, n, layout):
    d = eng.describe_rollout(P, N, n, layout)
    return d["kernel"], d["block"], d["cpt"], d["pack"], d["workgroups"]


@pytest.mark.parametrize("mode", [S, T])
@pytest.mark.parametrize("layout,n", [(SM, 8), (SM, 200), (CM, 129)])   # (candidate-major past the tile's horizons: the same rule)
def test_64_thread_workgroups_up_to_131072_candidates(mode, layout, n):
    eng = _engine(mode)
    for P, N in ((1, 1), (1, 64), (1, 65), (1, 131071), (32, 4096), (2, 65536), (32768, 4)):
        assert _form(eng, P, N, n, layout) == ("step", 64, 1, 1, (N + 63) // 64), (P, N)
    for P, N in ((1, 131073), (33, 3973), (3, 43691), (11, 11917)):   # odd N: one candidate per lane in both modes
        assert P * N > 131072
        assert _form(eng, P, N, n, layout) == ("step", 256, 1, 1, (N + 255) // 256), (P, N)
    eng.close()


def test_mode_s_takes_four_candidates_per_lane_from_1048576_candidates_with_n_a_multiple_of_four():
    eng = _engine(S)
    for n in (2, 49, 200):
        for P, N in ((256, 4096), (1, 1048576), (4096, 4096), (257, 4096), (1024, 1028), (2, 524288), (263, 3988)):
            assert P * N >= 1048576 and N % 4 == 0
            assert _form(eng, P, N, n, SM) == ("step", 256, 4, 2, (N + 1023) // 1024), (P, N)
        # 1 048 572 candidates, N a multiple of four: one short
        for P, N in ((255, 4096), (1, 1048572), (3, 349524), (33, 4096), (65535, 16)):
            assert P * N < 1048576 and P * N > 131072 and N % 4 == 0
            assert _form(eng, P, N, n, SM) == ("step", 256, 1, 1, (N + 255) // 256), (P, N)
        # 1 M candidates and more, N not a multiple of four: mode S never takes two per lane by itself
        for P, N in ((256, 4098), (1, 1048578), (1, 1048577), (257, 4095), (2048, 514), (4096, 4094), (256, 4097)):
            assert P * N >= 1048576 and N % 4 != 0
            assert _form(eng, P, N, n, SM) == ("step", 256, 1, 1, (N + 255) // 256), (P, N)
    assert _form(eng, 3, 349524, 8, SM)[2] == 1 and 3 * 349524 == 1048572
    eng.close()


@pytest.mark.parametrize("window", [None, (2, 5), (1, 2)])
def test_mode_t_takes_two_candidates_per_lane_for_even_n_and_one_for_odd(window):
    eng = _engine(T, window)
    for n in (2, 49, 200):
        for P, N in ((33, 4096), (1, 131074), (256, 4096), (1, 1048576), (4096, 4096), (2048, 514)):   # (never four by itself)
            assert _form(eng, P, N, n, SM) == ("step", 256, 2, 1, (N + 511) // 512), (P, N)
        for P, N in ((33, 4095), (1, 131073), (257, 4095), (1, 1048577)):
            assert _form(eng, P, N, n, SM) == ("step", 256, 1, 1, (N + 255) // 256), (P, N)
        assert _form(eng, 32, 4096, n, SM) == ("step", 64, 1, 1, 64)
    eng.close()


def test_the_candidate_major_tile_ends_at_128_steps_in_mode_s_and_113_in_mode_t():
    """64 rows of 2n floats, and in mode T the waypoint and key tables behind them, in 64 KiB of LDS."""
    for mode, last in ((S, 128), (T, 113)):
        eng = _engine(mode)
        for P, N in ((1, 1), (2, 65), (3, 1000), (40, 8192)):
            for n in (1, 2, 49, 81, last - 1, last):
                kernel = "rows" if (mode == S and n <= 80 and (P, N) == (40, 8192)) else "tile"   # (5 120 tiles: see below)
                assert _form(eng, P, N, n, CM) == (kernel, 64, 1, 1, (N + 63) // 64), (mode, P, N, n)
            for n in (last + 1, last + 2, 256):
                big = P * N > 131072
                assert _form(eng, P, N, n, CM) == ("step", 256 if big else 64, 1, 1, (N + (255 if big else 63)) // (256 if big else 64)), \
                    (mode, P, N, n)
        d = eng.describe_rollout(2, 65, last, CM)
        assert not d["tailed_fits"] and not d["chained_fits"]   # (both are step-major forms)
        eng.close()


def test_the_rows_kernel_from_2048_tiles_up_to_80_steps_on_spans_that_start_on_16_bytes():
    eng = _engine(S)
    rows = lambda P, N, n: eng.describe_rollout(P, N, n, CM)["kernel"] == "rows"
    # 2047 | 2048 tiles of 64 candidates
    for P, N, want in ((32, 4096, True), (31, 4096, False), (32, 4095, True), (32, 4032, False), (1, 131072, True),
                       (1, 131008, False), (1, 131009, True), (2048, 1, True), (2047, 1, False), (2048, 64, True),
                       (1024, 65, True), (1023, 128, False), (683, 129, True), (682, 192, False)):
        assert rows(P, N, 8) == want, (P, N)
        assert eng.describe_rollout(P, N, 8, CM)["workgroups"] == (N + 63) // 64   # partial keys per problem, either kernel
    # 80 | 81 steps at 2048 tiles
    for n, want in ((1, True), (32, True), (33, True), (50, True), (64, True), (79, True), (80, True), (81, False), (128, False)):
        assert rows(32, 4096, n) == want, n
        assert eng.describe_rollout(32, 4096, n, CM)["kernel"] == ("rows" if want else "tile")
    # several problems: every problem's span must start on a 16-byte boundary, 2 N n floats a multiple of four
    for P, N, n, want in ((2048, 65, 3, False), (2048, 65, 4, True), (2048, 66, 3, True), (2048, 67, 79, False),
                          (1, 131073, 3, True), (1, 131073, 79, True), (2, 65537, 3, False), (2, 65538, 3, True)):
        assert (2 * N * n) % 4 == (2 if P == 1 else 0 if want else 2)   # (one problem: its span starts where the matrix does)
        assert rows(P, N, n) == want, (P, N, n)
    eng.close()
    eng = _engine(T)   # mode T never takes it
    for P, N, n in ((32, 4096, 8), (2048, 64, 49), (1, 131072, 80), (4096, 4096, 8)):
        assert _form(eng, P, N, n, CM) == ("tile", 64, 1, 1, (N + 63) // 64)
    eng.set_option("ACMPC_TILE_ROWS", 4)
    assert _form(eng, 32, 4096, 8, CM)[0] == "tile"
    eng.close()


def test_the_rows_kernels_table_comes_from_lds_between_33_and_50_steps_and_from_512_problems():
    eng = _engine(S)
    table = lambda P, N, n: eng.describe_rollout(P, N, n, CM)["table"]
    for P, N, n, want in ((32, 4096, 8, "scalar"), (32, 4096, 32, "scalar"), (32, 4096, 33, "lds"), (32, 4096, 50, "lds"),
                          (32, 4096, 51, "scalar"), (32, 4096, 80, "scalar"), (511, 4096, 51, "scalar"), (512, 4096, 51, "lds"),
                          (512, 256, 80, "lds"), (511, 320, 80, "scalar"), (512, 256, 32, "scalar"), (4096, 4096, 49, "lds")):
        assert table(P, N, n) == want, (P, N, n)
    assert table(31, 4096, 49) is None and table(32, 4096, 81) is None   # (not the rows kernel)
    for value, want in (("lds", "lds"), ("scalar", "scalar"), (None, "scalar")):
        eng.set_option("ACMPC_TILE_TABLE", value)
        assert table(32, 4096, 8) == want
    for value, want in (("lds", "lds"), ("scalar", "scalar"), (None, "lds")):
        eng.set_option("ACMPC_TILE_TABLE", value)
        assert table(32, 4096, 49) == want
    eng.close()


ACCEPTED = {"64,1": (64, 1), "256,1": (256, 1), "256,2": (256, 2), "256,4": (256, 4)}
IGNORED = ("128,1", "64,2", "64,4", "256,3", "256,8", "512,1", "0,0", "256", "256;4", "wide", "", "4,256", "-64,1")


@pytest.mark.parametrize("mode", [S, T])
def test_every_forced_shape_and_those_the_rule_ignores(mode):
    eng = _engine(mode)
    pack = lambda cpt: 2 if (mode == S and cpt >= 2) else 1
    for P, N in ((1, 4), (3, 1028), (2, 2048), (256, 4096), (33, 4096)):           # N a multiple of four: all four take
        for value, (block, cpt) in ACCEPTED.items():
            eng.set_option("ACMPC_SHAPE", value)
            assert _form(eng, P, N, 8, SM) == ("step", block, cpt, pack(cpt), (N + block * cpt - 1) // (block * cpt)), (value, P, N)
    eng.set_option("ACMPC_SHAPE", None)
    default = {(P, N): _form(eng, P, N, 8, SM) for P, N in ((1, 6), (1, 510), (1, 511), (3, 1027), (300, 4098), (300, 4097))}
    for (P, N), want in default.items():
        for value in IGNORED:
            eng.set_option("ACMPC_SHAPE", value)
            assert _form(eng, P, N, 8, SM) == want, (value, P, N)
        eng.set_option("ACMPC_SHAPE", "256,4")     # N not a multiple of four
        assert _form(eng, P, N, 8, SM) == want, (P, N)
        eng.set_option("ACMPC_SHAPE", "256,2")
        assert _form(eng, P, N, 8, SM) == (("step", 256, 2, pack(2), (N + 511) // 512) if N % 2 == 0 else want), (P, N)
    # candidate-major: the tile takes no shape; past it (and with ACMPC_NO_TILE) one candidate per lane only
    for value in ("64,1", "256,1", "256,2", "256,4"):
        eng.set_option("ACMPC_SHAPE", value)
        assert _form(eng, 2, 2048, 8, CM) == ("tile", 64, 1, 1, 32), value
    eng.set_option("ACMPC_NO_TILE", 1)
    for value, want in (("64,1", ("step", 64, 1, 1, 32)), ("256,1", ("step", 256, 1, 1, 8)), ("256,2", ("step", 64, 1, 1, 32)),
                        ("256,4", ("step", 64, 1, 1, 32)), (None, ("step", 64, 1, 1, 32))):
        eng.set_option("ACMPC_SHAPE", value)
        assert _form(eng, 2, 2048, 8, CM) == want, value
        assert _form(eng, 2, 2048, 200, CM) == want, value
    eng.close()


def test_the_environment_sets_what_set_option_sets(monkeypatch):
    monkeypatch.setenv("ACMPC_SHAPE", "256,4")
    monkeypatch.setenv("ACMPC_NO_TILE", "1")
    eng = _engine(S)
    assert _form(eng, 1, 1028, 8, SM) == ("step", 256, 4, 2, 2)
    assert _form(eng, 1, 1026, 8, SM) == ("step", 64, 1, 1, 17)
    assert _form(eng, 1, 1028, 8, CM) == ("step", 64, 1, 1, 17)
    eng.set_option("ACMPC_NO_TILE", None)
    assert _form(eng, 1, 1028, 8, CM) == ("tile", 64, 1, 1, 17)
    eng.close()


def test_no_tile_and_tile_rows():
    eng = _engine(S)
    assert _form(eng, 32, 4096, 8, CM)[0] == "rows"
    eng.set_option("ACMPC_TILE_ROWS", 0)
    assert _form(eng, 32, 4096, 8, CM) == ("tile", 64, 1, 1, 64)
    eng.set_option("ACMPC_TILE_ROWS", 4)
    assert _form(eng, 32, 4096, 8, CM) == ("rows", 64, 1, 1, 64)
    for P, N, n in ((31, 4096, 8), (32, 4096, 81), (2048, 65, 3)):   # ... which forces nothing outside the kernel's gate
        assert _form(eng, P, N, n, CM)[0] == "tile", (P, N, n)
    eng.set_option("ACMPC_NO_TILE", 1)
    assert _form(eng, 32, 4096, 8, CM) == ("step", 64, 1, 1, 64)
    assert _form(eng, 33, 4096, 8, CM) == ("step", 256, 1, 1, 16)
    assert _form(eng, 256, 4096, 8, CM) == ("step", 256, 1, 1, 16)     # (no multi-candidate lanes on this layout)
    eng.set_option("ACMPC_NO_TILE", 0)
    eng.set_option("ACMPC_TILE_ROWS", None)
    assert _form(eng, 32, 4096, 8, CM)[0] == "rows"
    eng.close()
    eng = _engine(T)
    eng.set_option("ACMPC_NO_TILE", 1)
    assert _form(eng, 33, 4096, 8, CM) == ("step", 256, 1, 1, 16)
    eng.close()


def test_t_pack_moves_mode_t_alone():
    eng = _engine(T)
    for value, want in ((None, 1), (2, 2), (1, 1), (2, 2), (None, 1)):
        eng.set_option("ACMPC_T_PACK", value)
        assert _form(eng, 33, 4096, 8, SM) == ("step", 256, 2, want, 8), value
        assert _form(eng, 33, 4095, 8, SM) == ("step", 256, 1, 1, 16), value      # one candidate per lane: nothing to pack
        eng.set_option("ACMPC_SHAPE", "256,4")
        assert _form(eng, 3, 1028, 8, SM) == ("step", 256, 4, want, 2), value
        eng.set_option("ACMPC_SHAPE", None)
    eng.close()
    eng = _engine(S)
    for value in (None, 1, 2):
        eng.set_option("ACMPC_T_PACK", value)
        assert _form(eng, 256, 4096, 8, SM) == ("step", 256, 4, 2, 4), value
    eng.close()


def test_the_tailed_and_the_chained_fits_at_each_lane_width():
    """Both are mode S's, step-major, on the 256-thread shapes; the chained stream also needs the pending finalize's LDS
    image (four problems per workgroup) within 20 KiB - 59 steps - and one grid row of finalize per problem at the most."""
    eng = _engine(S)
    fits = lambda P, N, n, layout=SM: (eng.describe_rollout(P, N, n, layout)["tailed_fits"], eng.describe_rollout(P, N, n, layout)["chained_fits"])
    assert fits(32, 4096, 49) == (False, False)       # 64-thread workgroups
    assert fits(33, 4096, 49) == (True, True)         # 256 x 1
    assert fits(256, 4096, 49) == (True, True)        # 256 x 4 by the default rule (the benchmark's batch: 4096 x 4096)
    assert fits(4096, 4096, 49) == (True, True)
    assert fits(256, 4098, 49) == (True, True)        # 256 x 1 at 1 M
    assert fits(33, 4096, 49, CM) == (False, False)
    for value, cpt in ACCEPTED.items():
        eng.set_option("ACMPC_SHAPE", value)
        for P, N in ((1, 4), (3, 1028), (3, 2052), (64, 4096)):
            assert eng.describe_rollout(P, N, 19, SM)["cpt"] == cpt[1]
            assert fits(P, N, 19) == ((True, True) if cpt[0] == 256 else (False, False)), (value, P, N)
        for n, chained in ((2, True), (58, True), (59, True), (60, False), (79, False), (200, False)):
            assert fits(3, 1028, n) == ((True, chained) if cpt[0] == 256 else (False, False)), (value, n)
    eng.set_option("ACMPC_SHAPE", None)
    # the pending finalize takes four problems per workgroup, in grid rows behind the rollout's: P + rows <= 65 535
    assert _form(eng, 52428, 256, 8, SM) == ("step", 256, 4, 2, 1)
    assert fits(52428, 256, 8) == (True, True)        # one workgroup per row: 52 428 + 13 107 rows
    assert fits(52429, 256, 8) == (True, False)       # 52 429 + 13 108
    assert fits(52429, 2048, 8) == (True, True)       # two workgroups per row: 52 429 + 6 554
    eng.close()
    eng = _engine(T)
    for value in (None, "256,1", "256,2", "256,4"):
        eng.set_option("ACMPC_SHAPE", value)
        assert fits(64, 4096, 19) == (False, False), value
    eng.close()


def test_the_one_launch_solve_is_reported():
    """`acmpc_solve_device` and `acmpc_solve` do not make the described launch where the one-launch solve takes the problem:
    mode S, up to 1 024 workgroups of 64 candidates in all."""
    eng = _engine(S)
    solo = lambda P, N, n=8, layout=SM: eng.describe_rollout(P, N, n, layout)["solo"]
    assert solo(1, 4) and solo(1, 65536) and solo(16, 4096) and solo(3, 1028) and solo(1, 65536, 8, CM)
    assert not solo(1, 65537) and not solo(17, 4096) and not solo(33, 4096)
    eng.set_option("ACMPC_NO_SOLO", 1)
    assert not solo(1, 4) and not solo(1, 65536)
    eng.close()
    eng = _engine(T)
    assert not eng.describe_rollout(1, 4, 8, SM)["solo"]
    eng.close()


def test_errors():
    eng = _engine(S, max_problems=4, max_candidates=1000, max_steps=50)
    assert eng.describe_rollout(4, 1000, 50, SM)["block"] == 64
    for shape in ((5, 1000, 50), (4, 1001, 50), (4, 1000, 51)):
        with pytest.raises(_capi.EngineError) as e:
            eng.describe_rollout(*shape, SM)
        assert e.value.code == _capi.ECAPACITY
    for shape in ((0, 10, 5, SM), (1, 0, 5, SM), (1, 10, 0, SM), (1, 10, 5, 2), (1, 10, 5, -1)):
        with pytest.raises(_capi.EngineError) as e:
            eng.describe_rollout(*shape)
        assert e.value.code == _capi.EINVAL
    eng.close()
    eng = _engine(_capi.MODE_DYNAMIC, max_steps=128)
    with pytest.raises(_capi.EngineError) as e:
        eng.describe_rollout(1, 130, 50, SM)
    assert e.value.code == _capi.ESTATE
    eng.close()


@pytest.mark.parametrize("mode", [S, T])
def test_a_misaligned_matrix_or_cost_buffer_is_refused_before_any_device_work(mode):
    """Lanes with two or four candidates read their controls and write their costs as one 8- or 16-byte vector: every call
    that takes a step-major matrix refuses a pointer off that boundary with EINVAL, before it opens the device.  No kernel
    runs here on any machine: the pointers are numbers that are never dereferenced, every call made is one that must be
    refused, and the handle names a device ordinal that does not exist, so a call that got past the check would end at
    the device's door with another error (tests/test_gpu_rollout_shapes.py runs the aligned launches)."""
    P, N, n = 2, 2052, 5
    eng = _engine(mode, max_problems=P, max_candidates=N, max_steps=n, device=9999)
    eng.set_paths(np.ones((P, 7, n)))
    eng.set_option("ACMPC_NO_SOLO", 1)
    base = 1 << 20
    calls = {
        "rollout_device": lambda U, costs: eng.rollout_device(base, U, P, N, n, SM, 0, costs, base),
        "solve_device": lambda U, costs: eng.solve_device(base, U, P, N, n, SM, costs, base, base),
        "solve_sampled_device": lambda U, costs: eng.solve_sampled_device(base, U, base, 2 * n, base, P, N, n, SM, (1.0, 0.1), 1, 0,
                                                                          costs, base, base),
        "solve_stream_device": lambda U, costs: eng.solve_stream_device(base, U, base, 2 * n, base, P, N, n, SM, (1.0, 0.1), 1, 0,
                                                                        costs, base, base),
    }
    for shape, boundary in (("256,4", 16), ("256,2", 8)):
        eng.set_option("ACMPC_SHAPE", shape)
        assert eng.describe_rollout(P, N, n, SM)["cpt"] == boundary // 4
        for name, call in calls.items():
            for off in range(4, boundary, 4):
                for U, costs in ((base + off, base), (base, base + off), (base + off, 0)):
                    with pytest.raises(_capi.EngineError, match="%d-byte boundary" % boundary) as e:
                        call(U, costs)
                    assert e.value.code == _capi.EINVAL, (shape, name, off)
    eng.close()


def test_the_query_does_not_open_the_device():
    """With the HIP runtime logging its API calls (AMD_LOG_LEVEL), a process that creates handles of both modes, asks for
    their launch shapes and destroys them logs nothing: no HIP call was made, so the runtime was never initialised.  The
    same process then makes a compute call, whose first HIP call shows up - the log does see one when there is one."""
    script = textwrap.dedent("""
        import sys
        sys.path[:0] = [%r, %r]
        import numpy as np
        from acmpc_amd import Engine, _capi
        kw = dict(max_problems=4096, max_candidates=8192, max_steps=128, step_cost=[1.0, 1.0, 0.0], r_term=[1.0, 1.0],
                  final_cost=[1.0, 0.0, 0.0], u_min=[0.0, -1.0], u_max=[30.0, 1.0], margin=0.5, wheelbase=2.65)
        for mode in (0, 1):
            eng = Engine(mode=mode, **kw)
            for layout in (0, 1):
                for P, N, n in ((1, 4, 3), (33, 4096, 49), (256, 4096, 49), (32, 4096, 8), (2, 65, 128)):
                    assert eng.describe_rollout(P, N, n, layout)["block"] in (64, 256)
            eng.set_option("ACMPC_SHAPE", "256,4")
            assert eng.describe_rollout(3, 1028, 5, 1)["cpt"] == 4
            eng.close()
        sys.stderr.write("== queried ==\\n")
        sys.stderr.flush()
        eng = Engine(mode=0, **kw)
        eng.set_paths(np.ones((1, 7, 10)))
        try:
            eng.solve(np.zeros((1, 3)), np.ones((1, 64, 10, 2)))
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
