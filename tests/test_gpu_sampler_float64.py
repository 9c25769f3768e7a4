"""The sampler on the MI355X against the float64 reference of tests/sampler_reference64.py and against what its numbers are
meant to be.  The normals are read off the device at a shape where a candidate IS its normals times a power of two; the
candidate sets go through acmpc_sample_device at the horizon and launch edges; and mode D's three draw sites (the rollout
that draws, the finalize and the softmin that re-draw) meet the reference through one winner.  Bit-for-bit ties to the
oracle ride along - the tolerances and the conditions are those of tests/test_sampler_float64.py.

`python tests/test_gpu_sampler_float64.py` runs the RESTATEMENT (no GPU) at exactly the sets the device test draws and
prints the statistics the comments below quote: the reference alone stays inside the conditions."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "ac-mpc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acmpc_oracle as orc  # noqa: E402
import sampler_reference64 as r64  # noqa: E402
import test_sampler_float64 as cpu  # noqa: E402
from test_support import engine_kwargs, make_problem  # noqa: E402

pytestmark = pytest.mark.gpu

# ---- 1. normals read off the device --------------------------------------------------------------------------------------------
# n = 8, centre 0, no u_ref, sigma (1, 1), box +-100: the knot table is weight 1 on knot i for steps 0 .. 6 and weight 0 on
# knot 6 (so 1 on knot 7) for step 7, and U[c, i, :] = amp_c z_c[i] with nothing else left of the blend.  For the levels amp
# in {1/8, 1/4, 1/2, 1} - c & 7 in {0, 1, 3, 7}, global candidate 0 excluded - the product is exact: z = U / amp.
# N = 2^20 per call: 524 287 candidates x 16 = 8 388 592 normals per (problem, round, seed).
#
# What the RESTATEMENT gives at these sets (this file's __main__, on the CPU), in standard errors as in the CPU file:
#   problem round  mean   var    skew   kurt   KS    largest  pair  squares block neighbours knots c/c+1 c/c+8
#      0      0    +0.61  +1.58  -1.39  +0.12  0.96  5.34     0.99  0.03    1.99  1.97       2.62  0.54  1.08
#      1      0    +1.85  +0.06  -1.50  -0.96  1.36  5.89     1.04  1.35    0.98  0.61       3.19  0.69  1.34
#      0      1    -0.01  +0.61  -1.02  -0.44  0.48  5.22     0.22  1.42    2.41  2.91       3.16  0.20  0.57
#      1      1    -0.87  -1.47  +0.73  +0.56  0.94  5.19     0.16  0.75    1.91  1.81       3.17  0.18  0.93
#   problems 0 / 1: 0.53 at round 0, 0.91 at round 1; problem 0 across rounds 0.15, across the key's low word 1.50, across its
#   high word 1.35.  (Problem 1, round 0 holds a draw of the smallest uniform: its largest |z| is the truncation bound 5.887.)
NORMALS_N = 1 << 20
CHECKED = 1 << 16                  # the first candidates, compared one by one with the oracle and the float64 reference
BIG_ODD_OFFSET = 3_000_000_013     # a slice of 1 000 there crosses three 256-lane workgroup edges; amplitudes start at 6/8
SLICE = 1000
EXACT_LEVELS = (0, 1, 3, 7)        # c & 7 of the amplitudes 1/8, 1/4, 1/2, 1
SETS = [(0, cpu.SEED), (1, cpu.SEED), (0, cpu.SEED_LOW), (0, cpu.SEED_HIGH)]      # (round, seed) drawn for both problems


def exact_candidates(N, offset=0):
    """(global indices, amplitudes) of the candidates of a launch whose amplitude is a power of two, candidate 0 excluded"""
    g = offset + np.arange(N, dtype=np.int64)
    keep = np.isin(g & 7, EXACT_LEVELS) & (g != 0)
    return g[keep], keep, ((g & 7) + 1) / 8.0


def set_figures(z, g):
    """Moments, Kolmogorov-Smirnov and the pairings inside one set z [M, 8, 2] whose rows are the global candidates g
    (ascending): every figure in standard errors but `ks` (D sqrt M) and `largest`."""
    out = dict(r64.moment_figures(z), ks=r64.ks_figure(z))
    out.update(r64.within_candidate_figures(z))
    for name, step in (("c / c + 1", 1), ("c / c + 8", 8)):
        j = np.searchsorted(g, g + step)
        ok = j < g.size
        ok[ok] &= g[j[ok]] == g[ok] + step
        out[name] = r64.correlation_figure(z[ok], z[j[ok]])
    return out


def assert_conditions(f, what):
    for name in ("mean", "variance", "skewness", "kurtosis", "pair", "pair_squares", "block", "neighbours", "knots",
                 "c / c + 1", "c / c + 8"):
        assert abs(f[name]) <= cpu.SIGMAS, "%s: %s is %.2f standard errors off" % (what, name, f[name])
    assert f["ks"] <= cpu.KS_LIMIT, "%s: Kolmogorov-Smirnov D sqrt M = %.2f" % (what, f["ks"])
    assert f["largest"] <= r64.Z_MAX + cpu.Z_ATOL, what


def _describe(f):
    return ("mean %+.2f var %+.2f skew %+.2f kurt %+.2f  KS %.2f  largest %.2f  pair %.2f squares %.2f block %.2f neighbours %.2f "
            "knots %.2f  c/c+1 %.2f  c/c+8 %.2f" % (f["mean"], f["variance"], f["skewness"], f["kurtosis"], f["ks"], f["largest"],
                                                    f["pair"], f["pair_squares"], f["block"], f["neighbours"], f["knots"],
                                                    f["c / c + 1"], f["c / c + 8"]))


def _mode_s_engine(P, N, n, u_min, u_max):
    """A mode S handle with tables of n steps (the sampler reads none of them)."""
    from acmpc_amd import Engine
    prob = make_problem(orc, "monza", 9, 4, seed=0)
    eng = Engine(**engine_kwargs(prob, 0, P, N, n, u_min=u_min, u_max=u_max))
    eng.set_coefficients(np.ones((P, n, orc.COEF_STRIDE_S), dtype=np.float32))
    return eng


class NormalsRig:
    """P = 2, n = 8 at the shape described above; draw() gives the candidate-major matrix [P, N, 8, 2] on the host."""

    P, n = 2, 8

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.s = torch.cuda.current_stream().cuda_stream
        self.eng = _mode_s_engine(self.P, NORMALS_N, self.n, (-100.0, -100.0), (100.0, 100.0))
        self.centre = torch.zeros(self.P, self.n, 2, device=self.dev)

    def draw(self, N, offset, rnd, seed, layout):
        t = self.torch
        U = t.full((self.P, N, self.n, 2) if layout == 0 else (self.P, self.n, 2, N), -7.0, device=self.dev)
        self.eng.sample_device(self.centre.data_ptr(), 2 * self.n, 0, self.P, N, self.n, layout, offset, (1.0, 1.0), seed, rnd,
                               U.data_ptr(), self.s)
        t.cuda.synchronize()
        return U if layout == 0 else U.permute(0, 3, 1, 2)

    def close(self):
        self.eng.close()


def _compare_with_both_references(U, N, offset, rnd, seed, what):
    """U [P, N, 8, 2] of a launch at `offset`: every candidate is amp x the oracle's normals bit for bit (one multiply), and
    where amp is a power of two U / amp is within the float64 tolerance of the reference's normals."""
    g, keep, amp = exact_candidates(N, offset)
    for p in range(U.shape[0]):
        gidx, zo = orc.candidate_normals(N, offset, p, rnd, seed)
        want = orc.candidate_amplitude(gidx)[:, None, None] * zo
        assert np.array_equal(U[p], want), "%s, problem %d: not the oracle's candidates" % (what, p)
        z = U[p][keep] / amp[keep][:, None, None].astype(np.float32)
        assert np.array_equal(z, zo[keep]), "%s, problem %d: not the oracle's normals" % (what, p)
        z64 = r64.normals64(N, offset, p, rnd, seed)[1][keep]
        err = np.abs(z.astype(np.float64) - z64).max()
        assert err <= cpu.Z_ATOL, "%s, problem %d: %.3e from the float64 normals" % (what, p, err)


@pytest.mark.parametrize("rnd,seed", SETS[:2])
def test_device_normals_against_float64_and_the_normal_distribution(rnd, seed):
    """Rounds 0 and 1, both problems, both layouts, 2^20 candidates a call: the layouts agree; the first 2^16 candidates and a
    slice at a large odd offset equal the oracle bit for bit and the float64 normals within Z_ATOL; each problem's 8.4 M
    normals meet the moment, Kolmogorov-Smirnov and correlation conditions, and the two problems are uncorrelated."""
    rig = NormalsRig()
    try:
        U = rig.draw(NORMALS_N, 0, rnd, seed, 0)
        assert rig.torch.equal(U, rig.draw(NORMALS_N, 0, rnd, seed, 1)), "the layouts differ"
        U = U.cpu().numpy()
        assert np.all(U[:, 0] == 0.0)                                          # global candidate 0: the centre
        _compare_with_both_references(U[:, :CHECKED], CHECKED, 0, rnd, seed, "round %d" % rnd)
        for layout in (0, 1):
            part = rig.draw(SLICE, BIG_ODD_OFFSET, rnd, seed, layout).cpu().numpy()
            _compare_with_both_references(part, SLICE, BIG_ODD_OFFSET, rnd, seed, "round %d, the slice, layout %d" % (rnd, layout))
        g, keep, amp = exact_candidates(NORMALS_N)
        z = U[:, keep] / amp[keep][None, :, None, None].astype(np.float32)
        assert z.shape == (2, (NORMALS_N >> 1) - 1, 8, 2)
        for p in range(2):
            f = set_figures(z[p], g)
            print("device, problem %d round %d seed %#x: %s" % (p, rnd, seed, _describe(f)))
            assert_conditions(f, "problem %d round %d" % (p, rnd))
        across = r64.correlation_figure(z[0], z[1])
        print("device, problems 0 / 1: %.2f" % across)
        assert across <= cpu.SIGMAS, "problems 0 and 1 correlate: |rho| sqrt M = %.2f" % across
    finally:
        rig.close()


def test_device_normals_are_uncorrelated_across_rounds_seeds_and_key_words():
    """Problem 0's 8.4 M normals of round 0 against those of round 1, of the seed's low word + 1 and of its high word ^ 1."""
    rig = NormalsRig()
    try:
        g, keep, amp = exact_candidates(NORMALS_N)
        z = []
        for rnd, seed in SETS:
            U = rig.draw(NORMALS_N, 0, rnd, seed, 1)[0].cpu().numpy()
            z.append(U[keep] / amp[keep][:, None, None].astype(np.float32))
        for other, name in ((1, "rounds"), (2, "the key's low word"), (3, "the key's high word")):
            figure = r64.correlation_figure(z[0], z[other])
            print("device, across %s: %.2f" % (name, figure))
            assert figure <= cpu.SIGMAS, "across %s: |rho| sqrt M = %.2f" % (name, figure)
    finally:
        rig.close()


# ---- 2. candidate sets at the horizon and launch edges ----------------------------------------------------------------------------
# The smallest horizon is 2: acmpc_set_paths and acmpc_set_coefficients both refuse n = 1 ("need P >= 1 and n >= 2"), so no
# launch reaches upload_segments' n = 1 branch through the C API; the test below asserts the refusal.  The oracle at n = 1 is
# held to the float64 reference on the CPU (tests/test_sampler_float64.py).
EDGE_HORIZONS = [2, 3, 7, 8, 9, 128, 1024]
EDGE_CANDIDATES = [1, 63, 65, 257, 1025]


def test_the_smallest_horizon_a_handle_takes_is_two():
    from acmpc_amd import Engine
    from acmpc_amd._capi import EngineError
    prob = make_problem(orc, "monza", 9, 4, seed=0)
    eng = Engine(**engine_kwargs(prob, 0, 1, 4, 8))
    try:
        with pytest.raises(EngineError):
            eng.set_coefficients(np.ones((1, 1, orc.COEF_STRIDE_S), dtype=np.float32))
        with pytest.raises(EngineError):
            eng.set_paths(np.ones((1, 7, 1)))
        eng.set_coefficients(np.ones((1, 2, orc.COEF_STRIDE_S), dtype=np.float32))
    finally:
        eng.close()


@pytest.mark.parametrize("n", EDGE_HORIZONS)
def test_candidate_sets_at_the_horizon_and_launch_edges(n):
    """acmpc_sample_device with u_ref, both layouts, index_offset 0 and the largest accepted, N at the wave and workgroup
    edges: the oracle's candidates bit for bit, the float64 reference's within U_TOL (inputs, box and sigma are the CPU
    file's, where U_TOL is measured)."""
    import torch
    P, rnd, seed = 2, 1, cpu.SEED_HIGH + 77
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    inputs = [cpu.problem_inputs(n, seed=5 + 100 * p) for p in range(P)]
    centre_h, ref_h = np.stack([i[0] for i in inputs]), np.stack([i[1] for i in inputs])
    centre, ref = torch.tensor(centre_h, device=dev), torch.tensor(ref_h, device=dev)
    eng = _mode_s_engine(P, max(EDGE_CANDIDATES), n, cpu.U_LO, cpu.U_HI)
    try:
        for N in EDGE_CANDIDATES:
            for offset in (0, (1 << 32) - 1 - N):
                want = [orc.sample_candidates(centre_h[p], ref_h[p], N, offset, p, rnd, seed, cpu.SIGMA, cpu.U_LO, cpu.U_HI)
                        for p in range(P)]
                for p in range(P):
                    U64 = r64.candidates64(centre_h[p], ref_h[p], N, offset, p, rnd, seed, cpu.SIGMA, cpu.U_LO, cpu.U_HI)
                    excess = cpu.candidate_excess(want[p], U64, cpu.SIGMA).max()
                    assert excess <= cpu.U_TOL, "the restatement itself, n %d N %d offset %d: %.3e sigma" % (n, N, offset, excess)
                for layout in (0, 1):
                    U = torch.full((P, N, n, 2) if layout == 0 else (P, n, 2, N), -7.0, device=dev)
                    eng.sample_device(centre.data_ptr(), 2 * n, ref.data_ptr(), P, N, n, layout, offset, cpu.SIGMA, seed, rnd,
                                      U.data_ptr(), s)
                    torch.cuda.synchronize()
                    got = (U if layout == 0 else U.permute(0, 3, 1, 2)).cpu().numpy()
                    what = "n %d N %d offset %d layout %d" % (n, N, offset, layout)
                    for p in range(P):
                        assert np.array_equal(got[p], want[p]), what + ": not the oracle's candidates"
                        U64 = r64.candidates64(centre_h[p], ref_h[p], N, offset, p, rnd, seed, cpu.SIGMA, cpu.U_LO, cpu.U_HI)
                        excess = cpu.candidate_excess(got[p], U64, cpu.SIGMA).max()
                        assert excess <= cpu.U_TOL, "%s: %.3e sigma from the float64 candidates" % (what, excess)
    finally:
        eng.close()


# ---- 3. mode D: three draw sites, one winner ---------------------------------------------------------------------------------------
def test_mode_d_draw_sites_meet_the_float64_reference_through_one_winner():
    """n = 8.  acmpc_rollout_sampled_device draws the candidates and names a winner; acmpc_finalize_sampled_device re-draws
    it into the record; acmpc_softmin_sampled_device, given costs that are +inf everywhere but at the winner, re-draws it as
    its mean (weight 1 on one candidate).  Both equal the winner's row of the matrix acmpc_sample_device writes, and that row
    is within U_TOL of the reference's candidate.  At index_offset 0 and at a large odd one."""
    import torch
    import test_gpu_dynamic_sampled as tds
    from acmpc_amd import _capi
    P, N, n, sigma, seed, rnd = 2, 1000, 8, (0.04, 0.35), 0xC0FFEE1234, 1
    rig = tds.Rig(P, N, n, K=1, window=(2, 5), seed=108, with_ref=True)
    try:
        kw = rig.dps[0]["kw"]
        for offset in (0, BIG_ODD_OFFSET):
            costs, keys = rig.fused(N, offset, sigma, seed, rnd)
            U = rig.matrix(N, offset, sigma, seed, rnd)[0].permute(0, 3, 1, 2).cpu().numpy()           # [P, N, n, 2]
            keys_h, costs_h = keys.cpu().numpy(), costs.cpu().numpy()
            winners = [_capi.key_index(int(k)) - offset for k in keys_h]
            # the rollout's own winner, then the last candidate of the launch with a finite cost, named by a key made here
            others = [int(np.flatnonzero(np.isfinite(costs_h[p]) & (np.arange(N) != winners[p]))[-1]) for p in range(P)]
            for name, picks in (("winner", winners), ("last finite", others)):
                lone = np.full((P, N), np.inf, dtype=np.float32)
                for p, w in enumerate(picks):
                    assert 0 <= w < N and np.isfinite(costs_h[p, w])
                    lone[p, w] = costs_h[p, w]
                picked = keys if name == "winner" else torch.tensor(
                    np.array([_capi.pack_key(float(costs_h[p, w]), w + offset) for p, w in enumerate(picks)], dtype=np.int64),
                    device=rig.dev)
                rig.fused(N, offset, sigma, seed, rnd, want_costs=False, want_keys=False)
                rec = rig.finalize_sampled(picked, N, sigma, seed, rnd)
                mean = torch.full((P, n, 2), -7.0, device=rig.dev)
                wsum = torch.full((P,), -7.0, dtype=torch.float64, device=rig.dev)
                lone_d = torch.tensor(lone, device=rig.dev)
                rig.eng.softmin_sampled_device(lone_d.data_ptr(), picked.data_ptr(), rig.centre.data_ptr(), 2 * n, rig.ref_ptr, P,
                                               N, n, offset, sigma, seed, rnd, mean.data_ptr(), wsum.data_ptr(), rig.s)
                torch.cuda.synchronize()
                mean_h = mean.cpu().numpy()
                assert np.all(wsum.cpu().numpy() == 1.0)
                for p, w in enumerate(picks):
                    what = "problem %d, offset %d, %s %d" % (p, offset, name, w + offset)
                    row = U[p, w]
                    tds._same_bits(_capi.split_record(rec[p], n)["u"], row, what + ": the record's controls")
                    tds._same_bits(mean_h[p], row, what + ": the softmin mean of the lone finite cost")
                    U64 = r64.candidates64(rig.centre_h[p], rig.ref_h[p], N, offset, p, rnd, seed, sigma, kw["u_min"], kw["u_max"])
                    excess = cpu.candidate_excess(row, U64[w], sigma).max()
                    assert excess <= cpu.U_TOL, "%s: %.3e sigma from the float64 candidate" % (what, excess)
    finally:
        rig.close()


if __name__ == "__main__":
    # the restatement at the device test's sets, on the CPU: about 8 s per 2^20 candidates
    g, keep, amp = exact_candidates(NORMALS_N)
    z = {}
    for rnd, seed in SETS:
        for p in ((0, 1) if (rnd, seed) in SETS[:2] else (0,)):
            z[p, rnd, seed] = orc.candidate_normals(NORMALS_N, 0, p, rnd, seed)[1][keep]
            if (rnd, seed) in SETS[:2]:
                f = set_figures(z[p, rnd, seed], g)
                assert_conditions(f, "the restatement")
                print("restated, problem %d round %d seed %#x: %s" % (p, rnd, seed, _describe(f)))
    for rnd, seed in SETS[:2]:
        print("restated, problems 0 / 1 at round %d: %.2f" % (rnd, r64.correlation_figure(z[0, rnd, seed], z[1, rnd, seed])))
    for (rnd, seed), name in zip(SETS[1:], ("rounds", "the key's low word", "the key's high word")):
        print("restated, across %s: %.2f" % (name, r64.correlation_figure(z[0, 0, cpu.SEED], z[0, rnd, seed])))
