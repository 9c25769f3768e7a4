"""The softmin (MPPI) mean on the MI355X against its float64 reference (tests/softmin_reference64.py: the contract, the
inputs, the error measure r).

Matrix form - acmpc_softmin_device, both layouts, handles of mode S and mode D - at every shape of
softmin_reference64.MATRIX_SHAPES: the exact inputs bit for bit (mean and weight sum), the general inputs within R_TOL, with
`weight_sum` given and null; the uniform fallback's VALUE in the last problem of every call; one call at exactly a handle's
capacity (n = 1 024: eight passes of the candidate-major kernel) and a smaller one behind it.  Every shape's launch is asserted
through `describe_softmin`, the launcher's own numbers (tests/test_softmin_shapes.py has them as literals).

Sampled form - acmpc_softmin_sampled_device at three shapes whose waves walk several items (gridDim.z = 16, 4 and 1): bit
for bit the matrix form over the sampler's matrix (test_gpu_dynamic_softmin._both_forms), and that matrix side within R_TOL
of mean64 over the same matrix read back, so the new path hangs on the reference and not only on its sibling kernel.

Tolerance (softmin_reference64.R_TOL, WSUM_RTOL).  Measured on the MI355X over these very inputs: max r = 0.933 - at (n, N) =
(129, 2), where the final rounding of the mean is most of it; 0.19 - 0.20 at N >= 1023, 0.49 - 0.58 at N = 63 .. 65, 0.54 - 0.63 on
the matrix side of the sampled shapes, the same on handles of mode S and mode D - and the weight sum within 0.260 x 2^-24
relative (the sampled shape of 256 problems; 0.235 x 2^-24 among the matrix shapes).  Held at 4 x those: r <= 3.732, weight sum
within 1.04 x 2^-24.  An r of this size is a float32 expf of a float32 quotient summed in float64; the inputs are built so that a
candidate dropped or counted twice shows as r >= 1 087 (tests/test_softmin_reference64.py).  Every test prints its own maximum
before it asserts."""
import numpy as np
import pytest

import softmin_reference64 as sr
import test_gpu_dynamic_softmin as tgs

pytestmark = pytest.mark.gpu

P = sr.P
CM, SM, SAMPLED = 0, 1, 2
MODES = {"S": 0, "D": 2}
# candidate-major: thread groups and 256-entry passes of a row of 2n floats
ROWS = {2: (64, 1), 64: (2, 1), 85: (1, 1), 127: (1, 1), 128: (1, 1), 129: (1, 2), 256: (1, 2), 512: (1, 4), 1024: (1, 8)}
CHUNKS = {1: 1, 2: 1, 63: 1, 64: 1, 65: 1, 1023: 1, 1024: 1, 1025: 2, 2049: 3}

_cache = {}


def _engine(mode, max_candidates, max_steps):
    from acmpc_amd import DynamicBicycleParams, Engine, _capi
    assert (_capi.MODE_SPATIAL, _capi.MODE_DYNAMIC) == (MODES["S"], MODES["D"])
    eng = Engine(mode=mode, max_problems=P, max_candidates=max_candidates, max_steps=max_steps, step_cost=(1.0, 1.0, 0.0),
                 r_term=(0.5, 10.0), final_cost=(1.0, 1.0, 0.0), u_min=(-0.3, -1.0), u_max=(0.3, 1.0), margin=0.0,
                 wheelbase=2.898, dt=0.05, softmin_lambda=sr.LAMBDA)
    if mode == _capi.MODE_DYNAMIC:
        eng.set_dynamics(DynamicBicycleParams.reference())
    return eng


def _set_horizon(eng, n):
    """Tables of n steps: the softmin reads none of them, a call's (P, n) must be theirs."""
    from acmpc_amd import _capi
    eng.set_coefficients(np.zeros((P, n, _capi.COEF_STRIDE[eng.mode]), dtype=np.float32))


def _inputs(kind, n, N):
    """The inputs of a shape and what they must give, computed once for both modes and layouts."""
    key = (kind, n, N)
    if key not in _cache:
        if kind == "exact":
            d = sr.exact_problem(P, N, n)
        else:
            from acmpc_amd import _capi
            d = sr.general_problem(P, N, n)
            ref = [sr.mean64(d["costs"][p], _capi.key_cost(int(d["keys"][p])), d["U"][p], np.float32(sr.LAMBDA)) for p in range(P)]
            d.update(m=np.stack([r[0] for r in ref]), weight_sum=np.array([r[1] for r in ref]), s=np.stack([r[2] for r in ref]))
        for a in d.values():
            a.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def _describe(eng, n, N):
    assert eng.describe_softmin(P, N, n, CM) == dict(chunks=CHUNKS[N], groups=ROWS[n][0], passes=ROWS[n][1])
    assert eng.describe_softmin(P, N, n, SM) == dict(chunks=CHUNKS[N])


def _run(torch, eng, d, n, N, layout, want_wsum):
    """(mean [P, n, 2] float32, weight sums [P] or None) of acmpc_softmin_device over the inputs `d`."""
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    U_h = d["U"] if layout == CM else np.ascontiguousarray(d["U"].transpose(0, 2, 3, 1))
    U = torch.tensor(U_h, device=dev)
    costs, keys = torch.tensor(d["costs"], device=dev), torch.tensor(d["keys"], device=dev)
    mean = torch.full((P, n, 2), -7.0, device=dev)
    wsum = torch.full((P,), -7.0, dtype=torch.float64, device=dev)
    eng.softmin_device(costs.data_ptr(), keys.data_ptr(), U.data_ptr(), P, N, n, layout, mean.data_ptr(),
                       wsum.data_ptr() if want_wsum else 0, s)
    torch.cuda.synchronize()
    if not want_wsum:
        assert np.all(wsum.cpu().numpy() == -7.0)
    return mean.cpu().numpy(), wsum.cpu().numpy() if want_wsum else None


def _check_shape(torch, eng, n, N, what):
    """Both kinds of input, both layouts, the weight sum given and null.  Returns (max r, max relative weight-sum error)."""
    exact, general = _inputs("exact", n, N), _inputs("general", n, N)
    r_max, w_max, over = 0.0, 0.0, []
    for layout in (CM, SM):
        for want_wsum in (True, False):
            tag = "%s n=%d N=%d layout=%d weight_sum=%s" % (what, n, N, layout, want_wsum)
            mean, wsum = _run(torch, eng, exact, n, N, layout, want_wsum)
            assert np.array_equal(mean.view(np.uint32), exact["mean"].view(np.uint32)), "exact mean: " + tag
            if want_wsum:
                assert np.array_equal(wsum, exact["weight_sum"]) and wsum[P - 1] == 0.0, "exact weight sum: " + tag
            mean, wsum = _run(torch, eng, general, n, N, layout, want_wsum)
            r = sr.error_r(mean, general["m"], general["s"])
            r_max = max(r_max, float(r.max()))
            if want_wsum:
                assert wsum[P - 1] == 0.0 and general["weight_sum"][P - 1] == 0.0, tag      # the fallback, exactly 0
                w_err = np.abs(wsum[:P - 1] - general["weight_sum"][:P - 1]) / general["weight_sum"][:P - 1]
                w_max = max(w_max, float(w_err.max()))
                if not w_err.max() <= sr.WSUM_RTOL:
                    over.append("weight sum off by %.3g: %s" % (w_err.max(), tag))
            if not (np.all(np.isfinite(mean)) and r.max() <= sr.R_TOL):
                over.append("r = %.3g at problem %d: %s" % (r.max(), int(np.argmax(r.reshape(P, -1).max(axis=1))), tag))
    print("softmin %s n=%d N=%d: max r %.3f, weight sum %.3f x 2^-24" % (what, n, N, r_max, w_max / sr.EPS))
    assert not over, over
    return r_max, w_max


@pytest.mark.parametrize("mode", ["S", "D"])
@pytest.mark.parametrize("shape", sr.MATRIX_SHAPES, ids=lambda s: "n%d_N%d" % s)
def test_the_matrix_form_against_the_float64_reference(shape, mode):
    import torch
    n, N = shape
    eng = _engine(MODES[mode], 2049, 512)
    try:
        _set_horizon(eng, n)
        _describe(eng, n, N)
        _check_shape(torch, eng, n, N, "mode " + mode)
    finally:
        eng.close()


def test_a_call_at_the_handles_capacity_and_a_smaller_one_behind_it():
    """P, N and n all at the capacity the handle was created with - what its partial sums' buffer is sized for - with n = 1 024
    on a mode S handle (eight passes over a row; mode D ends at 512 steps), then a smaller call on the same handle."""
    import torch
    n, N = sr.CAPACITY_SHAPE
    eng = _engine(MODES["S"], N, n)
    try:
        from acmpc_amd import EngineError, _capi
        _set_horizon(eng, n)
        _describe(eng, n, N)
        for over in ((P + 1, N, n), (P, N + 1, n), (P, N, n + 1)):
            with pytest.raises(EngineError) as refused:
                eng.describe_softmin(*over, CM)
            assert refused.value.code == _capi.ECAPACITY
        _check_shape(torch, eng, n, N, "at capacity")
        n, N = sr.SHAPE_AFTER_CAPACITY
        _set_horizon(eng, n)
        _describe(eng, n, N)
        _check_shape(torch, eng, n, N, "behind it")
    finally:
        eng.close()


# ---- the sampled form where a wave walks several items ---------------------------------------------------------------------
# (P, N, n): what describe_softmin must say of it
SAMPLED_SHAPES = {
    (4, 7169, 512): dict(chunks=8, items=70, grid_z=16, items_per_wave=2),     # 32 chunks: z = 16 < ceil(70 / 4) = 18
    (64, 1025, 129): dict(chunks=2, items=21, grid_z=4, items_per_wave=2),     # 128 chunks
    (256, 1025, 49): dict(chunks=2, items=7, grid_z=1, items_per_wave=2),      # 512 chunks: one workgroup per chunk
}


@pytest.mark.parametrize("offset", [0, tgs.BIG_OFFSET], ids=["offset0", "offset_past_2_31"])
@pytest.mark.parametrize("with_ref", [False, True], ids=["no_u_ref", "u_ref"])
@pytest.mark.parametrize("shape", list(SAMPLED_SHAPES), ids=lambda s: "P%d_N%d_n%d" % s)
def test_sampled_waves_that_walk_several_items(shape, with_ref, offset):
    import acmpc_oracle as orc
    import dynamic_spec as ds
    import test_gpu_dynamic_ensemble as tge
    import torch
    from acmpc_amd import Engine, _capi
    Pn, N, n = shape
    dp = ds.make_dynamic_problem(orc, "monza", n + 1, 4, 40 + n)
    eng = Engine(**dict(dp["kw"], max_problems=Pn, max_candidates=N, max_steps=n, softmin_lambda=tgs.LAMBDA))
    try:
        eng.set_dynamics(tge._vehicles()[0])
        eng.set_paths(np.stack([dp["table"]] * Pn))
        assert eng.describe_softmin(Pn, N, n, SAMPLED) == SAMPLED_SHAPES[shape]
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream().cuda_stream
        centre_h, ref_h = tgs._centres([dp] * Pn, n, n)
        centre, ref = torch.tensor(centre_h, device=dev), torch.tensor(ref_h, device=dev) if with_ref else None
        costs_h, keys_h = tgs._synthetic_costs(Pn, N, seed=17 * n + N)
        costs, keys = torch.tensor(costs_h, device=dev), torch.tensor(keys_h, device=dev)
        seed, rnd = 0x1234567890AB, 2
        got, want = tgs._both_forms(torch, eng, dev, s, costs, keys, centre, ref, Pn, N, n, offset, tgs.SIGMA, seed, rnd)
        assert np.array_equal(tgs._u32(got[0]), tgs._u32(want[0])), "mean"
        assert np.array_equal(tgs._u64(got[1]), tgs._u64(want[1])), "weight sum"
        # the matrix side against the reference, over the matrix it read
        U = torch.empty(Pn, n, 2, N, device=dev)
        eng.sample_device(centre.data_ptr(), 2 * n, ref.data_ptr() if with_ref else 0, Pn, N, n, SM, offset, tgs.SIGMA, seed, rnd,
                          U.data_ptr(), s)
        torch.cuda.synchronize()
        U_h = U.cpu().numpy()
    finally:
        eng.close()
    mean, wsum = want[0].cpu().numpy(), want[1].cpu().numpy()
    r_max, w_max = 0.0, 0.0
    for p in range(Pn):
        m, total, scale = sr.mean64(costs_h[p], _capi.key_cost(int(keys_h[p])), U_h[p].transpose(2, 0, 1), np.float32(tgs.LAMBDA))
        r_max = max(r_max, float(sr.error_r(mean[p], m, scale).max()))
        if p == Pn - 1:
            assert total == 0.0 and wsum[p] == 0.0
        else:
            w_max = max(w_max, abs(wsum[p] - total) / total)
    print("softmin sampled P=%d N=%d n=%d u_ref=%s offset=%d: max r %.3f, weight sum %.3f x 2^-24"
          % (Pn, N, n, with_ref, offset, r_max, w_max / sr.EPS))
    assert r_max <= sr.R_TOL and w_max <= sr.WSUM_RTOL
