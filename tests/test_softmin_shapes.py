"""The launches of the softmin mean, as literal numbers (no GPU): `acmpc_describe_softmin` answers from the host functions the
launchers themselves ask (csrc: softmin_chunks, softmin_rows, softmin_item_count, softmin_items) and from the sampler's knot
table, so the sizes below are those at which `acmpc_softmin_device` takes another pass over a row and
`acmpc_softmin_sampled_device` gives a wave more than one item.  They are fixed here on purpose: whoever changes a rule moves
the cases of tests/test_gpu_softmin_float64.py, which run them on the device, with it."""
import pytest

from acmpc_amd import MODE_DYNAMIC, MODE_SPATIAL, Engine, EngineError, _capi

CM, SM, SAMPLED = _capi.SOFTMIN_CANDIDATE_MAJOR, _capi.SOFTMIN_STEP_MAJOR, _capi.SOFTMIN_SAMPLED


def _engine(mode=MODE_SPATIAL, **extra):
    kw = dict(mode=mode, max_problems=256, max_candidates=8192, max_steps=1024 if mode == MODE_SPATIAL else 512,
              step_cost=[1.0, 1.0, 0.0], r_term=[1.0, 1.0], final_cost=[1.0, 0.0, 0.0], u_min=[-0.3, -1.0], u_max=[0.3, 1.0],
              margin=0.5, wheelbase=2.65, softmin_lambda=0.5)
    kw.update(extra)
    return Engine(**kw)


def _dynamic_engine():
    from acmpc_amd import DynamicBicycleParams
    eng = _engine(MODE_DYNAMIC)
    eng.set_dynamics(DynamicBicycleParams.reference())
    return eng


@pytest.mark.parametrize("mode", [MODE_SPATIAL, MODE_DYNAMIC])
def test_chunks_of_1024_candidates_in_every_form(mode):
    eng = _engine() if mode == MODE_SPATIAL else _dynamic_engine()
    for N, chunks in ((1, 1), (2, 1), (63, 1), (64, 1), (65, 1), (1023, 1), (1024, 1), (1025, 2), (2048, 2), (2049, 3), (7169, 8),
                      (8192, 8)):
        for form in (CM, SM, SAMPLED):
            assert eng.describe_softmin(3, N, 129, form)["chunks"] == chunks, (N, form)
    assert eng.describe_softmin(3, 1025, 129, SM) == dict(chunks=2)        # nothing else decides the step-major launch
    eng.close()


def test_candidate_major_thread_groups_and_passes():
    """A row is 2n floats: 256 / 2n rows side by side while a row fits the workgroup at least twice, one row from n = 65, and
    from n = 129 a row takes more than one pass of 256 entries."""
    eng = _engine()
    for n, groups, passes in ((1, 128, 1), (2, 64, 1), (3, 42, 1), (49, 2, 1), (64, 2, 1), (65, 1, 1), (85, 1, 1), (127, 1, 1),
                              (128, 1, 1), (129, 1, 2), (256, 1, 2), (257, 1, 3), (384, 1, 3), (512, 1, 4), (513, 1, 5),
                              (1023, 1, 8), (1024, 1, 8)):
        for N in (1, 1025):
            assert eng.describe_softmin(3, N, n, CM) == dict(chunks=(N + 1023) // 1024, groups=groups, passes=passes), (n, N)
    eng.close()
    eng = _dynamic_engine()
    assert eng.describe_softmin(3, 1025, 512, CM) == dict(chunks=2, groups=1, passes=4)
    eng.close()


def test_sampled_items_and_workgroups_per_chunk():
    """Items: runs of at most 8 steps that share a left knot, 7 knot intervals over the horizon.  gridDim.z = min(ceil(512 /
    (chunks P)), ceil(items / 4)): while the chunks of a launch are few every wave owns one item; from 32 chunks at n = 512,
    128 at n = 129 and 512 at any n, a wave walks several."""
    eng = _dynamic_engine()
    # (n = 2: two intervals with a step; 56: seven of 8 steps; 57: the last has 9; 58: the first and the last have 9)
    items = {2: 2, 7: 7, 8: 7, 49: 7, 56: 7, 57: 8, 58: 9, 129: 21, 512: 70}
    for n, m in items.items():
        d = eng.describe_softmin(1, 1, n, SAMPLED)
        assert d == dict(chunks=1, items=m, grid_z=(m + 3) // 4, items_per_wave=1), n
    # every shape the suite ran before: chunks P <= 9, one item per wave
    for P, N, n in ((3, 3000, 512), (3, 1025, 129), (3, 3000, 49), (3, 1500, 49), (1, 8192, 512)):
        d = eng.describe_softmin(P, N, n, SAMPLED)
        assert d["grid_z"] == (d["items"] + 3) // 4 and d["items_per_wave"] == 1, (P, N, n)
    # the first shapes at which the chip's share is the smaller number
    assert eng.describe_softmin(4, 7168, 512, SAMPLED) == dict(chunks=7, items=70, grid_z=18, items_per_wave=1)   # 28 chunks: 19 > 18
    assert eng.describe_softmin(4, 7169, 512, SAMPLED) == dict(chunks=8, items=70, grid_z=16, items_per_wave=2)   # 32 chunks
    assert eng.describe_softmin(64, 1024, 129, SAMPLED) == dict(chunks=1, items=21, grid_z=6, items_per_wave=1)   # 64 chunks: 8 > 6
    assert eng.describe_softmin(64, 1025, 129, SAMPLED) == dict(chunks=2, items=21, grid_z=4, items_per_wave=2)   # 128 chunks
    assert eng.describe_softmin(256, 1024, 49, SAMPLED) == dict(chunks=1, items=7, grid_z=2, items_per_wave=1)    # 256 chunks
    assert eng.describe_softmin(256, 1025, 49, SAMPLED) == dict(chunks=2, items=7, grid_z=1, items_per_wave=2)    # 512 chunks
    assert eng.describe_softmin(256, 8192, 512, SAMPLED) == dict(chunks=8, items=70, grid_z=1, items_per_wave=18)
    eng.close()
    eng = _engine()
    assert eng.describe_softmin(1, 1025, 1024, SAMPLED) == dict(chunks=2, items=133, grid_z=34, items_per_wave=1)
    assert eng.describe_softmin(256, 1025, 1024, SAMPLED) == dict(chunks=2, items=133, grid_z=1, items_per_wave=34)
    eng.close()


def test_it_refuses_what_the_calls_refuse():
    def code(eng, *args):
        with pytest.raises(EngineError) as refused:
            eng.describe_softmin(*args)
        return refused.value.code

    eng = _engine()
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        for form in (CM, SM, SAMPLED):
            assert code(eng, *shape, form) == _capi.EINVAL, (shape, form)
    for form in (-1, 3):
        assert code(eng, 1, 8, 8, form) == _capi.EINVAL
    for shape in ((257, 8, 8), (1, 8193, 8), (1, 8, 1025)):
        for form in (CM, SM, SAMPLED):
            assert code(eng, *shape, form) == _capi.ECAPACITY, (shape, form)
    assert eng.describe_softmin(256, 8192, 1024, CM) == dict(chunks=8, groups=1, passes=8)      # the capacity itself
    eng.close()
    eng = _engine(MODE_DYNAMIC)
    assert code(eng, 1, 8, 8, SM) == _capi.ESTATE                     # mode D without a vehicle
    eng.close()
    eng = _dynamic_engine()
    assert code(eng, 1, 8, 513, SM) == _capi.ECAPACITY and eng.describe_softmin(1, 8, 512, SM) == dict(chunks=1)
    eng.close()
    eng = _engine(softmin_lambda=0.0)
    assert code(eng, 1, 8, 8, SM) == _capi.EINVAL                     # as acmpc_softmin_device: lambda must be positive
    eng.close()
    lib = _capi.load_library()
    eng = _engine()
    assert lib.acmpc_describe_softmin(eng._ctx, 1, 8, 8, SM, None) == _capi.EINVAL
    assert lib.acmpc_describe_softmin(None, 1, 8, 8, SM, None) == _capi.EINVAL
    eng.close()
