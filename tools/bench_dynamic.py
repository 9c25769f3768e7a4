#!/usr/bin/env python3
"""Mode D's measurement (needs an MI355X): one JSON line with
  - candidate-trajectories/s of the rollout (acmpc_rollout_device, step-major, the 8-waypoint search window) at
    4 096 problems x 4 096 candidates x horizon 50 and at 1 M candidates (256 x 4 096) x horizon 50;
  - p50 / p99 of one 16 384-candidate acmpc_solve_device (rollout + finalize, host-synchronised);
  - VALU instructions per candidate-step of the step loop (profiles/*_isa_mix.json, entry `dynamic`: the compiler's own
    assembly, tools/isa_mix.py);
  - the fraction of the vector-issue roof at 1 M: bench.valu_roofline on that count, the mix priced per opcode with
    profiles/*_valu_probe.json (eight waves per SIMD) over 1 024 SIMDs, with its check that the mix was compiled from the
    loaded sources (`opcode_mix_matches_loaded_sources`).

With `--vehicles K` every figure is measured with an ensemble of K vehicles (acmpc_set_dynamics_ensemble: the default
vehicle at grips 1.0, 0.9, 1.1, 0.8, ...) combined by `--reduce`; rates then count vehicle-candidate-steps too, and the roof
prices the `dynamic_ensemble` entry's mix over P N K candidates.  A comma list (`--vehicles 1,4`) measures each K in the
same process and adds the ratios of each K to the first.

usage: python3 tools/bench_dynamic.py [--reps 20] [--vehicles 1,4] [--reduce mean|max]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ac-mpc_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)


def issue_roof(bench, candidates, steps, kernel_s, name="dynamic"):
    """bench.valu_roofline for the `dynamic` entry (`dynamic_ensemble`: candidates = vehicle-candidates): the step loop's
    static VALU count per candidate-step (the isa mix, whose sources must be the loaded build's -
    `opcode_mix_matches_loaded_sources`) priced per opcode with the valu probe."""
    mix, mix_path = bench.newest_profile("isa_mix.json")
    entry = mix["entries"][name]
    per_step = sum(entry["valu"].values()) / float(entry["candidates_per_lane"])
    counted = (per_step, mix_path + " (static count of the step loop)", {"source_sha256": mix.get("source_sha256")})
    roof, _ = bench.valu_roofline(counted, candidates, steps, kernel_s, mix_entry=name,
                                  cpt=entry["candidates_per_lane"])
    return roof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions (a profiler run)")
    ap.add_argument("--vehicles", default=None, help="K, or a comma list of K: an ensemble of K vehicles")
    ap.add_argument("--reduce", default="mean", choices=("mean", "max"))
    args = ap.parse_args()
    if args.vehicles is None:
        print(json.dumps(measure(args, 1)))
        return
    ks = [int(k) for k in args.vehicles.split(",")]
    by_k = {k: measure(args, k) for k in ks}
    if len(ks) == 1:
        print(json.dumps(by_k[ks[0]]))
        return
    first = by_k[ks[0]]
    out = {"tool": "tools/bench_dynamic.py --vehicles %s --reduce %s" % (args.vehicles, args.reduce),
           "by_vehicles": {str(k): v for k, v in by_k.items()}, "ratios_to_K%d" % ks[0]: {}}
    for k in ks[1:]:
        f = by_k[k]
        out["ratios_to_K%d" % ks[0]][str(k)] = {
            "vehicle_candidate_steps_per_s_4096x4096": f["4096x4096"]["vehicle_candidate_steps_per_s"]
            / first["4096x4096"]["vehicle_candidate_steps_per_s"],
            "vehicle_candidate_steps_per_s_1M": f["1M"]["vehicle_candidate_steps_per_s"]
            / first["1M"]["vehicle_candidate_steps_per_s"],
            "solve_16384_p50": f["solve_16384"]["p50_ms"] / first["solve_16384"]["p50_ms"]}
    print(json.dumps(out))


GRIPS = (1.0, 0.9, 1.1, 0.8, 1.2, 0.7, 1.05, 0.95)


def measure(args, K):
    import torch
    import acmpc_oracle as orc
    import bench
    import dynamic_spec as ds
    from acmpc_amd import DynamicBicycleParams, Engine

    H = 50
    n = H - 1
    dp = ds.make_dynamic_problem(orc, "monza", H, 8, 0)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    reps = 3 if args.quick else args.reps
    out = {"tool": "tools/bench_dynamic.py", "horizon": H, "search": "window (2, 5)"}
    if K > 1:
        out.update(vehicles=K, reduce=args.reduce, grips=list(GRIPS[:K]))

    def engine(P, N):
        kw = dict(dp["kw"], max_problems=P, max_candidates=N, max_steps=n, nn_window=(2, 5))
        eng = Engine(**kw)
        if K == 1:
            eng.set_dynamics(DynamicBicycleParams.reference())
        else:
            eng.set_dynamics_ensemble([DynamicBicycleParams.reference().with_grip(g) for g in GRIPS[:K]],
                                      reduce=args.reduce)
        eng.set_paths(np.repeat(dp["table"][None], P, axis=0))
        eng.sync_tables(s)
        return eng

    def controls(P, N):
        g = torch.Generator(device=dev).manual_seed(7)
        U = torch.empty(P, n, 2, N, device=dev)
        U[:, :, 0] = torch.randn(P, n, N, device=dev, generator=g) * 0.05
        U[:, :, 1] = torch.rand(P, n, N, device=dev, generator=g) * 1.2 - 0.4
        return U

    for name, P, N in (("4096x4096", 4096, 4096), ("1M", 256, 4096)):
        eng = engine(P, N)
        U = controls(P, N)
        x0 = torch.tensor(np.repeat(dp["x0"][None], P, axis=0), device=dev)
        eng.rollout_device(x0.data_ptr(), U.data_ptr(), P, N, n, 1, 0, 0, 0, s)   # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(reps):
            e0.record()
            eng.rollout_device(x0.data_ptr(), U.data_ptr(), P, N, n, 1, 0, 0, 0, s)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        t = float(np.median(times))
        out[name] = dict(P=P, N=N, ms=t * 1e3, traj_per_s=P * N / t, candidate_steps_per_s=P * N * n / t,
                         vehicle_candidate_steps_per_s=P * N * K * n / t)
        eng.close()
        del U
        torch.cuda.empty_cache()

    P, N = 1, 16384
    eng = engine(P, N)
    U = controls(P, N)
    x0 = torch.tensor(dp["x0"][None], device=dev)
    keys = torch.empty(P, dtype=torch.int64, device=dev)
    from acmpc_amd import _capi
    recs = torch.empty(P, _capi.record_floats(n), device=dev)
    lat = []
    for i in range(20 + (20 if args.quick else 400)):
        t0 = time.perf_counter()
        eng.solve_device(x0.data_ptr(), U.data_ptr(), P, N, n, 1, 0, keys.data_ptr(), recs.data_ptr(), s)
        torch.cuda.synchronize()
        if i >= 20:
            lat.append(time.perf_counter() - t0)
    eng.close()
    out["solve_16384"] = dict(p50_ms=float(np.percentile(lat, 50)) * 1e3, p99_ms=float(np.percentile(lat, 99)) * 1e3,
                              calls=len(lat))
    one_m = out["1M"]
    roof = issue_roof(bench, one_m["P"] * one_m["N"] * K, n, one_m["ms"] * 1e-3,
                      "dynamic" if K == 1 else "dynamic_ensemble")
    out["valu_per_candidate_step"] = roof["valu_instructions_per_candidate_step"]
    out["vector_issue_roof"] = roof
    if not roof["opcode_mix_matches_loaded_sources"]:
        print("warning: profiles/*_isa_mix.json does not describe the loaded sources: python3 tools/isa_mix.py <tag>",
              file=sys.stderr)
    return out


if __name__ == "__main__":
    main()
