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

With `--sampled` the rollout that draws its own candidates (acmpc_rollout_sampled_device) is measured against the pair it
replaces - acmpc_sample_device into a matrix + acmpc_rollout_device of it - at the same two sizes, in the same process:
pair / sample / rollout / fused times, fused over pair and over the rollout alone, the fused kernel's fraction of the
vector-issue roof (entry `dynamic_sampled` / `dynamic_sampled_ensemble`); and one acmpc_optimize of 16 384 x 49, 2 rounds
(p50 / p99, host-synchronised) in its two-launch form and with ACMPC_DYNAMIC_MATRIX_ROUNDS=1.  `--optimize` measures that
acmpc_optimize alone, through nothing newer than Engine.optimize - the form to run from a checkout of an earlier commit.

With `--optimize --update softmin` one softmin ROUND of acmpc_optimize (centre_update = 1) is timed in its two forms, in one
process, warm, alternating: the matrix-free round - acmpc_rollout_sampled_device with costs and keys,
acmpc_finalize_sampled_device, acmpc_softmin_sampled_device - against the round through the control matrix -
acmpc_sample_device, acmpc_solve_device with costs and keys, acmpc_softmin_device - at 16 384 x 49 on one problem and at
4 096 x 4 096 x 49; the two softmin calls alone too; median, minimum and maximum of the repetitions (device events).
`--out PATH` also writes the JSON there.

With `--substeps M` and / or `--blend LO,HI` every handle is given that integration setting (acmpc_set_dynamics_integration:
M Euler sub-steps per control step, the low-speed blend between LO and HI m/s); rates still count CONTROL steps.  The rollout's
vector-issue roof then prices the FINE kernels' mix: the step loop's own trip (`dynamic_fine_step`) plus M trips of the
sub-step loop (`dynamic_fine_substep`, whose static count holds the blend's block whether or not the blend is on).

With `--terms` every handle is given rate and slip terms (acmpc_set_dynamics_terms: both parts on, weights and limits as a
controller would set them - TERMS below) and a previous control of zeros for each of its problems: the same shapes, the
kernels of csrc/acmpc_dynamic_terms.hip; with `--substeps` / `--blend` as well, under that integration setting.  The roof
prices `dynamic_terms_step` + M `dynamic_terms_substep`.  With `--objective` (beside `--terms` or alone) every handle is also
given the progress reward and a speed ceiling (acmpc_set_dynamics_objective: both parts on, OBJECTIVE_ON below): the
TermsObjective kernels of the same unit, priced with `dynamic_objective_step` + M `dynamic_objective_substep`.

With `--coupling RF,RR` every handle is given the tyre coupling (acmpc_set_dynamics_coupling: the ratios of the front and the
rear axle; a single number is both): the TermsCoupled kernels of csrc/acmpc_dynamic_coupled.hip, with whatever `--terms` /
`--objective` / `--substeps` / `--blend` set beside it, priced with `dynamic_coupled_step` + M `dynamic_coupled_substep`; and
with `--identify`, identify_grip_coupled_kernel (`identify_grip_coupled`).  To price the coupling, alternate the command with
and without the flag in one job on one card.

With `--load-transfer H[,FRAC]` every handle is given the load transfer (acmpc_set_dynamics_load_transfer: the CG height and
w_frac, 0.9 when left out): the TermsLoaded kernels of csrc/acmpc_dynamic_loaded.hip, with whatever `--coupling` / `--terms` /
`--objective` / `--substeps` / `--blend` set beside it, priced with `dynamic_loaded_step` + M `dynamic_loaded_substep`; and with
`--identify`, identify_grip_loaded_kernel (`identify_grip_loaded`).  To price it, alternate `--coupling 1,1` with
`--coupling 1,1 --load-transfer 0.35` in one job on one card.

With `--downforce KF,KR[,VSAT]` every handle is given the downforce (acmpc_set_dynamics_downforce: the two coefficients and
v_sat, 100 m/s when left out): the TermsAero kernels of csrc/acmpc_dynamic_aero.hip, with whatever `--load-transfer` /
`--coupling` / `--terms` / `--objective` / `--substeps` / `--blend` set beside it, priced with `dynamic_aero_step` + M
`dynamic_aero_substep`; and with `--identify`, identify_grip_aero_kernel (`identify_grip_aero`).  To price it, alternate
`--coupling 1,1 --load-transfer 0.35` with the same plus `--downforce 7.35e-4,1.1025e-3` in one job on one card.

With `--surface` every handle is given a surface table (acmpc_set_surface: a seeded table in [0.5, 1] over all of the handle's
problems and steps, SURFACE_SEED below): the TermsSurface kernels of csrc/acmpc_dynamic_surface.hip - the aero step on per-lane
peaks - with whatever else is set beside it, priced with `dynamic_surface_step` + M `dynamic_surface_substep` (the table adds one
8-byte load and two multiplies per candidate and control step, and per-lane peaks where the aero step reads scalars).  To price it, alternate `--coupling 1,1 --load-transfer 0.35 --downforce
7.35e-4,1.1025e-3` with the same plus `--surface` in one job on one card.  acmpc_score_grips does not read the table.

With `--road` every handle is given a road table (acmpc_set_road: a seeded table over all of the handle's problems and steps, the
grade within +-0.10 rad and the bank within +-0.12 rad per waypoint, ROAD_SEED below): the TermsRoad kernels of
csrc/acmpc_dynamic_road.hip - the surface step with the row's load factor in the peaks and its two accelerations in every sub-step,
with or without `--surface` beside it - priced with `dynamic_road_step` + M `dynamic_road_substep` (`dynamic_actuator_road_*` under
`--actuator`): one 16-byte load and two multiplies per candidate and control step, two adds per sub-step.  To price it, alternate
`--coupling 1,1 --load-transfer 0.35 --downforce 7.35e-4,1.1025e-3 --surface` with the same plus `--road` in one job on one card.
acmpc_score_grips does not read the table.

With `--actuator TAUD,TAUP` every handle is given the actuator lag (acmpc_set_dynamics_actuator) and actuator positions of zero
for all of its problems (acmpc_set_actuator_state): the WithActuator kernels of csrc/acmpc_dynamic_actuator.hip - the aero step,
or with `--surface` the surface step, driven on the lagged control - priced with `dynamic_actuator_step` + M
`dynamic_actuator_substep` (`dynamic_actuator_surface_*` under a table): three VALU operations per channel and control step and
the two carried positions.  To price it, alternate a run with the flag and the same run without it in one job on one card: without
it the handle launches the aero (or surface) pack's kernels.  acmpc_score_grips does not apply the setting.

With `--identify` the grip identification (acmpc_score_grips: host pointers, one blocking round trip) is timed at K = 4 096
(the 64 x 64 split grid) and K = 65 536 (256 x 256) hypotheses over a window of W = 40 steps, in one-step (L = 1) and
eight-step (L = 8) segments, under the run's integration setting: p50 / p99 of the call, the static VALU count per
hypothesis and control step (profiles/*_isa_mix.json, entry `identify_grip`: M sub-step trips + the rest of the step loop),
and the vector-issue time that count needs (bench.valu_roofline) as a fraction of the CALL - a lower bound on the step
kernel's own fraction, which a `rocprofv3 --kernel-trace --stats` run of this command gives (kernel identify_grip_kernel).

With `--trace` the plan trace (acmpc_trace_plans: host pointers, one blocking round trip, a latency call) is timed at
(P, M, K, n) = (1, 1, 1, 49) - one plan under one vehicle, what `plan_states` adds to a solve - and (1, 64, 8, 49), under the
run's settings: p50 / p99 of the call with all three outputs, and of the states alone.

usage: python3 tools/bench_dynamic.py [--reps 20] [--vehicles 1,4] [--reduce mean|max] [--substeps M] [--blend LO,HI] [--terms] [--objective] [--coupling RF,RR]
                                      [--load-transfer H[,FRAC]] [--downforce KF,KR[,VSAT]] [--surface] [--road] [--actuator TAUD,TAUP]
                                      [--sampled | --optimize [--update softmin] | --identify | --trace]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ac-mpc_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)


INTEGRATION = (1, None)   # (--substeps, --blend): what every handle of this run is set to


TERMS = None              # --terms: the rate and slip terms every handle of this run is given
TERMS_ON = dict(rate_weight=(0.5, 0.05), rate_max=(1.0, 8.0), slip_weight=10.0, slip_max=0.1)


OBJECTIVE = None          # --objective: the progress reward and the speed ceiling every handle of this run is given
OBJECTIVE_ON = dict(progress_weight=1.0, speed_ceiling=(1.1, 0.0))


COUPLING = None           # --coupling: the tyre coupling (rho_f, rho_r) every handle of this run is given
LOAD_TRANSFER = None      # --load-transfer: the load transfer (h_cg, w_frac) every handle of this run is given
DOWNFORCE = None          # --downforce: the downforce (k_f, k_r, v_sat) every handle of this run is given
SURFACE = False           # --surface: a seeded surface table in [0.5, 1] on every handle of this run
SURFACE_SEED = 27
ROAD = False              # --road: a seeded road table (grade within +-0.10 rad, bank within +-0.12 rad) on every handle of this run
ROAD_SEED = 29
ACTUATOR = None           # --actuator: the actuator lag (tau_d, tau_p) every handle of this run is given, from positions of zero


def integrate(eng):
    """The run's integration setting and terms on a new handle (a library without the entry points takes only the defaults)."""
    if INTEGRATION != (1, None):
        eng.set_dynamics_integration(*INTEGRATION)
    if TERMS is not None:
        eng.set_dynamics_terms(**TERMS)
        eng.set_previous_control(np.zeros((eng.params.max_problems, 2), dtype=np.float32))   # (a handle's solves use all of them)
    if OBJECTIVE is not None:
        eng.set_dynamics_objective(**OBJECTIVE)
    if COUPLING is not None:
        eng.set_dynamics_coupling(COUPLING)
    if LOAD_TRANSFER is not None:
        eng.set_dynamics_load_transfer(LOAD_TRANSFER)
    if DOWNFORCE is not None:
        eng.set_dynamics_downforce(DOWNFORCE)
    if SURFACE:   # (a handle's solves use all of its problems and steps)
        rng = np.random.default_rng(SURFACE_SEED)
        eng.set_surface(rng.uniform(0.5, 1.0, (eng.params.max_problems, eng.params.max_steps, 2)).astype(np.float32))
    if ROAD:   # (a handle's solves use all of its problems and steps)
        from acmpc_amd.dynamic_model import road_table
        rng = np.random.default_rng(ROAD_SEED)
        shape = (eng.params.max_problems, eng.params.max_steps)
        rows = road_table(rng.uniform(-0.10, 0.10, shape).ravel(), rng.uniform(-0.12, 0.12, shape).ravel())
        eng.set_road(rows.reshape(shape + (3,)))
    if ACTUATOR is not None:
        eng.set_dynamics_actuator(ACTUATOR)
        eng.set_actuator_state(np.zeros((eng.params.max_problems, 2), dtype=np.float32))   # (a handle's solves use all of them)
    return eng


def fine_issue_roof(bench, candidates, steps, kernel_s, name):
    """issue_roof for a FINE kernel: VALU per control step = the step loop's trip + M sub-step trips, priced with the
    sub-step loop's mix (which is nearly all of it)."""
    mix, mix_path = bench.newest_profile("isa_mix.json")
    kind = "_actuator_road_" if ACTUATOR is not None and ROAD else "_road_" if ROAD else "_actuator_surface_" if ACTUATOR is not None and SURFACE else "_actuator_" if ACTUATOR is not None else "_surface_" if SURFACE else "_aero_" if DOWNFORCE is not None else "_loaded_" if LOAD_TRANSFER is not None else "_coupled_" if COUPLING is not None else "_objective_" if OBJECTIVE is not None else "_terms_" if TERMS is not None else "_fine_"
    step, sub = mix["entries"][name + kind + "step"], mix["entries"][name + kind + "substep"]
    per_step = (sum(step["valu"].values()) + INTEGRATION[0] * sum(sub["valu"].values())) / float(sub["candidates_per_lane"])
    counted = (per_step, mix_path + " (static count: step trip + M sub-step trips)", {"source_sha256": mix.get("source_sha256")})
    roof, _ = bench.valu_roofline(counted, candidates, steps, kernel_s, mix_entry=name + kind + "substep",
                                  cpt=sub["candidates_per_lane"])
    roof["substep_count_holds_the_blend_block"] = True
    return roof


def issue_roof(bench, candidates, steps, kernel_s, name="dynamic"):
    """bench.valu_roofline for the `dynamic` entry (`dynamic_ensemble`: candidates = vehicle-candidates): the step loop's
    static VALU count per candidate-step (the isa mix, whose sources must be the loaded build's -
    `opcode_mix_matches_loaded_sources`) priced per opcode with the valu probe."""
    if (INTEGRATION != (1, None) or TERMS is not None or OBJECTIVE is not None or COUPLING is not None or LOAD_TRANSFER is not None or DOWNFORCE is not None or SURFACE or ROAD or ACTUATOR is not None) and name in ("dynamic", "dynamic_ensemble"):
        return fine_issue_roof(bench, candidates, steps, kernel_s, name)
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
    ap.add_argument("--sampled", action="store_true", help="the fused sample + rollout against the matrix pair, and acmpc_optimize")
    ap.add_argument("--optimize", action="store_true", help="acmpc_optimize 16 384 x 49, 2 rounds, alone")
    ap.add_argument("--update", default="argmin", choices=("argmin", "softmin"),
                    help="with --optimize: softmin = one softmin round, matrix-free against through the matrix")
    ap.add_argument("--identify", action="store_true", help="acmpc_score_grips at K = 4 096 and 65 536, W = 40, L = 1 and 8")
    ap.add_argument("--trace", action="store_true", help="acmpc_trace_plans at (P, M, K, n) = (1, 1, 1, 49) and (1, 64, 8, 49)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--substeps", type=int, default=1, help="Euler sub-steps per control step (1 .. 16)")
    ap.add_argument("--blend", default=None, help="LO,HI m/s: the low-speed blend")
    ap.add_argument("--terms", action="store_true", help="rate and slip terms on every handle (TERMS_ON)")
    ap.add_argument("--objective", action="store_true", help="the progress reward and a speed ceiling on every handle (OBJECTIVE_ON)")
    ap.add_argument("--coupling", default=None, help="RF,RR (or one ratio for both axles): the tyre coupling on every handle")
    ap.add_argument("--load-transfer", default=None, help="H[,FRAC]: the load transfer (CG height, w_frac = 0.9) on every handle")
    ap.add_argument("--downforce", default=None, help="KF,KR[,VSAT]: the downforce (per-axle coefficients, v_sat = 100) on every handle")
    ap.add_argument("--surface", action="store_true", help="a seeded surface table in [0.5, 1] on every handle")
    ap.add_argument("--road", action="store_true", help="a seeded road table (grade +-0.10 rad, bank +-0.12 rad) on every handle")
    ap.add_argument("--actuator", default=None, help="TAUD,TAUP: the actuator lag (seconds, steering and pedal) on every handle")
    args = ap.parse_args()
    global INTEGRATION, TERMS, OBJECTIVE, COUPLING, LOAD_TRANSFER, DOWNFORCE, SURFACE, ACTUATOR, ROAD
    SURFACE = bool(args.surface)
    ROAD = bool(args.road)
    if args.actuator is not None:
        ACTUATOR = tuple(float(v) for v in args.actuator.split(","))
        if len(ACTUATOR) != 2:
            ap.error("--actuator takes TAUD,TAUP")
    if args.downforce is not None:
        aero = tuple(float(v) for v in args.downforce.split(","))
        if len(aero) not in (2, 3):
            ap.error("--downforce takes KF,KR or KF,KR,VSAT")
        DOWNFORCE = aero + (100.0,) if len(aero) == 2 else aero
    if args.load_transfer is not None:
        load = tuple(float(v) for v in args.load_transfer.split(","))
        if len(load) not in (1, 2):
            ap.error("--load-transfer takes H or H,FRAC")
        LOAD_TRANSFER = load + (0.9,) if len(load) == 1 else load
    if args.coupling is not None:
        ratios = tuple(float(v) for v in args.coupling.split(","))
        if len(ratios) not in (1, 2):
            ap.error("--coupling takes RF,RR or one ratio")
        COUPLING = ratios * 2 if len(ratios) == 1 else ratios
    TERMS = dict(TERMS_ON) if args.terms else None
    OBJECTIVE = dict(OBJECTIVE_ON) if args.objective else None
    INTEGRATION = (args.substeps, None if args.blend is None else tuple(float(v) for v in args.blend.split(",")))
    if args.update == "softmin" and not args.optimize:
        ap.error("--update softmin goes with --optimize")
    if args.identify:
        emit(args, measure_identify(args))
        return
    if args.trace:
        emit(args, measure_trace(args))
        return
    if args.sampled or args.optimize:
        ks = [int(k) for k in (args.vehicles or "1").split(",")]
        run = measure_sampled if args.sampled else measure_softmin_round if args.update == "softmin" else measure_optimize
        name = "--sampled" if args.sampled else "--optimize" + (" --update softmin" if args.update == "softmin" else "")
        emit(args, {"tool": "tools/bench_dynamic.py " + name, "by_vehicles": {str(k): run(args, k) for k in ks}})
        return
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


def emit(args, result):
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as handle:
            handle.write(line + "\n")


GRIPS = (1.0, 0.9, 1.1, 0.8, 1.2, 0.7, 1.05, 0.95)


def _engine(dp, P, N, n, K, reduce, stream, **extra):
    from acmpc_amd import DynamicBicycleParams, Engine
    eng = Engine(**dict(dp["kw"], max_problems=P, max_candidates=N, max_steps=n, nn_window=(2, 5), **extra))
    if K == 1:
        eng.set_dynamics(DynamicBicycleParams.reference())
    else:
        eng.set_dynamics_ensemble([DynamicBicycleParams.reference().with_grip(g) for g in GRIPS[:K]], reduce=reduce)
    eng.set_paths(np.repeat(dp["table"][None], P, axis=0))
    eng.sync_tables(stream)
    return integrate(eng)


def _centre(dp, P, n):
    import acmpc_oracle as orc
    d_ref = np.arctan(float(dp["kw"]["wheelbase"]) * dp["table"][orc.ROW_KAPPA])[:n]
    return np.repeat(np.stack([d_ref, np.full(n, 0.2)], axis=1)[None], P, axis=0).astype(np.float32)


SIGMA = (0.05, 0.3)


def measure_optimize(args, K, out=None):
    """p50 / p99 of one acmpc_optimize, 16 384 candidates x 49 steps, 2 rounds (host-synchronised: the call returns the
    record); with the handle's ACMPC_DYNAMIC_MATRIX_ROUNDS too where the library knows the option."""
    import torch
    import acmpc_oracle as orc
    import dynamic_spec as ds
    from acmpc_amd import EngineError

    H, N, rounds = 50, 16384, 2
    n = H - 1
    dp = ds.make_dynamic_problem(orc, "monza", H, 8, 0)
    out = {} if out is None else out
    eng = _engine(dp, 1, N, n, K, args.reduce, torch.cuda.current_stream().cuda_stream)
    x0, centre = dp["x0"][None], _centre(dp, 1, n)
    forms = [("optimize_16384x2", None)]
    try:
        eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", None)
        forms.append(("optimize_16384x2_matrix_rounds", "1"))
    except EngineError:
        pass   # (an earlier library: three launches per round is all it has)
    for name, option in forms:
        if option is not None:
            eng.set_option("ACMPC_DYNAMIC_MATRIX_ROUNDS", option)
        lat = []
        for i in range(20 + (20 if args.quick else 400)):
            t0 = time.perf_counter()
            eng.optimize(x0, centre, None, N, rounds, SIGMA, shrink=0.5, seed=i)
            if i >= 20:
                lat.append(time.perf_counter() - t0)
        out[name] = dict(p50_ms=float(np.percentile(lat, 50)) * 1e3, p99_ms=float(np.percentile(lat, 99)) * 1e3,
                         calls=len(lat))
    eng.close()
    return out


def measure_softmin_round(args, K):
    """One softmin round of acmpc_optimize built from device calls, the matrix-free form against the form through the
    control matrix (what a library without acmpc_softmin_sampled_device has), at 16 384 x 49 on one problem and at
    4 096 x 4 096 x 49: device-event times of the whole round and of its softmin call alone."""
    import torch
    import acmpc_oracle as orc
    import dynamic_spec as ds
    from acmpc_amd import _capi

    H = 50
    n = H - 1
    dp = ds.make_dynamic_problem(orc, "monza", H, 8, 0)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    reps = 3 if args.quick else args.reps
    out = {"horizon": H, "search": "window (2, 5)", "vehicles": K, "softmin_lambda": 1.0, "repetitions": reps}
    for name, P, N in (("16384x1", 1, 16384), ("4096x4096", 4096, 4096)):
        eng = _engine(dp, P, N, n, K, args.reduce, s, softmin_lambda=1.0)
        U = torch.empty(P, n, 2, N, device=dev)
        x0 = torch.tensor(np.repeat(dp["x0"][None], P, axis=0), device=dev)
        centre = torch.tensor(_centre(dp, P, n), device=dev)
        costs = torch.empty(P, N, device=dev)
        keys = torch.empty(P, dtype=torch.int64, device=dev)
        recs = torch.empty(P, _capi.record_floats(n), device=dev)
        means = [torch.empty(P, n, 2, device=dev) for _ in range(2)]

        def softmin_sampled():
            eng.softmin_sampled_device(costs.data_ptr(), keys.data_ptr(), centre.data_ptr(), 2 * n, 0, P, N, n, 0, SIGMA, 7,
                                       1, means[0].data_ptr(), 0, s)

        def softmin_matrix():
            eng.softmin_device(costs.data_ptr(), keys.data_ptr(), U.data_ptr(), P, N, n, 1, means[1].data_ptr(), 0, s)

        def round_sampled():
            eng.rollout_sampled_device(x0.data_ptr(), centre.data_ptr(), 2 * n, 0, P, N, n, 0, SIGMA, 7, 1, costs.data_ptr(),
                                       keys.data_ptr(), s)
            eng.finalize_sampled_device(keys.data_ptr(), x0.data_ptr(), centre.data_ptr(), 2 * n, 0, P, N, n, SIGMA, 7, 1,
                                        recs.data_ptr(), s)
            softmin_sampled()

        def round_matrix():
            eng.sample_device(centre.data_ptr(), 2 * n, 0, P, N, n, 1, 0, SIGMA, 7, 1, U.data_ptr(), s)
            eng.solve_device(x0.data_ptr(), U.data_ptr(), P, N, n, 1, costs.data_ptr(), keys.data_ptr(), recs.data_ptr(), s)
            softmin_matrix()

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        forms = (("round_matrix", round_matrix), ("round_sampled", round_sampled), ("softmin_matrix", softmin_matrix),
                 ("softmin_sampled", softmin_sampled))
        times = {label: [] for label, _ in forms}
        for _, call in forms:   # every shape warm before anything is timed
            call()
        torch.cuda.synchronize()
        for _ in range(reps):   # the forms alternate inside every repetition
            for label, call in forms:
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                times[label].append(e0.elapsed_time(e1))
        same = bool(torch.equal(means[0].view(torch.int32), means[1].view(torch.int32)))
        shape = dict(P=P, N=N, matrix_bytes=P * N * n * 8, means_equal_bit_for_bit=same)
        for label, _ in forms:
            t = np.asarray(times[label])
            shape[label + "_ms"] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))
        shape["round_sampled_over_matrix"] = shape["round_sampled_ms"]["median"] / shape["round_matrix_ms"]["median"]
        shape["softmin_sampled_over_matrix"] = shape["softmin_sampled_ms"]["median"] / shape["softmin_matrix_ms"]["median"]
        out[name] = shape
        eng.close()
        del U
        torch.cuda.empty_cache()
    return out


def measure_identify(args):
    """acmpc_score_grips on a log driven at grip (0.5, 0.7): the call's latency at the four shapes, and what the step
    kernel's instructions cost at the vector-issue rate."""
    import bench
    import grip_spec as gs
    from acmpc_amd import DynamicBicycleParams, Engine, _capi
    from acmpc_amd.grip_estimator import grip_scales

    base = DynamicBicycleParams.reference()
    W = 40
    states, controls = gs.steering_log(base.with_axle_grip(0.5, 0.7), 0.02, steps=W)
    eng = Engine(mode=_capi.MODE_DYNAMIC, max_problems=1, max_candidates=64, max_steps=8, step_cost=(1.0, 1.0, 0.0),
                 r_term=(0.5, 10.0), final_cost=(1.0, 1.0, 0.0), u_min=(-0.3, -1.0), u_max=(0.3, 1.0), margin=0.0,
                 wheelbase=base.lf + base.lr, dt=0.05)
    eng.set_dynamics(base)
    integrate(eng)
    mix, mix_path = bench.newest_profile("isa_mix.json")
    M = INTEGRATION[0]
    entry = "identify_grip_aero" if DOWNFORCE is not None else "identify_grip_loaded" if LOAD_TRANSFER is not None else "identify_grip_coupled" if COUPLING is not None else "identify_grip"
    per_step = M * sum(mix["entries"][entry]["valu"].values()) + sum(mix["entries"][entry + "_step"]["valu"].values())
    out = {"tool": "tools/bench_dynamic.py --identify", "W": W, "substeps": M, "low_speed_blend": INTEGRATION[1],
           "valu_per_hypothesis_step": per_step}
    if COUPLING is not None:
        out["coupling"] = list(COUPLING)
    if LOAD_TRANSFER is not None:
        out["load_transfer"] = list(LOAD_TRANSFER)
    if DOWNFORCE is not None:
        out["downforce"] = list(DOWNFORCE)
    calls = 20 if args.quick else 200
    for side in (64, 256):
        scales = grip_scales(np.linspace(0.3, 1.5, side), "split")
        K = scales.shape[0]
        for L in (1, 8):
            lat = []
            for i in range(10 + calls):
                t0 = time.perf_counter()
                errors, best = eng.score_grips(states, controls, 0.05, scales, segment=L)
                if i >= 10:
                    lat.append(time.perf_counter() - t0)
            p50 = float(np.percentile(lat, 50))
            counted = (float(per_step), mix_path + " (static count: M sub-step trips + the step loop's rest)",
                       {"source_sha256": mix.get("source_sha256")})
            roof, _ = bench.valu_roofline(counted, K, W, p50, mix_entry=entry, cpt=1)
            out["K%d_L%d" % (K, L)] = dict(K=K, L=L, segments=(W + L - 1) // L, p50_ms=p50 * 1e3,
                                           p99_ms=float(np.percentile(lat, 99)) * 1e3, calls=len(lat),
                                           best=[float(v) for v in scales[best]], error_best=float(errors[best]),
                                           vector_issue_time_over_call_p50=roof["frac"],
                                           opcode_mix_matches_loaded_sources=roof["opcode_mix_matches_loaded_sources"])
    eng.close()
    return out


def measure_trace(args):
    """acmpc_trace_plans' latency at the two shapes DESIGN.md section 4.10 records."""
    import acmpc_oracle as orc
    import dynamic_spec as ds

    n = 49
    dp = ds.make_dynamic_problem(orc, "monza", n + 1, 64, 0)
    out = {"tool": "tools/bench_dynamic.py --trace", "substeps": INTEGRATION[0], "low_speed_blend": INTEGRATION[1]}
    calls = 20 if args.quick else 200
    for M, K in ((1, 1), (64, 8)):
        eng = _engine(dp, 1, 64, n, K, args.reduce, 0)
        U = np.ascontiguousarray(dp["U"][None, :M])
        x0 = dp["x0"][None]
        shape = {"P": 1, "M": M, "K": K, "n": n}
        for name, want in (("all_outputs", ("states", "totals", "terms")), ("states_only", ("states",))):
            lat = []
            for i in range(10 + calls):
                t0 = time.perf_counter()
                eng.trace_plans(x0, U, want=want)
                if i >= 10:
                    lat.append(time.perf_counter() - t0)
            shape[name] = dict(p50_ms=float(np.percentile(lat, 50)) * 1e3, p99_ms=float(np.percentile(lat, 99)) * 1e3, calls=len(lat))
        out["M%d_K%d" % (M, K)] = shape
        eng.close()
    return out


def measure_sampled(args, K):
    import torch
    import acmpc_oracle as orc
    import bench
    import dynamic_spec as ds

    H = 50
    n = H - 1
    dp = ds.make_dynamic_problem(orc, "monza", H, 8, 0)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    reps = 3 if args.quick else args.reps
    out = {"tool": "tools/bench_dynamic.py --sampled", "horizon": H, "search": "window (2, 5)", "vehicles": K}
    entry = "dynamic_sampled" if K == 1 else "dynamic_sampled_ensemble"
    for name, P, N in (("4096x4096", 4096, 4096), ("1M", 256, 4096)):
        eng = _engine(dp, P, N, n, K, args.reduce, s)
        U = torch.empty(P, n, 2, N, device=dev)
        x0 = torch.tensor(np.repeat(dp["x0"][None], P, axis=0), device=dev)
        centre = torch.tensor(_centre(dp, P, n), device=dev)

        def sample():
            eng.sample_device(centre.data_ptr(), 2 * n, 0, P, N, n, 1, 0, SIGMA, 7, 1, U.data_ptr(), s)

        def rollout():
            eng.rollout_device(x0.data_ptr(), U.data_ptr(), P, N, n, 1, 0, 0, 0, s)

        def pair():
            sample()
            rollout()

        def fused():
            eng.rollout_sampled_device(x0.data_ptr(), centre.data_ptr(), 2 * n, 0, P, N, n, 0, SIGMA, 7, 1, 0, 0, s)

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {}
        for _ in range(2):   # (the whole set twice, the second kept: every form measured warm, interleaved with the others)
            for label, call in (("pair", pair), ("sample", sample), ("rollout", rollout), ("fused", fused)):
                call()
                torch.cuda.synchronize()
                times = []
                for _ in range(reps):
                    e0.record()
                    call()
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1))
                ms[label] = float(np.median(times))
        roof = issue_roof(bench, P * N * K, n, ms["fused"] * 1e-3, entry)
        out[name] = dict(P=P, N=N, pair_ms=ms["pair"], sample_ms=ms["sample"], rollout_ms=ms["rollout"], fused_ms=ms["fused"],
                         fused_over_pair=ms["fused"] / ms["pair"], fused_over_rollout=ms["fused"] / ms["rollout"],
                         fused_vehicle_candidate_steps_per_s=P * N * K * n / (ms["fused"] * 1e-3),
                         matrix_bytes=P * N * n * 8, fused_vector_issue_roof_frac=roof["frac"],
                         valu_per_candidate_step=roof["valu_instructions_per_candidate_step"],
                         opcode_mix_matches_loaded_sources=roof["opcode_mix_matches_loaded_sources"])
        eng.close()
        del U
        torch.cuda.empty_cache()
    return measure_optimize(args, K, out)


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
    if INTEGRATION != (1, None):
        out.update(substeps=INTEGRATION[0], low_speed_blend=INTEGRATION[1])
    if OBJECTIVE is not None:
        out.update(objective={k: list(v) if isinstance(v, tuple) else v for k, v in OBJECTIVE.items()})
    if TERMS is not None:
        out.update(terms={k: list(v) if isinstance(v, tuple) else v for k, v in TERMS.items()})
    if COUPLING is not None:
        out.update(coupling=list(COUPLING))
    if LOAD_TRANSFER is not None:
        out.update(load_transfer=list(LOAD_TRANSFER))
    if DOWNFORCE is not None:
        out.update(downforce=list(DOWNFORCE))
    if SURFACE:
        out.update(surface="uniform [0.5, 1], seed %d" % SURFACE_SEED)
    if ROAD:
        out.update(road="grade uniform +-0.10 rad, bank uniform +-0.12 rad, seed %d" % ROAD_SEED)
    if ACTUATOR is not None:
        out.update(actuator=list(ACTUATOR))
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
        return integrate(eng)

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
