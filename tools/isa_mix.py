#!/usr/bin/env python3
"""Development tool: the VALU opcode mix of the instruction-bound kernels' hot loops, from the compiler's own assembly.

Compiles the sources of the named kernels (csrc/acmpc_kernels_temporal.hip, csrc/acmpc_kernels.hip, mode D's units) with the library's flags + --save-temps in a scratch
directory, takes the innermost loops of the named kernels (tools/isa_loops.py) and writes
profiles/<tag>_isa_mix.json: per entry the static opcode histogram of ONE trip of the loop (one wave-step), the wave's
candidates per lane, and the sha256 of the sources it was compiled from - bench.py prices the mix with the issue costs of
profiles/<tag>_valu_probe.json (tools/valu_probe.hip) and flags a mix whose sources are not the loaded library's.

usage: python3 tools/isa_mix.py r04        (CPU only: hipcc cross-compiles)"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ac-mpc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from acmpc_amd import _build  # noqa: E402
from isa_loops import loops  # noqa: E402

# entry -> (source, kernel name substring, how to recognise the loop: (opcode, count) pairs that must match)
ENTRIES = {
    "window_2_5": ("acmpc_kernels_temporal.hip", "rollout_kernelILi1ELi1ELi2ELi256ELi1ELi8E", {"ds_read_b128": 16}),
    "window_1_2": ("acmpc_kernels_temporal.hip", "rollout_kernelILi1ELi1ELi2ELi256ELi1ELi8E", {"ds_read_b128": 10}),
    "exhaustive": ("acmpc_kernels_temporal.hip", "rollout_kernelILi1ELi1ELi2ELi256ELi1ELi8E", {"ds_read_b128": 20}),
    # the fused sample + rollout round: its step loop comes in several unrolled pieces of one mix; the largest stands for it
    # (the SQ count per candidate-step also holds the Philox draws and the staging, priced with the same mix)
    "fused_round": ("acmpc_kernels.hip", "rollout_sampled_kernelILi0E", None),
    # mode D (the dynamic bicycle, two candidates per lane, step-major): the largest step loop - a windowed search's, whose
    # trip is the dynamics + an unrolled window + the cost; the exhaustive form adds its waypoint loop to the same trip
    "dynamic": ("acmpc_dynamic.hip", "rollout_dynamic_kernelILi1ELi2ELb0EJEEE", None),
    # mode D with an ensemble of vehicles (one wavefront per vehicle): the same step loop under wave k's vehicle
    "dynamic_ensemble": ("acmpc_dynamic.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb0EJEEE", None),
    # mode D drawing its own candidates (two per lane): the same step loop with the blend of the step's control in front.
    # The loop holds the Philox draws as loops of its own, run on at most seven of a rollout's trips: the mix is the trip
    # without them (OUTER)
    "dynamic_sampled": ("acmpc_dynamic.hip", "rollout_dynamic_sampled_kernelILi2ELb0EJEEE", None),
    "dynamic_sampled_ensemble": ("acmpc_dynamic.hip", "rollout_dynamic_sampled_ensemble_kernelILi2ELb0EJEEE", None),
    # mode D with an integration setting (the FINE kernels): a control step is the step loop's own trip - the control's
    # terms, the search, the cost (`_step`: the trip less its inner loop, OUTER) - plus M trips of the sub-step loop, the
    # dynamics and the blend (`_substep`, the largest innermost loop, the blend's block counted): VALU per control step =
    # step + M substep
    "dynamic_fine_step": ("acmpc_dynamic.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJEEE", None),
    "dynamic_fine_substep": ("acmpc_dynamic.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJEEE", None),
    "dynamic_ensemble_fine_step": ("acmpc_dynamic.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJEEE", None),
    "dynamic_ensemble_fine_substep": ("acmpc_dynamic.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJEEE", None),
    # mode D with rate and slip terms (acmpc_set_dynamics_terms: the kernels of acmpc_dynamic_terms.hip, the FINE step plus
    # the terms after the cost): the same two loops.  The terms' block is in the step loop's own trip: its instructions =
    # `dynamic_terms_step` - `dynamic_fine_step`, both parts on (the count is static: a part that is off is branched over)
    "dynamic_terms_step": ("acmpc_dynamic_terms.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_5TermsEEE", None),
    "dynamic_terms_substep": ("acmpc_dynamic_terms.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_5TermsEEE", None),
    "dynamic_ensemble_terms_step": ("acmpc_dynamic_terms.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_5TermsEEE", None),
    "dynamic_ensemble_terms_substep": ("acmpc_dynamic_terms.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_5TermsEEE", None),
    # mode D with the objective (acmpc_set_dynamics_objective: the TermsObjective kernels of the same unit, all four parts):
    # the ceiling's block is in the step loop's own trip - `dynamic_objective_step` - `dynamic_terms_step` - and the progress
    # part is outside both loops, once per candidate
    "dynamic_objective_step": ("acmpc_dynamic_terms.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_14TermsObjectiveEEE", None),
    "dynamic_objective_substep": ("acmpc_dynamic_terms.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_14TermsObjectiveEEE", None),
    "dynamic_ensemble_objective_step": ("acmpc_dynamic_terms.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_14TermsObjectiveEEE", None),
    "dynamic_ensemble_objective_substep": ("acmpc_dynamic_terms.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_14TermsObjectiveEEE", None),
    # mode D with the tyre coupling (acmpc_set_dynamics_coupling: the TermsCoupled kernels of acmpc_dynamic_coupled.hip, the
    # general step with the friction-ellipse block in every sub-step and all four term parts): the block's instructions =
    # `dynamic_coupled_substep` - `dynamic_objective_substep` - per axle the clip, an IEEE division and a correctly rounded
    # square root
    "dynamic_coupled_step": ("acmpc_dynamic_coupled.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12TermsCoupledEEE", None),
    "dynamic_coupled_substep": ("acmpc_dynamic_coupled.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12TermsCoupledEEE", None),
    "dynamic_ensemble_coupled_step": ("acmpc_dynamic_coupled.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12TermsCoupledEEE", None),
    "dynamic_ensemble_coupled_substep": ("acmpc_dynamic_coupled.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12TermsCoupledEEE", None),
    # mode D with the load transfer (acmpc_set_dynamics_load_transfer: the TermsLoaded kernels of acmpc_dynamic_loaded.hip, the
    # coupled step with the loaded peaks in front of it): the block's instructions = `dynamic_loaded_substep` -
    # `dynamic_coupled_substep` - two clips at the static caps, the transfer and its clip, two quadratics, two products, and
    # the caps per lane instead of per wave
    "dynamic_loaded_step": ("acmpc_dynamic_loaded.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_11TermsLoadedEEE", None),
    "dynamic_loaded_substep": ("acmpc_dynamic_loaded.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_11TermsLoadedEEE", None),
    "dynamic_ensemble_loaded_step": ("acmpc_dynamic_loaded.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_11TermsLoadedEEE", None),
    "dynamic_ensemble_loaded_substep": ("acmpc_dynamic_loaded.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_11TermsLoadedEEE", None),
    # mode D with the downforce (acmpc_set_dynamics_downforce: the TermsAero kernels of acmpc_dynamic_aero.hip, the loaded step
    # with the downforce of the sub-step's speed under the load moved): the block's instructions = `dynamic_aero_substep` -
    # `dynamic_loaded_substep` - the clip at v_sat, the square, two products, two more quadratics and products for the caps at
    # this speed, and the caps' negations per lane
    "dynamic_aero_step": ("acmpc_dynamic_aero.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_9TermsAeroEEE", None),
    "dynamic_aero_substep": ("acmpc_dynamic_aero.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_9TermsAeroEEE", None),
    "dynamic_ensemble_aero_step": ("acmpc_dynamic_aero.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_9TermsAeroEEE", None),
    "dynamic_ensemble_aero_substep": ("acmpc_dynamic_aero.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_9TermsAeroEEE", None),
    # mode D with a surface table (acmpc_set_surface: the TermsSurface kernels of acmpc_dynamic_surface.hip, the aero step on
    # per-lane peaks): the table's instructions = `dynamic_surface_step` - `dynamic_aero_step` - the gather's address arithmetic,
    # its loads and the two multiplies, once per control step; the sub-step differs by what per-lane peaks cost against scalars
    "dynamic_surface_step": ("acmpc_dynamic_surface.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12TermsSurfaceEEE", None),
    "dynamic_surface_substep": ("acmpc_dynamic_surface.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12TermsSurfaceEEE", None),
    "dynamic_ensemble_surface_step": ("acmpc_dynamic_surface.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12TermsSurfaceEEE", None),
    "dynamic_ensemble_surface_substep": ("acmpc_dynamic_surface.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12TermsSurfaceEEE", None),
    # mode D with the actuator lag (acmpc_set_dynamics_actuator: the WithActuator kernels of acmpc_dynamic_actuator.hip): the aero
    # step, or the surface step, driven on the lagged control - `dynamic_actuator_step` - `dynamic_aero_step` is the filter's six
    # subtractions and four multiplies (packed: one instruction per pair of candidates) and what carrying two more values costs
    "dynamic_actuator_step": ("acmpc_dynamic_actuator.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_9TermsAeroEEEEE", None),
    "dynamic_actuator_substep": ("acmpc_dynamic_actuator.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_9TermsAeroEEEEE", None),
    "dynamic_ensemble_actuator_step": ("acmpc_dynamic_actuator.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_9TermsAeroEEEEE", None),
    "dynamic_ensemble_actuator_substep": ("acmpc_dynamic_actuator.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_9TermsAeroEEEEE", None),
    "dynamic_actuator_surface_step": ("acmpc_dynamic_actuator.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_12TermsSurfaceEEEEE", None),
    "dynamic_actuator_surface_substep": ("acmpc_dynamic_actuator.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_12TermsSurfaceEEEEE", None),
    "dynamic_ensemble_actuator_surface_step": ("acmpc_dynamic_actuator.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_12TermsSurfaceEEEEE", None),
    "dynamic_ensemble_actuator_surface_substep": ("acmpc_dynamic_actuator.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_12TermsSurfaceEEEEE", None),
    # mode D with a road table (acmpc_set_road: the TermsRoad kernels of acmpc_dynamic_road.hip, the surface step with the row's n_z
    # in the peaks and its two accelerations in every sub-step): `dynamic_road_step` - `dynamic_surface_step` is the 16-byte
    # gather, the surface's switch and the two extra multiplies, once per control step; `dynamic_road_substep` -
    # `dynamic_surface_substep` the two adds; `dynamic_actuator_road_*` the same under the lag (acmpc_dynamic_road_actuator.hip)
    "dynamic_road_step": ("acmpc_dynamic_road.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_9TermsRoadEEE", None),
    "dynamic_road_substep": ("acmpc_dynamic_road.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_9TermsRoadEEE", None),
    "dynamic_ensemble_road_step": ("acmpc_dynamic_road.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_9TermsRoadEEE", None),
    "dynamic_ensemble_road_substep": ("acmpc_dynamic_road.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_9TermsRoadEEE", None),
    "dynamic_actuator_road_step": ("acmpc_dynamic_road_actuator.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_9TermsRoadEEEEE", None),
    "dynamic_actuator_road_substep": ("acmpc_dynamic_road_actuator.hip", "rollout_dynamic_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_9TermsRoadEEEEE", None),
    "dynamic_ensemble_actuator_road_step": ("acmpc_dynamic_road_actuator.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_9TermsRoadEEEEE", None),
    "dynamic_ensemble_actuator_road_substep": ("acmpc_dynamic_road_actuator.hip", "rollout_dynamic_ensemble_kernelILi1ELi2ELb1EJNS_12WithActuatorINS_9TermsRoadEEEEE", None),
    # mode D's grip identification (acmpc_score_grips, one hypothesis per lane): the sub-step loop of its step kernel - the
    # dynamics and the blend's block, WITHOUT the pose (nothing reads it there: no sincos_spec(yaw), no X, Y, yaw updates).
    # VALU per hypothesis and control step = M trips of it + `identify_grip_step`: the control's terms and the residual, the
    # step loop's own trip (OUTER)
    "identify_grip": ("acmpc_identify.hip", "identify_grip_kernel", None),
    "identify_grip_step": ("acmpc_identify.hip", "identify_grip_kernel", None),
    # the same under the tyre coupling (each lane's caps from its own two peaks): the block = the difference of the sub-steps
    "identify_grip_coupled": ("acmpc_identify.hip", "identify_grip_coupled_kernel", None),
    "identify_grip_coupled_step": ("acmpc_identify.hip", "identify_grip_coupled_kernel", None),
    # and under the load transfer (the base vehicle's factors on each lane's own two peaks)
    "identify_grip_loaded": ("acmpc_identify.hip", "identify_grip_loaded_kernel", None),
    "identify_grip_loaded_step": ("acmpc_identify.hip", "identify_grip_loaded_kernel", None),
    # and under the downforce (the handle's coefficients and the base vehicle's factors on each lane's own two peaks)
    "identify_grip_aero": ("acmpc_identify.hip", "identify_grip_aero_kernel", None),
    "identify_grip_aero_step": ("acmpc_identify.hip", "identify_grip_aero_kernel", None),
}
CANDIDATES_PER_LANE = {"fused_round": 1, "identify_grip": 1, "identify_grip_step": 1, "identify_grip_coupled": 1,
                       "identify_grip_coupled_step": 1, "identify_grip_loaded": 1, "identify_grip_loaded_step": 1,
                       "identify_grip_aero": 1, "identify_grip_aero_step": 1}
OUTER = ("dynamic_sampled", "dynamic_sampled_ensemble", "dynamic_fine_step", "dynamic_ensemble_fine_step",
         "dynamic_terms_step", "dynamic_ensemble_terms_step", "dynamic_objective_step", "dynamic_ensemble_objective_step",
         "dynamic_coupled_step", "dynamic_ensemble_coupled_step", "dynamic_loaded_step", "dynamic_ensemble_loaded_step",
         "dynamic_aero_step", "dynamic_ensemble_aero_step", "dynamic_surface_step", "dynamic_ensemble_surface_step",
         "dynamic_actuator_step", "dynamic_ensemble_actuator_step", "dynamic_actuator_surface_step",
         "dynamic_ensemble_actuator_surface_step", "dynamic_road_step", "dynamic_ensemble_road_step",
         "dynamic_actuator_road_step", "dynamic_ensemble_actuator_road_step",
         "identify_grip_step", "identify_grip_coupled_step", "identify_grip_loaded_step", "identify_grip_aero_step")
# (exit test at the head: closes with s_branch)
ROTATED = ("dynamic_fine_substep", "dynamic_ensemble_fine_substep", "dynamic_terms_substep", "dynamic_ensemble_terms_substep",
           "dynamic_objective_substep", "dynamic_ensemble_objective_substep", "dynamic_coupled_substep",
           "dynamic_ensemble_coupled_substep", "dynamic_loaded_substep", "dynamic_ensemble_loaded_substep", "dynamic_aero_substep",
           "dynamic_ensemble_aero_substep", "dynamic_surface_substep", "dynamic_ensemble_surface_substep",
           "dynamic_actuator_substep", "dynamic_ensemble_actuator_substep", "dynamic_actuator_surface_substep",
           "dynamic_ensemble_actuator_surface_substep", "dynamic_road_substep", "dynamic_ensemble_road_substep",
           "dynamic_actuator_road_substep", "dynamic_ensemble_actuator_road_substep", "identify_grip",
           "identify_grip_coupled", "identify_grip_loaded", "identify_grip_aero")


def source_hash():
    h = hashlib.sha256()
    for name in sorted(_build.SOURCES + _build.HEADERS):
        with open(os.path.join(_build.CSRC_DIR, name), "rb") as handle:
            h.update(handle.read())
    h.update(_build.flag_record().encode())
    return h.hexdigest()


def assembly(source, scratch):
    flags = list(_build.HIPCC_FLAGS) + list(_build.EXTRA_FLAGS.get(source, ()))
    subprocess.run([_build.find_hipcc(), *flags, "-w", "-c", os.path.join(_build.CSRC_DIR, source), "-o",
                    os.path.join(scratch, "unit.o"), "--save-temps"], check=True, cwd=scratch)
    stem = os.path.splitext(source)[0]
    return os.path.join(scratch, stem + "-hip-amdgcn-amd-amdhsa-gfx950.s")


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "r04"
    out = {"tool": "tools/isa_mix.py " + tag, "source_sha256": source_hash(), "build_flags": _build.flag_record(),
           "unit": "instructions of ONE trip of the step loop = one wave-step (64 lanes x candidates_per_lane candidates)",
           "entries": {}}
    cache = {}
    with tempfile.TemporaryDirectory() as scratch:
        for entry, (source, kernel, signature) in ENTRIES.items():
            if source not in cache:
                cache[source] = assembly(source, scratch)
            every = loops(cache[source], kernel, outer=entry in OUTER, rotated=entry in ROTATED)
            if signature is None:
                found = [max(every, key=lambda lh: sum(lh[1].values()))]
            else:
                found = [(label, h) for label, h in every if all(h.get(op, 0) == count for op, count in signature.items())]
            if len(found) != 1:
                raise SystemExit("%s: %d loops match %r" % (entry, len(found), signature))
            label, hist = found[0]
            out["entries"][entry] = {"kernel": kernel, "loop": label, "candidates_per_lane": CANDIDATES_PER_LANE.get(entry, 2),
                                     "valu": {op: c for op, c in sorted(hist.items()) if op.startswith("v_")},
                                     "lds": {op: c for op, c in sorted(hist.items()) if op.startswith("ds_")},
                                     "salu": sum(c for op, c in hist.items() if op.startswith("s_")),
                                     "vmem": {op: c for op, c in sorted(hist.items())
                                              if op.startswith("global_") or op.startswith("buffer_")}}
    path = os.path.join(ROOT, "profiles", tag + "_isa_mix.json")
    with open(path, "w") as handle:
        json.dump(out, handle, indent=1)
    for entry, e in out["entries"].items():
        print(entry, e["loop"], "VALU", sum(e["valu"].values()), "LDS", sum(e["lds"].values()), "SALU", e["salu"])


if __name__ == "__main__":
    main()
