// The instantiations of acmpc_rollout.h's templates that are compiled with -fno-slp-vectorize (a flag is per unit; the
// measurements are with the launchers): mode T's step-major rollout on plain float32, the candidate-major rows kernel.
#include "acmpc_rollout.h"

namespace acmpc {

// Mode T on the step-major layout with one arithmetic state per candidate (plain v_*_f32 instructions).  The kernel is
// bound by instruction issue and by the latency of its two dependent LDS gathers per step, not by HBM: measured on
// MI355X (1 M candidates per launch) the compiler's SLP re-packing of neighbouring candidates into v_pk_* pairs costs
// 15 % at the 8-waypoint window (183 -> 155 us), because a packed instruction issues at half the rate of a plain one
// and the packing adds moves - so this translation unit is compiled with -fno-slp-vectorize (ac-mpc_amd/acmpc_amd/_build.py).
// (the candidate-major rows kernel gains the same way: its walk is one candidate per lane, and the SLP vectoriser's
// ten packed instructions + five moves per step cost more than the twenty plain ones they replace)
bool tile_rows_table_in_lds(const LaunchShape& shape, int P, int n) {
  // Table rows from LDS (one copy per workgroup) or by scalar loads - measured, 4 096 candidates per problem, LDS / scalar:
  //   H = 50:  256 problems 92 / 92 us, 1 024: 335 / 389, 4 096: 1 258 / 1 457   (more tables in flight, more scalar misses)
  //   H = 30:  256: 51.5 / 47.8, 1 024: 212 / 216;   H = 20, 2 048 problems: 297 / 280
  //   H = 65:  256: 183 / 173, 1 024: 654 / 685;     H = 80: 256: 221 / 220, 1 024: 799 / 1 094
  return shape.tile_table != 0 ? shape.tile_table == 1 : (n > 32 && (n <= 50 || P >= 512));   // (A/B: LaunchOptions::tile_table)
}

hipError_t launch_rollout_tile_rows_plain(const LaunchShape& shape, const RolloutArgs& args, hipStream_t s,
                                          hipEvent_t e0, hipEvent_t e1) {
  const bool lds = tile_rows_table_in_lds(shape, args.P, args.n);
  if (lds) {
    if (args.n <= 32) return launch_rollout_tile_rows<32, 4, true>(shape, args, s, e0, e1);
    if (args.n <= 50) return launch_rollout_tile_rows<50, 4, true>(shape, args, s, e0, e1);
    if (args.n <= 64) return launch_rollout_tile_rows<64, 4, true>(shape, args, s, e0, e1);
    return launch_rollout_tile_rows<kTileRowsMaxSteps, 4, true>(shape, args, s, e0, e1);
  }
  if (args.n <= 32) return launch_rollout_tile_rows<32, 4, false>(shape, args, s, e0, e1);
  if (args.n <= 50) return launch_rollout_tile_rows<50, 4, false>(shape, args, s, e0, e1);
  if (args.n <= 64) return launch_rollout_tile_rows<64, 4, false>(shape, args, s, e0, e1);
  return launch_rollout_tile_rows<kTileRowsMaxSteps, 4, false>(shape, args, s, e0, e1);
}

#ifdef ACMPC_T_STAMPS
}  // namespace acmpc
extern "C" int acmpc_debug_t_stamps(unsigned long long* out, int waves) {
  return static_cast<int>(hipMemcpyFromSymbol(out, HIP_SYMBOL(acmpc::g_t_stamps), static_cast<size_t>(waves) * 6 * sizeof(unsigned long long)));
}
namespace acmpc {
#endif
hipError_t launch_rollout_temporal_plain(const LaunchShape& shape, const RolloutArgs& args, hipStream_t s,
                                         hipEvent_t e0, hipEvent_t e1) {
  if (shape.block == 64 && shape.cpt == 1) return launch_rollout_t<1, 1, 1, 64, 1>(shape, args, s, e0, e1);
  if (shape.block == 256 && shape.cpt == 1) return launch_rollout_t<1, 1, 1, 256, 1>(shape, args, s, e0, e1);
  if (shape.block == 256 && shape.cpt == 2) {
    // two candidates per lane, the allocation capped for eight waves per SIMD (62 VGPRs either way since round 4's key
    // table).  Round 5: ONE instantiation for every search.  The uncapped one the 8-waypoint window used to take
    // (next_free_sgpr 74 against 72, otherwise the same resources) was dealt badly by the dispatcher in every launch
    // looked at: of 2 048 workgroups - eight per compute unit, all of which fit - 12 to 60 were held back until a first
    // workgroup had finished, 65 us into a 130 us launch, beside compute units that ran seven all along; this one starts
    // all 8 192 waves within 1.6 us, eight per SIMD (tools/modeT_stamps.py).
    RolloutArgs one = args;
    one.even_progress = static_cast<long long>(args.P) * shape.blocks_per_problem * (shape.block / kWave) <= 8 * 1024 ? 1 : 0;
    return launch_rollout_t<1, 1, 2, 256, 1, 8>(shape, one, s, e0, e1);
  }
  if (shape.block == 256 && shape.cpt == 4) return launch_rollout_t<1, 1, 4, 256, 1>(shape, args, s, e0, e1);
  return hipErrorInvalidConfiguration;
}

}  // namespace acmpc
