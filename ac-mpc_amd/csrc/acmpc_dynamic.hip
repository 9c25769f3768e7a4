// Mode D's public launchers (acmpc_dynamic.h): the launch shape, the dispatch over the handle's settings to the unit that
// holds their kernels, and the kernels of no setting but the integration's - the templates of acmpc_dynamic_kernels.h with
// the empty pack, FINE = false and FINE = true.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

int dynamic_candidates_per_lane(int P, int N, int K) {
  // 256 CUs x 4 SIMDs x 8 waves x 64 lanes = 524 288 lanes: two candidates per lane once every lane would get two
  // (an ensemble's lanes are P N K: one per vehicle and candidate)
  return (static_cast<int64_t>(P) * N * K >= (int64_t{1} << 20)) ? 2 : 1;
}

int dynamic_blocks_per_problem(int P, int N, int K) {
  const int per_block = (K > 1 ? kWave : kDynBlock) * dynamic_candidates_per_lane(P, N, K);
  return (N + per_block - 1) / per_block;
}

hipError_t launch_rollout_dynamic(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                  const Integration& g, const WithActuator<WithObstacles<TermsRoad>>& road, hipStream_t s) {
  if (has_road(road)) return launch_rollout_dynamic_road(layout, args, vehicles, g, road, s);
  const WithActuator<WithObstacles<TermsSurface>> tm = below_road(road);
  if (has_actuator(tm)) return launch_rollout_dynamic_actuator(layout, args, vehicles, g, tm, s);
  if (has_obstacles(tm)) return launch_rollout_dynamic_obstacles(layout, args, vehicles, g, tm, s);
  if (has_surface(tm)) return launch_rollout_dynamic_surface(layout, args, vehicles, g, tm, s);
  if (has_downforce(tm)) return launch_rollout_dynamic_aero(layout, args, vehicles, g, tm, s);
  if (has_load_transfer(tm)) return launch_rollout_dynamic_loaded(layout, args, vehicles, g, tm, s);
  if (has_coupling(tm)) return launch_rollout_dynamic_coupled(layout, args, vehicles, g, tm, s);
  if (has_terms(tm) || has_objective(tm)) return launch_rollout_dynamic_terms(layout, args, vehicles, g, tm, s);
  return rollout_dynamic_launch(layout, args, vehicles, g, s);
}

hipError_t launch_rollout_dynamic_sampled(const RolloutArgs& args, const SampleArgs& sample, const VehicleEnsemble& vehicles,
                                          const Integration& g, const WithActuator<WithObstacles<TermsRoad>>& road, hipStream_t s) {
  if (has_road(road)) return launch_rollout_dynamic_sampled_road(args, sample, vehicles, g, road, s);
  const WithActuator<WithObstacles<TermsSurface>> tm = below_road(road);
  if (has_actuator(tm)) return launch_rollout_dynamic_sampled_actuator(args, sample, vehicles, g, tm, s);
  if (has_obstacles(tm)) return launch_rollout_dynamic_sampled_obstacles(args, sample, vehicles, g, tm, s);
  if (has_surface(tm)) return launch_rollout_dynamic_sampled_surface(args, sample, vehicles, g, tm, s);
  if (has_downforce(tm)) return launch_rollout_dynamic_sampled_aero(args, sample, vehicles, g, tm, s);
  if (has_load_transfer(tm)) return launch_rollout_dynamic_sampled_loaded(args, sample, vehicles, g, tm, s);
  if (has_coupling(tm)) return launch_rollout_dynamic_sampled_coupled(args, sample, vehicles, g, tm, s);
  if (has_terms(tm) || has_objective(tm)) return launch_rollout_dynamic_sampled_terms(args, sample, vehicles, g, tm, s);
  return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s);
}

hipError_t launch_finalize_dynamic(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                   const Integration& g, const WithActuator<WithObstacles<TermsRoad>>& road, hipStream_t s) {
  if (has_road(road)) return launch_finalize_dynamic_road(layout, args, vehicles, g, road, s);
  const WithActuator<WithObstacles<TermsSurface>> tm = below_road(road);
  if (has_actuator(tm)) return launch_finalize_dynamic_actuator(layout, args, vehicles, g, tm, s);
  if (has_obstacles(tm)) return launch_finalize_dynamic_obstacles(layout, args, vehicles, g, tm, s);
  if (has_surface(tm)) return launch_finalize_dynamic_surface(layout, args, vehicles, g, tm, s);
  if (has_downforce(tm)) return launch_finalize_dynamic_aero(layout, args, vehicles, g, tm, s);
  if (has_load_transfer(tm)) return launch_finalize_dynamic_loaded(layout, args, vehicles, g, tm, s);
  if (has_coupling(tm)) return launch_finalize_dynamic_coupled(layout, args, vehicles, g, tm, s);
  if (has_terms(tm) || has_objective(tm)) return launch_finalize_dynamic_terms(layout, args, vehicles, g, tm, s);
  return finalize_dynamic_launch(layout, args, vehicles, g, s);
}

}  // namespace acmpc
