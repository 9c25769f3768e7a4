// Mode D's kernels with moving obstacles (acmpc_set_obstacles, acmpc_set_dynamics_clearance): the templates of
// acmpc_dynamic_kernels.h with a WithObstacles over TermsObjective, TermsCoupled, TermsLoaded and TermsAero - the step the handle would
// take without obstacles, the four term parts behind their switches, and the discs' lines after them.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

// The handle's settings over the pack of the step it would take without obstacles, with the launch's packed rows beside them;
// nothing is launched unless the obstacle data is what this launch's P and n index.  With a surface table set the surface unit's
// kernels over the obstacles' pack run instead (acmpc_dynamic_surface.hip).
bool obstacles_valid(const WithObstacles<TermsSurface>& tm, int P, int n) {
  return tm.K >= 1 && tm.K <= kMaxObstacles && tm.obs != nullptr && tm.radii != nullptr && tm.P == P && tm.n == n;
}

template <typename Launch>
hipError_t with_obstacle_pack(WithObstacles<TermsSurface> tm, const float* coef, Launch&& launch) {
  tm.coef = coef;
  if (has_downforce(tm)) return launch(obstacles_over<TermsAero>(tm));
  if (has_load_transfer(tm)) return launch(obstacles_over<TermsLoaded>(tm));
  if (has_coupling(tm)) return launch(obstacles_over<TermsCoupled>(tm));
  return launch(obstacles_over<TermsObjective>(tm));
}

hipError_t launch_rollout_dynamic_obstacles(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                            const Integration& g, const WithObstacles<TermsSurface>& tm, hipStream_t s) {
  if (!obstacles_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  if (has_surface(tm)) return launch_rollout_dynamic_surface(layout, args, vehicles, g, tm, s);
  return with_obstacle_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

hipError_t launch_rollout_dynamic_sampled_obstacles(const RolloutArgs& args, const SampleArgs& sample,
                                                    const VehicleEnsemble& vehicles, const Integration& g,
                                                    const WithObstacles<TermsSurface>& tm, hipStream_t s) {
  if (!obstacles_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  if (has_surface(tm)) return launch_rollout_dynamic_sampled_surface(args, sample, vehicles, g, tm, s);
  return with_obstacle_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, pack); });
}

hipError_t launch_finalize_dynamic_obstacles(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                             const Integration& g, const WithObstacles<TermsSurface>& tm, hipStream_t s) {
  if (!obstacles_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  if (has_surface(tm)) return launch_finalize_dynamic_surface(layout, args, vehicles, g, tm, s);
  return with_obstacle_pack(tm, args.coef, [&](const auto& pack) { return finalize_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

}  // namespace acmpc
