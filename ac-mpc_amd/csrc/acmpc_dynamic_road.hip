// Mode D's kernels with a road table (acmpc_set_road): the templates of acmpc_dynamic_kernels.h with a TermsRoad - the surface
// step with each lane's peaks scaled by n_z as well and gravity's a_x, a_y of the waypoint the candidate was at one control step
// before added to xd3, xd4 in every sub-step - and, while obstacles are set, with a WithObstacles<TermsRoad>.  With the actuator
// lag on, the unit beside this one holds the kernels (acmpc_dynamic_road_actuator.hip: the two build in parallel).
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

namespace {

using HandleTerms = WithActuator<WithObstacles<TermsRoad>>;

template <typename Launch>
hipError_t with_road_pack(const HandleTerms& tm, const float* coef, Launch&& launch) {
  if (!has_obstacles(tm)) return launch(static_cast<const TermsRoad&>(tm));
  WithObstacles<TermsRoad> pack = tm;
  pack.coef = coef;
  return launch(pack);
}

}  // namespace

hipError_t launch_rollout_dynamic_road(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                       const Integration& g, const HandleTerms& tm, hipStream_t s) {
  if (!road_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  if (has_actuator(tm)) return launch_rollout_dynamic_road_actuator(layout, args, vehicles, g, tm, s);
  return with_road_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

hipError_t launch_rollout_dynamic_sampled_road(const RolloutArgs& args, const SampleArgs& sample,
                                               const VehicleEnsemble& vehicles, const Integration& g,
                                               const HandleTerms& tm, hipStream_t s) {
  if (!road_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  if (has_actuator(tm)) return launch_rollout_dynamic_sampled_road_actuator(args, sample, vehicles, g, tm, s);
  return with_road_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, pack); });
}

hipError_t launch_finalize_dynamic_road(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                        const Integration& g, const HandleTerms& tm, hipStream_t s) {
  if (!road_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  if (has_actuator(tm)) return launch_finalize_dynamic_road_actuator(layout, args, vehicles, g, tm, s);
  return with_road_pack(tm, args.coef, [&](const auto& pack) { return finalize_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

}  // namespace acmpc
