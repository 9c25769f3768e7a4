// Mode D's kernels with a road table (acmpc_set_road) and the actuator lag (acmpc_set_dynamics_actuator): the templates of
// acmpc_dynamic_kernels.h with a WithActuator over TermsRoad, and over WithObstacles<TermsRoad> while obstacles are set.  The
// step is the road's, driven on the lagged control; the terms stay on the command.  acmpc_dynamic_road.hip hands over to these.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

namespace {

using HandleTerms = WithActuator<WithObstacles<TermsRoad>>;

template <typename Launch>
hipError_t with_road_actuator_pack(const HandleTerms& tm, const float* coef, Launch&& launch) {
  if (has_obstacles(tm)) return launch(actuator_over_obstacles<TermsRoad>(tm, coef));
  return launch(actuator_over<TermsRoad>(tm));
}

}  // namespace

hipError_t launch_rollout_dynamic_road_actuator(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                                const Integration& g, const HandleTerms& tm, hipStream_t s) {
  if (!has_actuator(tm) || !road_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_road_actuator_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

hipError_t launch_rollout_dynamic_sampled_road_actuator(const RolloutArgs& args, const SampleArgs& sample,
                                                        const VehicleEnsemble& vehicles, const Integration& g,
                                                        const HandleTerms& tm, hipStream_t s) {
  if (!has_actuator(tm) || !road_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_road_actuator_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, pack); });
}

hipError_t launch_finalize_dynamic_road_actuator(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                                 const Integration& g, const HandleTerms& tm, hipStream_t s) {
  if (!has_actuator(tm) || !road_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_road_actuator_pack(tm, args.coef, [&](const auto& pack) { return finalize_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

}  // namespace acmpc
