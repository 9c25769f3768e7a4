// Mode D's kernels with the actuator lag (acmpc_set_dynamics_actuator): the templates of acmpc_dynamic_kernels.h with a
// WithActuator over the packs of the top-tier step - TermsAero, or TermsSurface while a surface table is set, each under the
// obstacles' pack while obstacles are set.  The step is that pack's, driven on the lagged control; the terms stay on the command.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

namespace {

using HandleTerms = WithActuator<WithObstacles<TermsSurface>>;

// nothing is launched unless the actuator positions (if any), the surface table (if any) and the obstacle data (if any) are
// what this launch's P and n index
bool actuator_valid(const HandleTerms& tm, int P, int n) {
  if (!has_actuator(tm) || (tm.lag.a0 != nullptr && tm.lag.a0_P != P)) return false;
  if (has_surface(tm) && (tm.mu == nullptr || tm.mu_P != P || tm.mu_n != n)) return false;
  if (!has_obstacles(tm)) return true;
  return tm.K >= 1 && tm.K <= kMaxObstacles && tm.obs != nullptr && tm.radii != nullptr && tm.P == P && tm.n == n;
}

template <typename Launch>
hipError_t with_actuator_pack(const HandleTerms& tm, const float* coef, Launch&& launch) {
  if (has_obstacles(tm) && has_surface(tm)) return launch(actuator_over_obstacles<TermsSurface>(tm, coef));
  if (has_obstacles(tm)) return launch(actuator_over_obstacles<TermsAero>(tm, coef));
  if (has_surface(tm)) return launch(actuator_over<TermsSurface>(tm));
  return launch(actuator_over<TermsAero>(tm));
}

}  // namespace

hipError_t launch_rollout_dynamic_actuator(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                           const Integration& g, const HandleTerms& tm, hipStream_t s) {
  if (!actuator_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_actuator_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

hipError_t launch_rollout_dynamic_sampled_actuator(const RolloutArgs& args, const SampleArgs& sample,
                                                   const VehicleEnsemble& vehicles, const Integration& g,
                                                   const HandleTerms& tm, hipStream_t s) {
  if (!actuator_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_actuator_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, pack); });
}

hipError_t launch_finalize_dynamic_actuator(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                            const Integration& g, const HandleTerms& tm, hipStream_t s) {
  if (!actuator_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_actuator_pack(tm, args.coef, [&](const auto& pack) { return finalize_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

}  // namespace acmpc
