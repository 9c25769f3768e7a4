// Mode D's kernels with a surface table (acmpc_set_surface): the templates of acmpc_dynamic_kernels.h with a TermsSurface - the
// aero step on each lane's own peaks, the vehicle's scaled by (mu_f, mu_r) of the waypoint the candidate was at one control step
// before - and, while obstacles are set, with a WithObstacles<TermsSurface>: the same with the discs' lines after the terms.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

namespace {

// nothing is launched unless the table is what this launch's P and n index (0 <= j < n is all the kernels rely on)
bool surface_valid(const WithObstacles<TermsSurface>& tm, int P, int n) {
  if (!has_surface(tm) || tm.mu == nullptr || tm.mu_P != P || tm.mu_n != n) return false;
  if (!has_obstacles(tm)) return true;
  return tm.K >= 1 && tm.K <= kMaxObstacles && tm.obs != nullptr && tm.radii != nullptr && tm.P == P && tm.n == n;
}

template <typename Launch>
hipError_t with_surface_pack(WithObstacles<TermsSurface> tm, const float* coef, Launch&& launch) {
  if (!has_obstacles(tm)) return launch(static_cast<const TermsSurface&>(tm));
  tm.coef = coef;
  return launch(tm);
}

}  // namespace

hipError_t launch_rollout_dynamic_surface(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                          const Integration& g, const WithObstacles<TermsSurface>& tm, hipStream_t s) {
  if (!surface_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_surface_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

hipError_t launch_rollout_dynamic_sampled_surface(const RolloutArgs& args, const SampleArgs& sample,
                                                  const VehicleEnsemble& vehicles, const Integration& g,
                                                  const WithObstacles<TermsSurface>& tm, hipStream_t s) {
  if (!surface_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_surface_pack(tm, args.coef, [&](const auto& pack) { return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, pack); });
}

hipError_t launch_finalize_dynamic_surface(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                           const Integration& g, const WithObstacles<TermsSurface>& tm, hipStream_t s) {
  if (!surface_valid(tm, args.P, args.n)) return hipErrorInvalidValue;
  return with_surface_pack(tm, args.coef, [&](const auto& pack) { return finalize_dynamic_launch(layout, args, vehicles, g, s, pack); });
}

}  // namespace acmpc
