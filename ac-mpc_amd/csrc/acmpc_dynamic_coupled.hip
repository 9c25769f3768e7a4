// Mode D's kernels with the tyre coupling (acmpc_set_dynamics_coupling): the templates of acmpc_dynamic_kernels.h with a
// TermsCoupled - the general step with the friction-ellipse block in every sub-step, the four term parts behind their switches.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

hipError_t launch_rollout_dynamic_coupled(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                          const Integration& g, const TermsCoupled& tm, hipStream_t s) {
  return rollout_dynamic_launch(layout, args, vehicles, g, s, tm);
}

hipError_t launch_rollout_dynamic_sampled_coupled(const RolloutArgs& args, const SampleArgs& sample,
                                                  const VehicleEnsemble& vehicles, const Integration& g,
                                                  const TermsCoupled& tm, hipStream_t s) {
  return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, tm);
}

hipError_t launch_finalize_dynamic_coupled(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                           const Integration& g, const TermsCoupled& tm, hipStream_t s) {
  return finalize_dynamic_launch(layout, args, vehicles, g, s, tm);
}

}  // namespace acmpc
