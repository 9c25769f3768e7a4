// Mode D's kernels with the downforce (acmpc_set_dynamics_downforce): the templates of acmpc_dynamic_kernels.h with a TermsAero -
// the loaded step on the peaks at the sub-step's speed (c_h = w_max = 0 while the load transfer is off, the ratios +inf while
// the coupling is off) and the four term parts.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

hipError_t launch_rollout_dynamic_aero(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                       const Integration& g, const TermsAero& tm, hipStream_t s) {
  return rollout_dynamic_launch(layout, args, vehicles, g, s, tm);
}

hipError_t launch_rollout_dynamic_sampled_aero(const RolloutArgs& args, const SampleArgs& sample,
                                               const VehicleEnsemble& vehicles, const Integration& g,
                                               const TermsAero& tm, hipStream_t s) {
  return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, tm);
}

hipError_t launch_finalize_dynamic_aero(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                        const Integration& g, const TermsAero& tm, hipStream_t s) {
  return finalize_dynamic_launch(layout, args, vehicles, g, s, tm);
}

}  // namespace acmpc
