// Mode D's kernels with the load transfer (acmpc_set_dynamics_load_transfer): the templates of acmpc_dynamic_kernels.h with a
// TermsLoaded - the coupled step on the loaded peaks (the ratios +inf while the coupling is off) and the four term parts.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

hipError_t launch_rollout_dynamic_loaded(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                         const Integration& g, const TermsLoaded& tm, hipStream_t s) {
  return rollout_dynamic_launch(layout, args, vehicles, g, s, tm);
}

hipError_t launch_rollout_dynamic_sampled_loaded(const RolloutArgs& args, const SampleArgs& sample,
                                                 const VehicleEnsemble& vehicles, const Integration& g,
                                                 const TermsLoaded& tm, hipStream_t s) {
  return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, tm);
}

hipError_t launch_finalize_dynamic_loaded(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                          const Integration& g, const TermsLoaded& tm, hipStream_t s) {
  return finalize_dynamic_launch(layout, args, vehicles, g, s, tm);
}

}  // namespace acmpc
