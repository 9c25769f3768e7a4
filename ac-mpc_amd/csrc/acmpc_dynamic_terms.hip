// Mode D's kernels with the rate and slip terms (acmpc_set_dynamics_terms) and with the objective as well
// (acmpc_set_dynamics_objective): the templates of acmpc_dynamic_kernels.h with a Terms and with a TermsObjective.
#include "acmpc_dynamic_kernels.h"

namespace acmpc {

// (a handle without the objective runs the kernels of a plain Terms)
hipError_t launch_rollout_dynamic_terms(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                        const Integration& g, const TermsObjective& tm, hipStream_t s) {
  if (has_objective(tm)) return rollout_dynamic_launch(layout, args, vehicles, g, s, tm);
  return rollout_dynamic_launch(layout, args, vehicles, g, s, static_cast<const Terms&>(tm));
}

hipError_t launch_rollout_dynamic_sampled_terms(const RolloutArgs& args, const SampleArgs& sample,
                                                const VehicleEnsemble& vehicles, const Integration& g,
                                                const TermsObjective& tm, hipStream_t s) {
  if (has_objective(tm)) return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, tm);
  return rollout_dynamic_sampled_launch(args, sample, vehicles, g, s, static_cast<const Terms&>(tm));
}

hipError_t launch_finalize_dynamic_terms(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                         const Integration& g, const TermsObjective& tm, hipStream_t s) {
  if (has_objective(tm)) return finalize_dynamic_launch(layout, args, vehicles, g, s, tm);
  return finalize_dynamic_launch(layout, args, vehicles, g, s, static_cast<const Terms&>(tm));
}

}  // namespace acmpc
