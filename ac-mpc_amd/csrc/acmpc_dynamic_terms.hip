// Translation unit of mode D's kernels with the rate and slip terms (acmpc_set_dynamics_terms): the kernel templates of
// acmpc_dynamic.hip instantiated with the Terms argument - and, for a handle with the objective as well
// (acmpc_set_dynamics_objective), with the TermsObjective argument - and their launchers.  Apart from acmpc_dynamic.hip so that the
// code object of the kernels without the terms is not touched by them.
#define ACMPC_DYNAMIC_TERMS_TU 1
#include "acmpc_dynamic.hip"
