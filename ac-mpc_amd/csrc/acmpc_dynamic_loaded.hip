// Translation unit of mode D's kernels with the load transfer (acmpc_set_dynamics_load_transfer): the kernel templates of
// acmpc_dynamic.hip instantiated with the TermsLoaded argument - the general step with the loaded peaks and the
// friction-ellipse block in every sub-step (the ratios +inf while the coupling is off), and the four term parts behind their
// switches - and their launchers.  Apart from acmpc_dynamic.hip, acmpc_dynamic_terms.hip and acmpc_dynamic_coupled.hip so that
// the code objects of the kernels without the load transfer are not touched by them.
#define ACMPC_DYNAMIC_LOADED_TU 1
#include "acmpc_dynamic.hip"
