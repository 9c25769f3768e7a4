// Translation unit of mode D's kernels with the tyre coupling (acmpc_set_dynamics_coupling): the kernel templates of
// acmpc_dynamic.hip instantiated with the TermsCoupled argument - the general step with the friction-ellipse block in every
// sub-step, and the four term parts behind their switches - and their launchers.  Apart from acmpc_dynamic.hip and
// acmpc_dynamic_terms.hip so that the code objects of the kernels without the coupling are not touched by them.
#define ACMPC_DYNAMIC_COUPLED_TU 1
#include "acmpc_dynamic.hip"
