// Translation unit of mode D's kernels with moving obstacles (acmpc_set_obstacles, acmpc_set_dynamics_clearance): the kernel
// templates of acmpc_dynamic.hip instantiated with a WithObstacles argument over TermsObjective, TermsCoupled and TermsLoaded -
// the step the handle would take without obstacles, the four term parts behind their switches, and the discs' lines after
// them - and their launchers.  Apart from the other four units so that the code objects of the kernels without obstacles are
// not touched by them.
#define ACMPC_DYNAMIC_OBSTACLES_TU 1
#include "acmpc_dynamic.hip"
