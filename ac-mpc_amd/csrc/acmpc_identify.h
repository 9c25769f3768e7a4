// Mode D's grip identification (acmpc_score_grips): the launcher of acmpc_identify.hip and its limits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "acmpc_dynamic.h"

namespace acmpc {

constexpr int kIdentifyMaxSteps = 512;            // ACMPC_MAX_LOG_STEPS
constexpr int kIdentifyMaxHypotheses = 65536;     // ACMPC_MAX_GRIP_HYPOTHESES
constexpr int64_t kIdentifyMaxValues = int64_t{1} << 22;   // S K: the per-segment values e [S][K]

// Everything on the device.  states [W + 1][3] = (vx, vy, r), controls [W][2] = (delta, pedal), peaks [K][2] = the
// hypotheses' (Pf, Pr) (8-byte aligned), w = the residual's weights; e [S][K] scratch, S = identify_segments(W, L);
// errors [K], partial_keys [identify_blocks(K)] and best [1] are written.
struct IdentifyArgs {
  const float* states;
  const float* controls;
  const float* peaks;
  float* e;
  float* errors;
  int64_t* partial_keys;
  int64_t* best;
  int W, L, K;
  float w[3];
};

int identify_segments(int W, int L);   // ceil(W / L)
int identify_blocks(int K);            // workgroups (= partial keys) of K hypotheses: <= 256
// the grid of identify_grip_kernel over S segments of K hypotheses: `blocks` x `grid_y` workgroups, workgroup (x, y) rolling
// segments [y run, min((y + 1) run, S)) - `rows` is the number of runs aimed at.  launch_identify_grip launches what this
// returns and acmpc_describe_score_grips reports it.
struct IdentifyGrid {
  int blocks, rows, run, grid_y;
};
IdentifyGrid identify_grid(int S, int K);
// `vehicle`: the base vehicle (its Pf, Pr are not read); `g`: the integration setting with h of the LOG's period and
// inv_L[0] the base vehicle's; `coupling`: the two ratios of the handle's tyre coupling, or nullptr while it is off.  hipErrorInvalidValue
// beyond the limits above.
// `load`: the six scalars of the handle's load transfer for the base vehicle (acmpc_dynamic.h: LoadedPeaks), or nullptr while
// it is off.
struct IdentifyLoad {
  float c_h, w_max, a1_f, a2_f, a1_r, a2_r;
};
// `aero`: the handle's downforce (acmpc_dynamic.h: AeroPeaks), or nullptr while it is off; with it `load` holds the base
// vehicle's a1, a2 (and c_h = w_max = 0 while the load transfer is off).
struct IdentifyAero {
  float k_f, k_r, v_sat;
};
hipError_t launch_identify_grip(const IdentifyArgs& args, const Vehicle& vehicle, const Integration& g, const float* coupling,
                                const IdentifyLoad* load, const IdentifyAero* aero, hipStream_t s);

}  // namespace acmpc
