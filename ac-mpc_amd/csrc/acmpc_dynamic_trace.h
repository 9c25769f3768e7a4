// Mode D's plan trace (acmpc_trace_plans, DESIGN.md section 2 "Mode D, plan trace"): given controls are re-rolled under
// every vehicle of the handle with all of its settings, as the scoring kernels roll them, and every control step leaves its
// six states and what its cost lines saw.  The kernel and its launcher are acmpc_dynamic_trace.hip's.
#pragma once
#include "acmpc_dynamic.h"

namespace acmpc {

constexpr int kTraceTermFloats = 22;   // ACMPC_TRACE_TERM_FLOATS
// one row of `terms` per control step, on the state that step's dynamic_cost saw
constexpr int kTraceNearest = 0;       // the nearest waypoint j, as a float (exact: n <= kDynamicMaxSteps)
constexpr int kTraceEy = 1, kTraceEpsi = 2, kTraceDv = 3, kTraceDk = 4;
constexpr int kTraceBox = 5;           // 5, 6: u - med3(u, lo, hi) of steering and pedal
constexpr int kTraceCorridor = 7;
constexpr int kTraceRate = 8;          // 8, 9: dynamic_terms' hd, hp
constexpr int kTraceSlip = 10, kTraceCeiling = 11;
constexpr int kTraceDiscs = 12;        // 12 .. 19: disc q's penetration depth, +0 beyond K_obs
constexpr int kTraceV = 20, kTraceE = 21;   // the running sums after this step

struct TraceArgs {
  const float* U;      // [P][M][n][2] (delta, pedal)
  const float* x0;     // [P][6]
  const float* coef;   // [P][n][kCoefT] packed rows
  float* states;       // [P][M][K][n + 1][6], or nullptr
  float* totals;       // [P][M][K][2] = (c_k, V_k), or nullptr
  float* terms;        // [P][M][K][n][kTraceTermFloats], or nullptr
  int P, M, n;
  Weights w;
};

// One wavefront per (problem, plan, vehicle): grid (P M, K).  The instantiation is picked as launch_finalize_dynamic picks
// its own - the actuator lag first, then obstacles, then downforce, load transfer, coupling, terms / objective, the integration, the default - so
// that a trace is the arithmetic of the kernels that scored the plan.
hipError_t launch_trace_dynamic(const TraceArgs& args, const VehicleEnsemble& vehicles, const Integration& integration,
                                const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);

}  // namespace acmpc
