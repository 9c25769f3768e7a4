// Mode D's plan trace (acmpc_dynamic_trace.h): trace_dynamic_kernel and its launcher.  A latency kernel modelled on
// finalize_dynamic_kernel (acmpc_dynamic_kernels.h): one wavefront per (problem, plan, vehicle), the waypoint rows and the
// search keys staged in LDS, the plan's controls staged beside them and broadcast, every lane rolling the same state, the
// nearest-waypoint search spread over the lanes, lane 0 writing.  The step, the cost and the terms are the shared functions of
// acmpc_dynamic.h called as the finalize calls them; what the kernel adds is the hinges of every step RESTATED for output
// (trace_hinges and the three lines of dynamic_cost below).  Replaying V = fma(h, h, V) over a step's hinges from the previous
// step's V gives this step's V bit for bit (tests/test_gpu_dynamic_trace.py): that is what keeps the restatements from drifting
// away from the functions that score.
#include "acmpc_dynamic_trace.h"

#include "acmpc_dynamic_kernels.h"

namespace acmpc {

namespace {

constexpr int kTraceHinges = 4 + kMaxObstacles;   // slots 8 .. 19: rate (2), slip, ceiling, the discs
static_assert(kTraceRate + kTraceHinges == kTraceV, "the hinges of the terms fill slots 8 .. 19");

// The hinges dynamic_terms is about to square into V, in its order: h[0], h[1] the rates', h[2] the slip's, h[3] the ceiling's.
// Called BEFORE dynamic_terms (ts still holds the previous step's control) on the state it will see.  A part that is off
// leaves its +0.
template <typename TT>
__device__ __forceinline__ void trace_hinges(const StateD& s, float delta, float pedal, int i, [[maybe_unused]] int p,
                                             const Vehicle& k, [[maybe_unused]] const float* wp, [[maybe_unused]] int j,
                                             const TermsState<float>& ts, float (&h)[kTraceHinges], const TT& t) {
  if (t.rate != 0) {
    const bool own = i == 0 && t.u_prev == nullptr;
    const float pd = own ? delta : ts.pd;
    const float pp = own ? pedal : ts.pp;
    const float rd = (delta - pd) * t.inv_dt;
    const float rp = (pedal - pp) * t.inv_dt;
    h[0] = vmax(abs_(rd) - t.rd_max, 0.0f);
    h[1] = vmax(abs_(rp) - t.rp_max, 0.0f);
  }
  if (t.slip != 0) {
    const float b = (s.r * k.lr - s.vy) / (s.vx + kVxEps);
    h[2] = vmax(abs_(b) - t.b_max, 0.0f);
  }
  if constexpr (std::is_base_of<TermsObjective, TT>::value) {
    if (t.ceiling != 0) {
      const float cap = fma_(t.cs, wp[j * kCoefT + 5], t.co);
      h[3] = vmax(s.vx - cap, 0.0f);
    }
  }
}

// The same under the obstacles' pack: the base pack's hinges, then disc q's depth in h[4 + q] (plain loads: problem, step and
// disc are uniform)
template <typename Base>
__device__ __forceinline__ void trace_hinges(const StateD& s, float delta, float pedal, int i, int p, const Vehicle& k,
                                             const float* wp, int j, const TermsState<float>& ts, float (&h)[kTraceHinges],
                                             const WithObstacles<Base>& t) {
  trace_hinges<Base>(s, delta, pedal, i, p, k, wp, j, ts, h, static_cast<const Base&>(t));
  const float* __restrict__ coef = t.coef + static_cast<size_t>(p) * t.n * kCoefT;
  const float* __restrict__ row = t.obs + (static_cast<size_t>(p) * t.n + i) * t.K * 2;
#pragma unroll
  for (int q = 0; q < kMaxObstacles; ++q) {
    if (q < t.K) {
      const float ox = row[2 * q] - coef[0], oy = row[2 * q + 1] - coef[1];
      const float R = t.radii[static_cast<size_t>(p) * t.K + q];
      const float dx = s.t.X - ox, dy = s.t.Y - oy;
      const float d = sqrt_(fma_(dy, dy, dx * dx));
      h[4 + q] = vmax(R - d, 0.0f);
    }
  }
}

// Under the actuator's pack: the base pack's hinges, on the command
template <typename Base>
__device__ __forceinline__ void trace_hinges(const StateD& s, float delta, float pedal, int i, int p, const Vehicle& k,
                                             const float* wp, int j, const TermsState<float>& ts, float (&h)[kTraceHinges],
                                             const WithActuator<Base>& t) {
  trace_hinges(s, delta, pedal, i, p, k, wp, j, ts, h, static_cast<const Base&>(t));
}

template <bool FINE, typename... TM>
__global__ void __launch_bounds__(kWave)
    trace_dynamic_kernel(const TraceArgs a, const VehicleEnsemble e, const Integration g, const TM... tm) {
  extern __shared__ __attribute__((aligned(16))) float s_u[];   // the plan's controls, then the waypoint rows and keys
  const int n = a.n;
  const int p = static_cast<int>(blockIdx.x) / a.M;
  const int m = static_cast<int>(blockIdx.x) - p * a.M;
  const int k = static_cast<int>(blockIdx.y);   // this wave's vehicle: uniform, its constants are scalars
  const int K = static_cast<int>(gridDim.y);
  const int lane = static_cast<int>(threadIdx.x);
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefT;
  const float* __restrict__ x0 = a.x0 + static_cast<size_t>(p) * kDynamicStateFloats;
  const float* __restrict__ U = a.U + (static_cast<size_t>(p) * a.M + m) * n * 2;
  const size_t slot = (static_cast<size_t>(p) * a.M + m) * K + k;
  float* __restrict__ states = a.states != nullptr ? a.states + slot * (n + 1) * kDynamicStateFloats : nullptr;
  float* __restrict__ terms = a.terms != nullptr ? a.terms + slot * n * kTraceTermFloats : nullptr;
  float* s_wp = s_u + ((2 * n + 3) & ~3);
  float* s_abc = s_wp + n * kCoefT;
  stage_dynamic_tables(coef, n, lane, kWave, e.v[0].wheelbase, s_wp, s_abc);
  for (int q = lane; q < 2 * n; q += kWave) s_u[q] = U[q];
  const Vehicle veh = e.v[k];
  StateD st = start_dynamic<float>(x0, coef);
  constexpr bool kTerms = sizeof...(TM) != 0;
  [[maybe_unused]] TermsState<float> ts;
  if constexpr (kTerms) ts = start_terms<float>(p, tm...);
  else ts = TermsState<float>{0.0f, 0.0f, 0.0f, 0};
  [[maybe_unused]] ActuatorState<float> as;   // (the actuator lag: the two positions, a0[p] or step 0's command)
  if constexpr (kActuatorPack<TM...>) as = start_actuator<float>(p, lag_of(tm...));
  if (lane == 0 && states != nullptr) {
    states[0] = st.t.X + coef[0];   // (poses leave in the caller's frame: start_temporal())
    states[1] = st.t.Y + coef[1];
    states[2] = st.t.phi;
    states[3] = st.vx;
    states[4] = st.vy;
    states[5] = st.r;
  }
  __syncthreads();
  const bool exhaustive = w.nn_ahead < 0;
  const int win_w = w.nn_back + w.nn_ahead + 1;
  int j_prev = 0;
  for (int i = 0; i < n; ++i) {
    [[maybe_unused]] RoadRow<float> rr;   // (the road table: the row of the last step's waypoint, loaded like the scales)
    if constexpr (kRoadPack<TM...>) rr = road_row<float>(p, n, j_prev, tm...);
    [[maybe_unused]] SurfaceScales<float> ms;   // (the surface table: j_prev is uniform, a scalar load)
    if constexpr (kSurfacePack<TM...>) ms = surface_scales<float>(p, n, j_prev, tm...);
    const float d = s_u[2 * i], q = s_u[2 * i + 1];   // (LDS broadcast: every lane rolls the same state)
    float dx = d, qx = q;   // (what the step is driven on: the command, or what the actuator lag makes of it)
    if constexpr (kActuatorPack<TM...>) actuator_step<float>(i, d, q, as, lag_of(tm...), dx, qx);
    if constexpr (kRoadPack<TM...>) dynamic_advance_fine<float, RoadPeaks<float>>(st, dx, qx, veh, g, g.inv_L[k], road_peaks<float>(aero_peaks(k, tm...), veh, rr));
    else if constexpr (kSurfacePack<TM...>) dynamic_advance_fine<float, AeroPeaks<SurfacePeaks<float>>>(st, dx, qx, veh, g, g.inv_L[k], surface_peaks<float>(aero_peaks(k, tm...), veh, ms));
    else if constexpr (kAeroPack<TM...>) dynamic_advance_fine<float, AeroPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], aero_peaks(k, tm...));
    else if constexpr (kLoadedPack<TM...>) dynamic_advance_fine<float, LoadedPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], loaded_peaks(k, tm...));
    else if constexpr (kCoupledPack<TM...>) dynamic_advance_fine<float, CoupledPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], coupled_peaks(tm...));
    else dynamic_control_step<FINE, float>(st, dx, qx, veh, w.dt, g, g.inv_L[k]);
    // finalize_dynamic_kernel's search: the first minimum of the key over the search's waypoints, the lanes side by side;
    // ties -> the lower index, and the search's first waypoint when no key compares below +inf
    const int lo = exhaustive ? 0 : max(min(j_prev - w.nn_back, n - win_w), 0);
    const int hi = exhaustive ? n - 1 : min(lo + win_w, n) - 1;
    float best = __builtin_inff();
    int j = 0x7fffffff;
    for (int c = lo + lane; c <= hi; c += kWave) {
      const float key = search_key<float>(st.t.X, st.t.Y, s_abc[kKeyStride * c], s_abc[kKeyStride * c + kKeyB],
                                          s_abc[kKeyStride * c + kKeyC]);
      if (key < best) {
        best = key;
        j = c;
      }
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
      const float ob = __shfl_xor(best, mask, kWave);
      const int oj = __shfl_xor(j, mask, kWave);
      const bool take = (ob < best) || (ob == best && oj < j);
      best = take ? ob : best;
      j = take ? oj : j;
    }
    j = __builtin_amdgcn_readfirstlane(j);
    j = (j == 0x7fffffff) ? lo : j;
    j_prev = j;
    dynamic_settle(st, s_wp, j, d, q, w);
    float h[kTraceHinges];
#pragma unroll
    for (int c = 0; c < kTraceHinges; ++c) h[c] = 0.0f;
    if constexpr (kTerms) {
      trace_hinges(st, d, q, i, p, veh, s_wp, j, ts, h, tm...);
      dynamic_terms<float>(st, d, q, i, p, veh, s_wp, j, ts, tm...);
    }
    if (lane == 0) {
      if (states != nullptr) {
        float* __restrict__ x = states + static_cast<size_t>(i + 1) * kDynamicStateFloats;
        x[0] = st.t.X + coef[0];
        x[1] = st.t.Y + coef[1];
        x[2] = st.t.phi;
        x[3] = st.vx;
        x[4] = st.vy;
        x[5] = st.r;
      }
      if (terms != nullptr) {
        // dynamic_cost's operands and its three hinges again, on the row it read
        float row[kCoefT];
        load_row(s_wp, j, row);
        float* __restrict__ t = terms + static_cast<size_t>(i) * kTraceTermFloats;
        t[kTraceNearest] = static_cast<float>(j);
        t[kTraceEy] = st.t.ey;
        t[kTraceEpsi] = st.t.ep;
        t[kTraceDv] = st.vx - row[5];
        t[kTraceDk] = d - row[7];
        t[kTraceBox] = d - med3_(d, w.ulo0, w.uhi0);
        t[kTraceBox + 1] = q - med3_(q, w.ulo1, w.uhi1);
        t[kTraceCorridor] = vmax(abs_(st.t.ey) - row[6], 0.0f);
#pragma unroll
        for (int c = 0; c < kTraceHinges; ++c) t[kTraceRate + c] = h[c];
        t[kTraceV] = st.t.V;
        t[kTraceE] = ts.E;
      }
    }
  }
  if (lane == 0 && a.totals != nullptr) {
    float cost;
    if constexpr (kTerms) cost = finish_dynamic_terms<float>(st, ts, s_wp, j_prev, p, n, w, tm...);
    else cost = finish_temporal<float>(st.t, n, w);
    a.totals[2 * slot] = cost;
    a.totals[2 * slot + 1] = st.t.V;
  }
}

template <typename... TM>
hipError_t trace_dynamic_launch(const TraceArgs& args, const VehicleEnsemble& vehicles, const Integration& g, hipStream_t s,
                                const TM&... tm) {
  constexpr bool kGeneral = sizeof...(TM) != 0;
  const size_t lds = (((2 * static_cast<size_t>(args.n) + 3) & ~static_cast<size_t>(3)) +
                      static_cast<size_t>(args.n) * (kCoefT + kKeyStride)) * sizeof(float);   // n = 512: 36 KB
  const dim3 grid(static_cast<unsigned>(args.P) * static_cast<unsigned>(args.M), vehicles.K);
  return with_integration_kind<kGeneral>(g, [&](auto fine) {
    constexpr bool kFine = decltype(fine)::value;
    return launch_kernel(trace_dynamic_kernel<kFine, TM...>, grid, dim3(kWave), lds, s, nullptr, nullptr, args, vehicles, g,
                         tm...);
  });
}

}  // namespace

hipError_t launch_trace_dynamic(const TraceArgs& args, const VehicleEnsemble& vehicles, const Integration& g,
                                const WithActuator<WithObstacles<TermsRoad>>& road, hipStream_t s) {
  clear_stale_error();
  if (!integration_valid(g)) return hipErrorInvalidValue;
  if (args.n < 1 || args.n > kDynamicMaxSteps || args.M < 1 || args.P < 1) return hipErrorInvalidValue;
  if (static_cast<int64_t>(args.P) * args.M > 0x7fffffff) return hipErrorInvalidValue;
  if (vehicles.K < 1 || vehicles.K > kMaxVehicles) return hipErrorInvalidValue;
  if (args.U == nullptr || args.x0 == nullptr || args.coef == nullptr) return hipErrorInvalidValue;
  if (has_road(road)) {
    // (nothing is launched unless every table the handle has set is what this launch's P and n index): the road step, with or
    // without the obstacles' lines and the actuator lag
    if (!road_valid(road, args.P, args.n)) return hipErrorInvalidValue;
    if (has_actuator(road) && has_obstacles(road)) return trace_dynamic_launch(args, vehicles, g, s, actuator_over_obstacles<TermsRoad>(road, args.coef));
    if (has_actuator(road)) return trace_dynamic_launch(args, vehicles, g, s, actuator_over<TermsRoad>(road));
    if (has_obstacles(road)) {
      WithObstacles<TermsRoad> both = road;
      both.coef = args.coef;
      return trace_dynamic_launch(args, vehicles, g, s, both);
    }
    return trace_dynamic_launch(args, vehicles, g, s, static_cast<const TermsRoad&>(road));
  }
  const WithActuator<WithObstacles<TermsSurface>> tm = below_road(road);
  // (nothing is launched unless the surface table is what this launch's P and n index)
  if (has_surface(tm) && (tm.mu == nullptr || tm.mu_P != args.P || tm.mu_n != args.n)) return hipErrorInvalidValue;
  if (has_obstacles(tm) && (tm.K > kMaxObstacles || tm.obs == nullptr || tm.radii == nullptr || tm.P != args.P || tm.n != args.n))
    return hipErrorInvalidValue;   // (nor unless the obstacle data is)
  if (has_actuator(tm)) {
    // (nor unless the actuator positions, if any are set, are this launch's P): the aero or the surface step, the tiers that
    // are off at their neutral values (the handle fills them in), with or without the obstacles' lines
    if (tm.lag.a0 != nullptr && tm.lag.a0_P != args.P) return hipErrorInvalidValue;
    if (has_obstacles(tm) && has_surface(tm)) return trace_dynamic_launch(args, vehicles, g, s, actuator_over_obstacles<TermsSurface>(tm, args.coef));
    if (has_obstacles(tm)) return trace_dynamic_launch(args, vehicles, g, s, actuator_over_obstacles<TermsAero>(tm, args.coef));
    if (has_surface(tm)) return trace_dynamic_launch(args, vehicles, g, s, actuator_over<TermsSurface>(tm));
    return trace_dynamic_launch(args, vehicles, g, s, actuator_over<TermsAero>(tm));
  }
  if (has_obstacles(tm)) {
    if (has_surface(tm)) {
      WithObstacles<TermsSurface> both = tm;
      both.coef = args.coef;
      return trace_dynamic_launch(args, vehicles, g, s, both);
    }
    WithObstacles<TermsAero> pack = obstacles_over<TermsAero>(tm);
    pack.coef = args.coef;
    if (has_downforce(pack)) return trace_dynamic_launch(args, vehicles, g, s, pack);
    if (has_load_transfer(pack)) return trace_dynamic_launch(args, vehicles, g, s, obstacles_over<TermsLoaded>(pack));
    if (has_coupling(pack)) return trace_dynamic_launch(args, vehicles, g, s, obstacles_over<TermsCoupled>(pack));
    return trace_dynamic_launch(args, vehicles, g, s, obstacles_over<TermsObjective>(pack));
  }
  if (has_surface(tm)) return trace_dynamic_launch(args, vehicles, g, s, static_cast<const TermsSurface&>(tm));
  if (has_downforce(tm)) return trace_dynamic_launch(args, vehicles, g, s, static_cast<const TermsAero&>(tm));
  if (has_load_transfer(tm)) return trace_dynamic_launch(args, vehicles, g, s, static_cast<const TermsLoaded&>(tm));
  if (has_coupling(tm)) return trace_dynamic_launch(args, vehicles, g, s, static_cast<const TermsCoupled&>(tm));
  if (has_objective(tm)) return trace_dynamic_launch(args, vehicles, g, s, static_cast<const TermsObjective&>(tm));
  if (has_terms(tm)) return trace_dynamic_launch(args, vehicles, g, s, static_cast<const Terms&>(tm));
  return trace_dynamic_launch(args, vehicles, g, s);
}

}  // namespace acmpc
