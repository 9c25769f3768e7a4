// gfx950 kernels of mode D (the dynamic bicycle, acmpc_dynamic.h), their launch templates and the launchers of the
// units that instantiate them.  Internal: included only by acmpc_dynamic*.hip.  A rollout that scores every candidate and a
// finalize that re-rolls the winner into the standard record: two plain launches ordered by the stream, nothing crosses
// workgroups inside a launch, every store is a vector store.
//
//   rollout_dynamic_kernel   256 lanes per workgroup, one or two candidates per lane (CPT; two = f32x2, v_pk_*
//                            instructions).  The waypoint rows and the search keys are staged in LDS once per workgroup
//                            (stage_dynamic_tables); the vehicle's constants are a kernel argument (SGPRs).  Each workgroup
//                            writes its candidates' costs and ONE partial (cost, index) key + feasible count.
//   finalize_dynamic_kernel  one wavefront per problem: argmin over the partial keys, then the winner's trajectory on
//                            broadcast operands with the lanes scanning the waypoints side by side for the search.  With
//                            FinalizeArgs::regenerate it re-draws the winner from the global index in its key instead of
//                            loading it from U (every rank can, after one all-reduce(MIN) of the keys).
//   rollout_dynamic_sampled_kernel   the rollout without a control matrix: a lane draws its candidates' normals (Philox,
//                            sample_kernel's candidates bit for bit) and blends each step's control as it goes; the
//                            knot table, the centre and the reference controls are staged in LDS beside the tables.
//
// An ensemble of K > 1 vehicles (VehicleEnsemble, acmpc_dynamic.h) runs kernels of its own, with ONE WAVEFRONT PER
// VEHICLE: wave k's vehicle index is wave-uniform, so its constants are scalar as one vehicle's are and the step loop is
// the one above.
//   rollout_dynamic_ensemble_kernel   K waves per workgroup over the same 64 CPT candidates; the tables are staged once
//                                     for the K waves; each wave leaves its (c_k, V_k) in LDS, and after one barrier
//                                     wave 0 combines them in k order into the costs, the partial key and the count.
//   finalize_dynamic_ensemble_kernel  K waves per problem: wave k re-rolls the winner under vehicle k (one re-roll of
//                                     latency, not K); the K results are combined as in the rollout; wave 0's
//                                     trajectory is the record's x.
//   rollout_dynamic_sampled_ensemble_kernel   the ensemble rollout without a control matrix: wave 0 draws the workgroup's
//                                     candidates for the K waves.
//
// Every template takes FINE and a parameter pack `TM... tm`.  FINE = false is the step loop of the default integration
// setting; FINE = true makes a control step M Euler sub-steps - a scalar loop on a kernel argument - with the low-speed blend
// after each (acmpc_dynamic.h: Integration, dynamic_advance_fine).  The pack is empty - nothing of the terms is compiled - or
// one struct of the handle's settings: the general step of FINE = true (M = 1 under the default integration) plus that
// struct's parts behind scalar switches on the kernel argument.  One unit per kind of pack, so that no unit's code object
// is touched by another's kernels (why kernels of their own: DESIGN.md section 4.10); launch_*_dynamic (acmpc_dynamic.hip)
// takes the first row whose setting is on:
//
//   unit                          pack                                setter (acmpc_set_...)        kernels  launched while
//   acmpc_dynamic_road.hip        TermsRoad, WithObstacles<           road                          2 x 16   a road table is set and the actuator lag
//                                 TermsRoad>                                                                is off (with obstacles: the second pack)
//   acmpc_dynamic_road_actuator   WithActuator<TermsRoad |            road + dynamics_actuator      2 x 16   a road table is set and the actuator lag
//   .hip                          WithObstacles<TermsRoad>>                                                 is on
//   acmpc_dynamic_actuator.hip    WithActuator<TermsAero |            dynamics_actuator             4 x 16   the actuator lag is on: over the aero
//                                 TermsSurface | WithObstacles<                                             step, or the surface step while a table
//                                 TermsAero | TermsSurface>>                                                is set; with obstacles: over their pack
//   acmpc_dynamic_surface.hip     TermsSurface, WithObstacles<        surface                       2 x 16   a surface table is set (with obstacles:
//                                 TermsSurface>                                                             the second pack)
//   acmpc_dynamic_obstacles.hip   WithObstacles<TermsObjective |      obstacles                     4 x 16   obstacles are set: the pack of the
//                                 TermsCoupled | TermsLoaded |                                              step the handle would take without
//                                 TermsAero>
//   acmpc_dynamic_aero.hip        TermsAero                           dynamics_downforce            16       the downforce is on
//   acmpc_dynamic_loaded.hip      TermsLoaded                         dynamics_load_transfer        16       the load transfer is on
//   acmpc_dynamic_coupled.hip     TermsCoupled                        dynamics_coupling             16       the tyre coupling is on
//   acmpc_dynamic_terms.hip       TermsObjective                      dynamics_objective            16       progress or ceiling is on
//                                 Terms                               dynamics_terms                16       only rate or slip terms are on
//   acmpc_dynamic.hip             (empty), FINE = true                dynamics_integration          16       none of the above, a setting
//                                 (empty), FINE = false               -                             16       none of the above, the default
//
// Built with -ffp-contract=off: see acmpc_device.h.
#pragma once
#include "acmpc_dynamic.h"
#include "acmpc_kernels_impl.h"

#include <cstring>
#include <type_traits>

#pragma clang fp contract(off)

namespace acmpc {

namespace {

constexpr int kDynBlock = 256;

// control (delta, pedal) of candidate c of problem p at step i
template <int LAYOUT>
__device__ __forceinline__ void load_dynamic_control(const float* __restrict__ U, int p, int N, int n, int i, int c,
                                                     float& d, float& q) {
  if constexpr (LAYOUT == 1) {   // U[p][i][0|1][c]: lanes read consecutive candidates
    const float* row = U + (static_cast<size_t>(p) * n + i) * 2 * static_cast<size_t>(N) + c;
    d = row[0];
    q = row[N];
  } else {                       // U[p][c][i][0|1]
    const f32x2 dq = *reinterpret_cast<const f32x2*>(U + ((static_cast<size_t>(p) * N + c) * n + i) * 2);
    d = dq[0];
    q = dq[1];
  }
}

// the first minimum of the search key over all n waypoints (temporal_nearest on the pose alone)
template <typename F>
__device__ __forceinline__ typename IndexOf<F>::type nearest_all(F X, F Y, const float* abc, int n) {
  StateT_<F> probe{};
  probe.X = X;
  probe.Y = Y;
  return temporal_nearest<F>(probe, abc, n);
}

template <int SEARCH>
__device__ __forceinline__ int dynamic_nearest(float X, float Y, const float* abc, int n, const Weights& w, int j_prev) {
  if constexpr (SEARCH == kSearchExhaustive) {
    return nearest_all<float>(X, Y, abc, n);
  } else {
    return temporal_nearest_window<SEARCH>(X, Y, abc, n, j_prev, w.nn_back, w.nn_ahead);
  }
}
template <int SEARCH>
__device__ __forceinline__ i32x2 dynamic_nearest(f32x2 X, f32x2 Y, const float* abc, int n, const Weights& w, i32x2 j_prev) {
  if constexpr (SEARCH == kSearchExhaustive) {
    return nearest_all<f32x2>(X, Y, abc, n);
  } else {
    i32x2 j;
    j[0] = temporal_nearest_window<SEARCH>(X[0], Y[0], abc, n, j_prev[0], w.nn_back, w.nn_ahead);
    j[1] = temporal_nearest_window<SEARCH>(X[1], Y[1], abc, n, j_prev[1], w.nn_back, w.nn_ahead);
    return j;
  }
}

__device__ __forceinline__ void dynamic_settle(StateD& s, const float* wp, int j, float d, float q, const Weights& w) {
  float row[kCoefT];
  load_row(wp, j, row);
  dynamic_cost<float>(s, row, d, q, w);
}
__device__ __forceinline__ void dynamic_settle(StateD_<f32x2>& s, const float* wp, i32x2 j, f32x2 d, f32x2 q,
                                               const Weights& w) {
  f32x2 g[kCoefT];
  float g0[kCoefT], g1[kCoefT];
  load_row(wp, j[0], g0);
  load_row(wp, j[1], g1);
#pragma unroll
  for (int e = 0; e < kCoefT; ++e) {
    g[e][0] = g0[e];
    g[e][1] = g1[e];
  }
  dynamic_cost<f32x2>(s, g, d, q, w);
}

template <int LAYOUT, int CPT, bool FINE, typename... TM>
__global__ void __launch_bounds__(kDynBlock)
    rollout_dynamic_kernel(const RolloutArgs a, const Vehicle veh, const Integration g, const TM... tm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // carve: [0, 32) wave keys | [32, 48) wave feasible counts | [64, ...) waypoint rows, then the search keys
  int64_t* s_key = reinterpret_cast<int64_t*>(smem);
  int* s_feas = reinterpret_cast<int*>(smem + 32);
  float* s_wp = reinterpret_cast<float*>(smem + 64);
  const int n = a.n;
  float* s_xy = s_wp + n * kCoefT;
  const int p = static_cast<int>(blockIdx.y);
  const int tid = static_cast<int>(threadIdx.x);
  const int c0 = (static_cast<int>(blockIdx.x) * kDynBlock + tid) * CPT;
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefT;
  const float* __restrict__ x0 = a.x0 + static_cast<size_t>(p) * kDynamicStateFloats;
  stage_dynamic_tables(coef, n, tid, kDynBlock, veh.wheelbase, s_wp, s_xy);
  __syncthreads();

  // every lane rolls CPT real candidates; past the problem's end (the tail of the last workgroup, an odd N's last pair)
  // it repeats candidate N - 1, whose cost it does not report - no lane diverges from the step loop
  using F = typename std::conditional<CPT == 2, f32x2, float>::type;
  using I = typename IndexOf<F>::type;
  int cand[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) cand[j] = min(c0 + j, a.N - 1);
  StateD_<F> st = start_dynamic<F>(x0, coef);
  constexpr bool kTerms = sizeof...(TM) != 0;
  [[maybe_unused]] TermsState<F> ts;
  if constexpr (kTerms) ts = start_terms<F>(p, tm...);
  [[maybe_unused]] ActuatorState<F> as;   // (the actuator lag: the two positions, a0[p] or step 0's command)
  if constexpr (kActuatorPack<TM...>) as = start_actuator<F>(p, lag_of(tm...));
  I nearest = I(0);
  with_search_kind(w, n, [&](auto kind) {
    constexpr int kKind = (decltype(kind)::value == kSearchVerified) ? kSearchExhaustive : decltype(kind)::value;
    for (int i = 0; i < n; ++i) {
      [[maybe_unused]] RoadRow<F> rr;   // (the road table: the row of the last step's waypoint, loaded like the scales)
      if constexpr (kRoadPack<TM...>) rr = road_row<F>(p, n, nearest, tm...);
      [[maybe_unused]] SurfaceScales<F> ms;   // (the surface table: the scales of the last step's waypoint, loaded ahead of the control)
      if constexpr (kSurfacePack<TM...>) ms = surface_scales<F>(p, n, nearest, tm...);
      F d, q;
      if constexpr (CPT == 2) {
        float d0, q0, d1, q1;
        load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, cand[0], d0, q0);
        load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, cand[CPT - 1], d1, q1);
        d = f32x2{d0, d1};
        q = f32x2{q0, q1};
      } else {
        load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, cand[0], d, q);
      }
      F dx = d, qx = q;   // (what the step is driven on: the command, or what the actuator lag makes of it)
      if constexpr (kActuatorPack<TM...>) actuator_step<F>(i, d, q, as, lag_of(tm...), dx, qx);
      if constexpr (kRoadPack<TM...>) dynamic_advance_fine<F, RoadPeaks<F>>(st, dx, qx, veh, g, g.inv_L[0], road_peaks<F>(aero_peaks(0, tm...), veh, rr));
      else if constexpr (kSurfacePack<TM...>) dynamic_advance_fine<F, AeroPeaks<SurfacePeaks<F>>>(st, dx, qx, veh, g, g.inv_L[0], surface_peaks<F>(aero_peaks(0, tm...), veh, ms));
      else if constexpr (kAeroPack<TM...>) dynamic_advance_fine<F, AeroPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[0], aero_peaks(0, tm...));
      else if constexpr (kLoadedPack<TM...>) dynamic_advance_fine<F, LoadedPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[0], loaded_peaks(0, tm...));
      else if constexpr (kCoupledPack<TM...>) dynamic_advance_fine<F, CoupledPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[0], coupled_peaks(tm...));
      else dynamic_control_step<FINE, F>(st, dx, qx, veh, w.dt, g, g.inv_L[0]);
      nearest = dynamic_nearest<kKind>(st.t.X, st.t.Y, s_xy, n, w, nearest);
      dynamic_settle(st, s_wp, nearest, d, q, w);
      if constexpr (kTerms) dynamic_terms<F>(st, d, q, i, p, veh, s_wp, nearest, ts, tm...);
    }
  });
  F cost_v;
  if constexpr (kTerms) cost_v = finish_dynamic_terms<F>(st, ts, s_wp, nearest, p, n, w, tm...);
  else cost_v = finish_temporal<F>(st.t, n, w);
  float cost[CPT];
  bool feas[CPT];
  if constexpr (CPT == 2) {
    cost[0] = cost_v[0];
    cost[1] = cost_v[1];
    feas[0] = st.t.V[0] == 0.0f;
    feas[1] = st.t.V[1] == 0.0f;
  } else {
    cost[0] = cost_v;
    feas[0] = st.t.V == 0.0f;
  }
  int64_t key = kKeyMax;
  int nfeas = 0;
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    if (c0 + j < a.N) {
      if (a.costs != nullptr) a.costs[static_cast<size_t>(p) * a.N + c0 + j] = cost[j];
      const int64_t kj = pack_key(cost[j], static_cast<uint32_t>(a.index_offset + c0 + j));
      key = (kj < key) ? kj : key;
      nfeas += feas[j] ? 1 : 0;
    }
  }
  key = wave_min_key(key);
  nfeas = wave_sum_int(nfeas);
  constexpr int kWaves = kDynBlock / kWave;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  if (lane == 0) {
    s_key[wave] = key;
    s_feas[wave] = nfeas;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int q = 1; q < kWaves; ++q) {
      key = (s_key[q] < key) ? s_key[q] : key;
      nfeas += s_feas[q];
    }
    const size_t slot = static_cast<size_t>(p) * gridDim.x + blockIdx.x;
    a.partial_keys[slot] = key;
    a.partial_feas[slot] = nfeas;
  }
}

// ---- candidates drawn inside the rollout (launch_rollout_dynamic_sampled) -----------------------------------------------
// What a mode D kernel needs of SampleArgs to draw its own candidates - sample_kernel's candidates, bit for bit: Philox
// counter (uint32(index_offset + c), problem, round, draw), key = seed, draw_normal_block / candidate_amplitude /
// blend_control of acmpc_device.h.  A handful of scalars: the input box is the Weights' (the launcher checks that the
// spec's is the same), the knot table is staged in LDS, and the nine knot bounds of SampleSpec stay out of the SGPRs.
struct DynamicDraw {
  const float* centre;     // [P] x centre_stride floats
  const float* u_ref;      // [P][n][2] or nullptr: candidate 1
  const float* segments;   // [n][2]: left knot (as float), weight of the left knot
  const uint32_t* seed_ptr;
  int centre_stride;
  uint32_t seed_lo, seed_hi, round;
  float sigma_d, sigma_p;
};

constexpr int kDrawFloatsPerStep = 6;   // LDS behind the tables: [n][2] knot table | [n][2] centre | [n][2] reference
constexpr int kDrawSlots = 4;           // knots' pairs of normals resident per candidate (two Philox blocks): roll_sampled

__device__ __forceinline__ SampleSpec draw_spec(const DynamicDraw& d, const Weights& w) {
  SampleSpec sp{};
  sp.seed_lo = d.seed_ptr != nullptr ? d.seed_ptr[0] : d.seed_lo;
  sp.seed_hi = d.seed_ptr != nullptr ? d.seed_ptr[1] : d.seed_hi;
  sp.seed_ptr = nullptr;
  sp.round = d.round;
  sp.sigma_v = d.sigma_d;
  sp.sigma_k = d.sigma_p;
  sp.ulo0 = w.ulo0;
  sp.ulo1 = w.ulo1;
  sp.uhi0 = w.uhi0;
  sp.uhi1 = w.uhi1;
  return sp;
}

// knot table, centre and reference controls (the centre again when there are none) of problem p -> LDS, by the workgroup
__device__ __forceinline__ void stage_draw_tables(const DynamicDraw& d, int p, int n, int tid, int threads, float* s_seg,
                                                  float* s_centre, float* s_ref) {
  const float* __restrict__ centre = d.centre + static_cast<size_t>(p) * d.centre_stride;
  const float* __restrict__ ref = d.u_ref != nullptr ? d.u_ref + static_cast<size_t>(p) * n * 2 : centre;
  for (int e = tid; e < 2 * n; e += threads) {
    s_seg[e] = d.segments[e];
    s_centre[e] = centre[e];
    s_ref[e] = ref[e];
  }
}

// The step loop of rollout_dynamic_kernel with the controls drawn as it goes.  The normals stay out of the registers (the
// step loop has none to spare): knot k's pair lives in LDS slot k & 3 of its lane - s_z
// [4][row][CPT] pairs - which holds two Philox blocks (block b = knots 2b, 2b + 1) at a time, and a step reads the two knots
// that bracket it.  When the step's left knot changes - a wave-uniform event, at most seven times a rollout - the blocks of
// the new pair are drawn unless resident: four draws per candidate, as draw_normals() makes.  SHARED (the ensemble: the K
// waves of a workgroup roll the same candidates): one wave draws for all, between two barriers that every wave reaches -
// the knot changes are the same steps in every wave.
template <int CPT, bool SHARED, bool FINE, typename F, typename... TT>
__device__ __forceinline__ void roll_sampled(StateD_<F>& st, const SampleSpec& sp, const Vehicle& veh, const Weights& w,
                                             const Integration& g, const float inv_L, const int p, const int n, const uint32_t (&gidx)[CPT], const bool has_ref,
                                             const float* s_wp, const float* s_xy, const float* s_seg,
                                             const float* s_centre, const float* s_ref, f32x2* s_z, const int row,
                                             const int zi, const bool draws, [[maybe_unused]] const int vk, TT&... tt) {
  using I = typename IndexOf<F>::type;
  constexpr bool kTerms = sizeof...(TT) != 0;   // (tt: nothing, or the terms' state and the Terms)
  float amp[CPT];
  const float* cen[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const bool use_ref = has_ref && gidx[j] == 1u;   // candidate 1 = the reference controls: amplitude 0, own centre
    amp[j] = use_ref ? 0.0f : candidate_amplitude(gidx[j]);
    cen[j] = use_ref ? s_ref : s_centre;
  }
  [[maybe_unused]] LoadedPeaks<VehiclePeaks> loaded{};   // (the scalars of vehicle vk: read once, ahead of the step loop)
  if constexpr (kLoadedPack<TT...>) loaded = loaded_peaks(vk, tt...);
  [[maybe_unused]] AeroPeaks<VehiclePeaks> aero{};
  if constexpr (kAeroPack<TT...> || kSurfacePack<TT...> || kRoadPack<TT...>) aero = aero_peaks(vk, tt...);
  int resident[2] = {-1, -1};   // the Philox block in slots 0, 1 and in slots 2, 3
  int knot = -1;
  [[maybe_unused]] ActuatorState<F> as;   // (the actuator lag: the two positions, a0[p] or step 0's command)
  if constexpr (kActuatorPack<TT...>) as = start_actuator<F>(p, lag_of(tt...));
  I nearest = I(0);
  with_search_kind(w, n, [&](auto kind) {
    constexpr int kKind = (decltype(kind)::value == kSearchVerified) ? kSearchExhaustive : decltype(kind)::value;
    for (int i = 0; i < n; ++i) {
      [[maybe_unused]] RoadRow<F> rr;   // (the road table: the row of the last step's waypoint, loaded like the scales)
      if constexpr (kRoadPack<TT...>) rr = road_row<F>(p, n, nearest, tt...);
      [[maybe_unused]] SurfaceScales<F> ms;   // (the surface table: loaded ahead of the draw)
      if constexpr (kSurfacePack<TT...>) ms = surface_scales<F>(p, n, nearest, tt...);
      const int k0 = __builtin_amdgcn_readfirstlane(static_cast<int>(s_seg[2 * i]));
      if (k0 != knot) {
        knot = k0;
        if constexpr (SHARED) __syncthreads();   // every wave has read the old pair for the last time
#pragma nounroll
        for (int b = k0 >> 1; b <= (k0 + 1) >> 1; ++b) {
          if (resident[b & 1] == b) continue;
          resident[b & 1] = b;
          if (draws) {
#pragma nounroll
            for (int j = 0; j < CPT; ++j) {   // (one candidate at a time: two interleaved Philox blocks cost a wave of occupancy)
              float z[4];
              draw_normal_block(sp, j == 0 ? gidx[0] : gidx[CPT - 1], static_cast<uint32_t>(p), static_cast<uint32_t>(b), z);
              s_z[((2 * (b & 1)) * row + zi) * CPT + j] = f32x2{z[0], z[1]};
              s_z[((2 * (b & 1) + 1) * row + zi) * CPT + j] = f32x2{z[2], z[3]};
            }
          }
        }
        if constexpr (SHARED) __syncthreads();
      }
      const float w0 = s_seg[2 * i + 1];
      const f32x2* zl = s_z + ((k0 & 3) * row + zi) * CPT;
      const f32x2* zr = s_z + (((k0 + 1) & 3) * row + zi) * CPT;
      float dj[CPT], qj[CPT];
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const f32x2 l = zl[j], r = zr[j];
        blend_control(sp, amp[j], w0, cen[j][2 * i], cen[j][2 * i + 1], l[0], l[1], r[0], r[1], dj[j], qj[j]);
      }
      F d, q;
      if constexpr (CPT == 2) {
        d = f32x2{dj[0], dj[1]};
        q = f32x2{qj[0], qj[1]};
      } else {
        d = dj[0];
        q = qj[0];
      }
      F dx = d, qx = q;   // (what the step is driven on: the command, or what the actuator lag makes of it)
      if constexpr (kActuatorPack<TT...>) actuator_step<F>(i, d, q, as, lag_of(tt...), dx, qx);
      if constexpr (kRoadPack<TT...>) dynamic_advance_fine<F, RoadPeaks<F>>(st, dx, qx, veh, g, inv_L, road_peaks<F>(aero, veh, rr));
      else if constexpr (kSurfacePack<TT...>) dynamic_advance_fine<F, AeroPeaks<SurfacePeaks<F>>>(st, dx, qx, veh, g, inv_L, surface_peaks<F>(aero, veh, ms));
      else if constexpr (kAeroPack<TT...>) dynamic_advance_fine<F, AeroPeaks<VehiclePeaks>>(st, dx, qx, veh, g, inv_L, aero);
      else if constexpr (kLoadedPack<TT...>) dynamic_advance_fine<F, LoadedPeaks<VehiclePeaks>>(st, dx, qx, veh, g, inv_L, loaded);
      else if constexpr (kCoupledPack<TT...>) dynamic_advance_fine<F, CoupledPeaks<VehiclePeaks>>(st, dx, qx, veh, g, inv_L, coupled_peaks(tt...));
      else dynamic_control_step<FINE, F>(st, dx, qx, veh, w.dt, g, inv_L);
      nearest = dynamic_nearest<kKind>(st.t.X, st.t.Y, s_xy, n, w, nearest);
      dynamic_settle(st, s_wp, nearest, d, q, w);
      if constexpr (kTerms) dynamic_terms<F>(st, d, q, i, p, veh, s_wp, nearest, tt...);   // (the state keeps this step's blended control)
    }
  });
  if constexpr (kTerms) keep_nearest<F>(nearest, tt...);   // (the progress part reads the last step's at the finish)
}

// rollout_dynamic_kernel without a control matrix: the same workgroup shape, tail rule (lanes past N repeat candidate
// N - 1 unreported), costs, partial keys and feasible counts.
template <int CPT, bool FINE, typename... TM>
__global__ void __launch_bounds__(kDynBlock)
    rollout_dynamic_sampled_kernel(const RolloutArgs a, const DynamicDraw smp, const Vehicle veh, const Integration g,
                                   const TM... tm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // carve: [0, 32) wave keys | [32, 48) wave feasible counts | [64, ...) the lanes' normals [4][256][CPT] pairs, waypoint
  // rows, search keys, the draw's tables
  int64_t* s_key = reinterpret_cast<int64_t*>(smem);
  int* s_feas = reinterpret_cast<int*>(smem + 32);
  f32x2* s_z = reinterpret_cast<f32x2*>(smem + 64);
  float* s_wp = reinterpret_cast<float*>(s_z + kDrawSlots * kDynBlock * CPT);
  const int n = a.n;
  float* s_xy = s_wp + n * kCoefT;
  float* s_seg = s_xy + n * kKeyStride;
  float* s_centre = s_seg + 2 * n;
  float* s_ref = s_centre + 2 * n;
  const int p = static_cast<int>(blockIdx.y);
  const int tid = static_cast<int>(threadIdx.x);
  const int c0 = (static_cast<int>(blockIdx.x) * kDynBlock + tid) * CPT;
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefT;
  const float* __restrict__ x0 = a.x0 + static_cast<size_t>(p) * kDynamicStateFloats;
  stage_dynamic_tables(coef, n, tid, kDynBlock, veh.wheelbase, s_wp, s_xy);
  stage_draw_tables(smp, p, n, tid, kDynBlock, s_seg, s_centre, s_ref);
  __syncthreads();

  using F = typename std::conditional<CPT == 2, f32x2, float>::type;
  uint32_t gidx[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) gidx[j] = static_cast<uint32_t>(a.index_offset + min(c0 + j, a.N - 1));
  StateD_<F> st = start_dynamic<F>(x0, coef);
  constexpr bool kTerms = sizeof...(TM) != 0;
  [[maybe_unused]] TermsState<F> ts;
  if constexpr (kTerms) ts = start_terms<F>(p, tm...);
  roll_sampled<CPT, false, FINE, F>(st, draw_spec(smp, w), veh, w, g, g.inv_L[0], p, n, gidx, smp.u_ref != nullptr, s_wp,
                                    s_xy, s_seg, s_centre, s_ref, s_z, kDynBlock, tid, true, 0, state_of(ts, tm)..., tm...);
  F cost_v;
  if constexpr (kTerms) cost_v = finish_dynamic_terms<F>(st, ts, s_wp, ts.j, p, n, w, tm...);
  else cost_v = finish_temporal<F>(st.t, n, w);
  float cost[CPT];
  bool feas[CPT];
  if constexpr (CPT == 2) {
    cost[0] = cost_v[0];
    cost[1] = cost_v[1];
    feas[0] = st.t.V[0] == 0.0f;
    feas[1] = st.t.V[1] == 0.0f;
  } else {
    cost[0] = cost_v;
    feas[0] = st.t.V == 0.0f;
  }
  int64_t key = kKeyMax;
  int nfeas = 0;
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    if (c0 + j < a.N) {
      if (a.costs != nullptr) a.costs[static_cast<size_t>(p) * a.N + c0 + j] = cost[j];
      const int64_t kj = pack_key(cost[j], static_cast<uint32_t>(a.index_offset + c0 + j));
      key = (kj < key) ? kj : key;
      nfeas += feas[j] ? 1 : 0;
    }
  }
  key = wave_min_key(key);
  nfeas = wave_sum_int(nfeas);
  constexpr int kWaves = kDynBlock / kWave;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  if (lane == 0) {
    s_key[wave] = key;
    s_feas[wave] = nfeas;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int q = 1; q < kWaves; ++q) {
      key = (s_key[q] < key) ? s_key[q] : key;
      nfeas += s_feas[q];
    }
    const size_t slot = static_cast<size_t>(p) * gridDim.x + blockIdx.x;
    a.partial_keys[slot] = key;
    a.partial_feas[slot] = nfeas;
  }
}

// The winner's controls re-drawn from its global index (FinalizeArgs::regenerate) into the record image's u block: every
// lane draws the candidate's normals (the same for all), lane `first` + m `stride` blends step first + m stride -
// sample_kernel's arithmetic on the same operands, the bracketing knots picked by a select chain.
__device__ __forceinline__ void regenerate_dynamic_controls(const FinalizeArgs& a, int p, uint32_t gidx, int first,
                                                            int stride, float* su) {
  const int n = a.n;
  float z[kKnots][2];
  draw_normals(a.spec, gidx, static_cast<uint32_t>(p), z);
  const bool use_ref = gidx == 1u && a.u_ref != nullptr;
  const float amp = use_ref ? 0.0f : candidate_amplitude(gidx);
  // (not __restrict__: the centre may be the u block of the very record this launch rewrites - read before the barrier
  // that precedes the record's stores)
  const float* centre = use_ref ? a.u_ref + static_cast<size_t>(p) * n * 2 : a.centre + static_cast<size_t>(p) * a.centre_stride;
  for (int i = first; i < n; i += stride) {
    const int k0 = static_cast<int>(a.spec.segments[2 * i]);
    float z0d = z[0][0], z0p = z[0][1], z1d = z[1][0], z1p = z[1][1];
#pragma unroll
    for (int knot = 1; knot < kKnots - 1; ++knot) {
      const bool hit = (k0 == knot);
      z0d = hit ? z[knot][0] : z0d;
      z0p = hit ? z[knot][1] : z0p;
      z1d = hit ? z[knot + 1][0] : z1d;
      z1p = hit ? z[knot + 1][1] : z1p;
    }
    blend_control(a.spec, amp, a.spec.segments[2 * i + 1], centre[2 * i], centre[2 * i + 1], z0d, z0p, z1d, z1p, su[2 * i],
                  su[2 * i + 1]);
  }
}

template <int LAYOUT, bool FINE, typename... TM>
__global__ void __launch_bounds__(kWave)
    finalize_dynamic_kernel(const FinalizeArgs a, const Vehicle veh, const Integration g, const TM... tm) {
  extern __shared__ __attribute__((aligned(16))) float s_rec[];   // record image, then the waypoint rows and keys
  const int p = static_cast<int>(blockIdx.x);
  const int lane = static_cast<int>(threadIdx.x);
  const int n = a.n;
  int nfeas = 0;
  int64_t key = kKeyMax;
  for (int b = lane; b < a.blocks_per_problem; b += kWave) {
    const size_t slot = static_cast<size_t>(p) * a.blocks_per_problem + b;
    nfeas += a.partial_feas[slot];
    const int64_t kb = a.partial_keys[slot];
    key = (kb < key) ? kb : key;
  }
  nfeas = wave_sum_int(nfeas);
  key = wave_min_key(key);
  if (a.keys_in != nullptr) key = a.keys_in[p];
  if (a.keys_out != nullptr && lane == 0) a.keys_out[p] = key;
  if (a.records == nullptr) return;

  const int rec_floats = 4 + 2 * n + 3 * (n + 1);
  float* __restrict__ rec = a.records + static_cast<size_t>(p) * rec_floats;
  const int64_t local = static_cast<int64_t>(static_cast<uint32_t>(key & 0xffffffffLL)) - a.index_offset;
  // a winner on another rank (or nothing found): a blank record - unless it is re-drawn from its index, which any rank can
  if (!a.regenerate && !(local >= 0 && local < a.N)) {
    for (int e = lane; e < rec_floats; e += kWave) rec[e] = (e == 2) ? static_cast<float>(nfeas) : 0.0f;
    return;
  }
  const int c = static_cast<int>(local);
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefT;
  const float* __restrict__ x0 = a.x0 + static_cast<size_t>(p) * kDynamicStateFloats;
  float* su = s_rec + 4;
  float* sx = s_rec + 4 + 2 * n;
  float* s_wp = s_rec + ((rec_floats + 3) & ~3);
  float* s_abc = s_wp + n * kCoefT;
  stage_dynamic_tables(coef, n, lane, kWave, veh.wheelbase, s_wp, s_abc);
  if (a.regenerate) {
    regenerate_dynamic_controls(a, p, static_cast<uint32_t>(key & 0xffffffffLL), lane, kWave, su);
  } else {
    for (int i = lane; i < n; i += kWave) load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, c, su[2 * i], su[2 * i + 1]);
  }
  StateD st = start_dynamic<float>(x0, coef);
  constexpr bool kTerms = sizeof...(TM) != 0;
  [[maybe_unused]] TermsState<float> ts;
  if constexpr (kTerms) ts = start_terms<float>(p, tm...);
  [[maybe_unused]] ActuatorState<float> as;   // (the actuator lag: the two positions, a0[p] or step 0's command)
  if constexpr (kActuatorPack<TM...>) as = start_actuator<float>(p, lag_of(tm...));
  if (lane == 0) {
    sx[0] = st.t.X + coef[0];   // (poses leave in the caller's frame: start_temporal())
    sx[1] = st.t.Y + coef[1];
    sx[2] = st.t.phi;
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
    const float d = su[2 * i], q = su[2 * i + 1];   // (LDS broadcast: every lane rolls the same state)
    float dx = d, qx = q;   // (what the step is driven on: the command, or what the actuator lag makes of it)
    if constexpr (kActuatorPack<TM...>) actuator_step<float>(i, d, q, as, lag_of(tm...), dx, qx);
    if constexpr (kRoadPack<TM...>) dynamic_advance_fine<float, RoadPeaks<float>>(st, dx, qx, veh, g, g.inv_L[0], road_peaks<float>(aero_peaks(0, tm...), veh, rr));
    else if constexpr (kSurfacePack<TM...>) dynamic_advance_fine<float, AeroPeaks<SurfacePeaks<float>>>(st, dx, qx, veh, g, g.inv_L[0], surface_peaks<float>(aero_peaks(0, tm...), veh, ms));
    else if constexpr (kAeroPack<TM...>) dynamic_advance_fine<float, AeroPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[0], aero_peaks(0, tm...));
    else if constexpr (kLoadedPack<TM...>) dynamic_advance_fine<float, LoadedPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[0], loaded_peaks(0, tm...));
    else if constexpr (kCoupledPack<TM...>) dynamic_advance_fine<float, CoupledPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[0], coupled_peaks(tm...));
    else dynamic_control_step<FINE, float>(st, dx, qx, veh, w.dt, g, g.inv_L[0]);
    // the first minimum of the key over the search's waypoints, the lanes side by side; ties -> the lower index, and the
    // search's first waypoint when no key compares below +inf (as the rollout's `d < best` scans)
    const int lo = exhaustive ? 0 : max(min(j_prev - w.nn_back, n - win_w), 0);
    const int hi = exhaustive ? n - 1 : min(lo + win_w, n) - 1;
    float best = __builtin_inff();
    int j = 0x7fffffff;
    for (int m = lo + lane; m <= hi; m += kWave) {
      const float e = search_key<float>(st.t.X, st.t.Y, s_abc[kKeyStride * m], s_abc[kKeyStride * m + kKeyB],
                                        s_abc[kKeyStride * m + kKeyC]);
      if (e < best) {
        best = e;
        j = m;
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
    if constexpr (kTerms) dynamic_terms<float>(st, d, q, i, p, veh, s_wp, j, ts, tm...);
    if (lane == 0) {
      sx[3 * (i + 1)] = st.t.X + coef[0];
      sx[3 * (i + 1) + 1] = st.t.Y + coef[1];
      sx[3 * (i + 1) + 2] = st.t.phi;
    }
  }
  if (lane == 0) {
    if constexpr (kTerms) s_rec[0] = finish_dynamic_terms<float>(st, ts, s_wp, j_prev, p, n, w, tm...);
    else s_rec[0] = finish_temporal<float>(st.t, n, w);
    s_rec[1] = st.t.V;
    s_rec[2] = static_cast<float>(nfeas);
    s_rec[3] = 1.0f;
  }
  __syncthreads();
  for (int e = lane; e < rec_floats; e += kWave) rec[e] = s_rec[e];
}

template <int LAYOUT, int CPT, bool FINE, typename... TM>
__global__ void __launch_bounds__(kWave * kMaxVehicles)
    rollout_dynamic_ensemble_kernel(const RolloutArgs a, const VehicleEnsemble e, const Integration g, const TM... tm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // carve: [K][64 CPT] per-vehicle costs | [K][64 CPT] per-vehicle violations | waypoint rows | search keys
  constexpr int kPerGroup = kWave * CPT;
  const int K = e.K;
  float* s_c = reinterpret_cast<float*>(smem);
  float* s_v = s_c + K * kPerGroup;
  float* s_wp = s_v + K * kPerGroup;
  const int n = a.n;
  float* s_xy = s_wp + n * kCoefT;
  const int p = static_cast<int>(blockIdx.y);
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & (kWave - 1);
  const int k = __builtin_amdgcn_readfirstlane(tid / kWave);   // this wave's vehicle
  const int c0 = (static_cast<int>(blockIdx.x) * kWave + lane) * CPT;
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefT;
  const float* __restrict__ x0 = a.x0 + static_cast<size_t>(p) * kDynamicStateFloats;
  stage_dynamic_tables(coef, n, tid, kWave * K, e.v[0].wheelbase, s_wp, s_xy);
  __syncthreads();

  const Vehicle veh = e.v[k];
  // the step loop of rollout_dynamic_kernel, under vehicle k
  using F = typename std::conditional<CPT == 2, f32x2, float>::type;
  using I = typename IndexOf<F>::type;
  int cand[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) cand[j] = min(c0 + j, a.N - 1);
  StateD_<F> st = start_dynamic<F>(x0, coef);
  constexpr bool kTerms = sizeof...(TM) != 0;
  [[maybe_unused]] TermsState<F> ts;
  if constexpr (kTerms) ts = start_terms<F>(p, tm...);
  [[maybe_unused]] ActuatorState<F> as;   // (the actuator lag: the two positions, a0[p] or step 0's command)
  if constexpr (kActuatorPack<TM...>) as = start_actuator<F>(p, lag_of(tm...));
  I nearest = I(0);
  with_search_kind(w, n, [&](auto kind) {
    constexpr int kKind = (decltype(kind)::value == kSearchVerified) ? kSearchExhaustive : decltype(kind)::value;
    for (int i = 0; i < n; ++i) {
      [[maybe_unused]] RoadRow<F> rr;   // (the road table: the row of the last step's waypoint, loaded like the scales)
      if constexpr (kRoadPack<TM...>) rr = road_row<F>(p, n, nearest, tm...);
      [[maybe_unused]] SurfaceScales<F> ms;   // (the surface table: the scales of the last step's waypoint, loaded ahead of the control)
      if constexpr (kSurfacePack<TM...>) ms = surface_scales<F>(p, n, nearest, tm...);
      F d, q;
      if constexpr (CPT == 2) {
        float d0, q0, d1, q1;
        load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, cand[0], d0, q0);
        load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, cand[CPT - 1], d1, q1);
        d = f32x2{d0, d1};
        q = f32x2{q0, q1};
      } else {
        load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, cand[0], d, q);
      }
      F dx = d, qx = q;   // (what the step is driven on: the command, or what the actuator lag makes of it)
      if constexpr (kActuatorPack<TM...>) actuator_step<F>(i, d, q, as, lag_of(tm...), dx, qx);
      if constexpr (kRoadPack<TM...>) dynamic_advance_fine<F, RoadPeaks<F>>(st, dx, qx, veh, g, g.inv_L[k], road_peaks<F>(aero_peaks(k, tm...), veh, rr));
      else if constexpr (kSurfacePack<TM...>) dynamic_advance_fine<F, AeroPeaks<SurfacePeaks<F>>>(st, dx, qx, veh, g, g.inv_L[k], surface_peaks<F>(aero_peaks(k, tm...), veh, ms));
      else if constexpr (kAeroPack<TM...>) dynamic_advance_fine<F, AeroPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], aero_peaks(k, tm...));
      else if constexpr (kLoadedPack<TM...>) dynamic_advance_fine<F, LoadedPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], loaded_peaks(k, tm...));
      else if constexpr (kCoupledPack<TM...>) dynamic_advance_fine<F, CoupledPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], coupled_peaks(tm...));
      else dynamic_control_step<FINE, F>(st, dx, qx, veh, w.dt, g, g.inv_L[k]);
      nearest = dynamic_nearest<kKind>(st.t.X, st.t.Y, s_xy, n, w, nearest);
      dynamic_settle(st, s_wp, nearest, d, q, w);
      if constexpr (kTerms) dynamic_terms<F>(st, d, q, i, p, veh, s_wp, nearest, ts, tm...);
    }
  });
  F cost_v;
  if constexpr (kTerms) cost_v = finish_dynamic_terms<F>(st, ts, s_wp, nearest, p, n, w, tm...);
  else cost_v = finish_temporal<F>(st.t, n, w);
  if constexpr (CPT == 2) {
    s_c[k * kPerGroup + 2 * lane] = cost_v[0];
    s_c[k * kPerGroup + 2 * lane + 1] = cost_v[1];
    s_v[k * kPerGroup + 2 * lane] = st.t.V[0];
    s_v[k * kPerGroup + 2 * lane + 1] = st.t.V[1];
  } else {
    s_c[k * kPerGroup + lane] = cost_v;
    s_v[k * kPerGroup + lane] = st.t.V;
  }
  __syncthreads();
  if (k != 0) return;   // (wave-uniform: no barrier follows)
  int64_t key = kKeyMax;
  int nfeas = 0;
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    float J, V;
    ensemble_combine(s_c + CPT * lane + j, s_v + CPT * lane + j, kPerGroup, e, J, V);
    if (c0 + j < a.N) {
      if (a.costs != nullptr) a.costs[static_cast<size_t>(p) * a.N + c0 + j] = J;
      const int64_t kj = pack_key(J, static_cast<uint32_t>(a.index_offset + c0 + j));
      key = (kj < key) ? kj : key;
      nfeas += (V == 0.0f) ? 1 : 0;
    }
  }
  key = wave_min_key(key);
  nfeas = wave_sum_int(nfeas);
  if (lane == 0) {
    const size_t slot = static_cast<size_t>(p) * gridDim.x + blockIdx.x;
    a.partial_keys[slot] = key;
    a.partial_feas[slot] = nfeas;
  }
}

// rollout_dynamic_ensemble_kernel without a control matrix: wave 0 draws the workgroup's 64 CPT candidates for the K waves
// (roll_sampled's SHARED form)
template <int CPT, bool FINE, typename... TM>
__global__ void __launch_bounds__(kWave * kMaxVehicles)
    rollout_dynamic_sampled_ensemble_kernel(const RolloutArgs a, const DynamicDraw smp, const VehicleEnsemble e,
                                            const Integration g, const TM... tm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // carve: [K][64 CPT] per-vehicle costs | [K][64 CPT] per-vehicle violations | the candidates' normals [4][64][CPT] pairs |
  // waypoint rows | search keys | draw tables
  constexpr int kPerGroup = kWave * CPT;
  const int K = e.K;
  float* s_c = reinterpret_cast<float*>(smem);
  float* s_v = s_c + K * kPerGroup;
  f32x2* s_z = reinterpret_cast<f32x2*>(s_v + K * kPerGroup);
  float* s_wp = reinterpret_cast<float*>(s_z + kDrawSlots * kWave * CPT);
  const int n = a.n;
  float* s_xy = s_wp + n * kCoefT;
  float* s_seg = s_xy + n * kKeyStride;
  float* s_centre = s_seg + 2 * n;
  float* s_ref = s_centre + 2 * n;
  const int p = static_cast<int>(blockIdx.y);
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & (kWave - 1);
  const int k = __builtin_amdgcn_readfirstlane(tid / kWave);   // this wave's vehicle
  const int c0 = (static_cast<int>(blockIdx.x) * kWave + lane) * CPT;
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefT;
  const float* __restrict__ x0 = a.x0 + static_cast<size_t>(p) * kDynamicStateFloats;
  stage_dynamic_tables(coef, n, tid, kWave * K, e.v[0].wheelbase, s_wp, s_xy);
  stage_draw_tables(smp, p, n, tid, kWave * K, s_seg, s_centre, s_ref);
  __syncthreads();

  const Vehicle veh = e.v[k];
  using F = typename std::conditional<CPT == 2, f32x2, float>::type;
  uint32_t gidx[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) gidx[j] = static_cast<uint32_t>(a.index_offset + min(c0 + j, a.N - 1));
  StateD_<F> st = start_dynamic<F>(x0, coef);
  constexpr bool kTerms = sizeof...(TM) != 0;
  [[maybe_unused]] TermsState<F> ts;
  if constexpr (kTerms) ts = start_terms<F>(p, tm...);
  roll_sampled<CPT, true, FINE, F>(st, draw_spec(smp, w), veh, w, g, g.inv_L[k], p, n, gidx, smp.u_ref != nullptr, s_wp,
                                   s_xy, s_seg, s_centre, s_ref, s_z, kWave, lane, k == 0, k, state_of(ts, tm)..., tm...);
  F cost_v;
  if constexpr (kTerms) cost_v = finish_dynamic_terms<F>(st, ts, s_wp, ts.j, p, n, w, tm...);
  else cost_v = finish_temporal<F>(st.t, n, w);
  if constexpr (CPT == 2) {
    s_c[k * kPerGroup + 2 * lane] = cost_v[0];
    s_c[k * kPerGroup + 2 * lane + 1] = cost_v[1];
    s_v[k * kPerGroup + 2 * lane] = st.t.V[0];
    s_v[k * kPerGroup + 2 * lane + 1] = st.t.V[1];
  } else {
    s_c[k * kPerGroup + lane] = cost_v;
    s_v[k * kPerGroup + lane] = st.t.V;
  }
  __syncthreads();
  if (k != 0) return;   // (wave-uniform: no barrier follows)
  int64_t key = kKeyMax;
  int nfeas = 0;
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    float J, V;
    ensemble_combine(s_c + CPT * lane + j, s_v + CPT * lane + j, kPerGroup, e, J, V);
    if (c0 + j < a.N) {
      if (a.costs != nullptr) a.costs[static_cast<size_t>(p) * a.N + c0 + j] = J;
      const int64_t kj = pack_key(J, static_cast<uint32_t>(a.index_offset + c0 + j));
      key = (kj < key) ? kj : key;
      nfeas += (V == 0.0f) ? 1 : 0;
    }
  }
  key = wave_min_key(key);
  nfeas = wave_sum_int(nfeas);
  if (lane == 0) {
    const size_t slot = static_cast<size_t>(p) * gridDim.x + blockIdx.x;
    a.partial_keys[slot] = key;
    a.partial_feas[slot] = nfeas;
  }
}

template <int LAYOUT, bool FINE, typename... TM>
__global__ void __launch_bounds__(kWave * kMaxVehicles)
    finalize_dynamic_ensemble_kernel(const FinalizeArgs a, const VehicleEnsemble e, const Integration g, const TM... tm) {
  // record image | [kMaxVehicles] costs, [kMaxVehicles] violations | waypoint rows | search keys
  extern __shared__ __attribute__((aligned(16))) float s_rec[];
  const int p = static_cast<int>(blockIdx.x);
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & (kWave - 1);
  const int k = __builtin_amdgcn_readfirstlane(tid / kWave);   // this wave's vehicle
  const int threads = kWave * e.K;
  const int n = a.n;
  // every wave takes the argmin itself: the same loads, the same key, no barrier
  int nfeas = 0;
  int64_t key = kKeyMax;
  for (int b = lane; b < a.blocks_per_problem; b += kWave) {
    const size_t slot = static_cast<size_t>(p) * a.blocks_per_problem + b;
    nfeas += a.partial_feas[slot];
    const int64_t kb = a.partial_keys[slot];
    key = (kb < key) ? kb : key;
  }
  nfeas = wave_sum_int(nfeas);
  key = wave_min_key(key);
  if (a.keys_in != nullptr) key = a.keys_in[p];
  if (a.keys_out != nullptr && tid == 0) a.keys_out[p] = key;
  if (a.records == nullptr) return;

  const int rec_floats = 4 + 2 * n + 3 * (n + 1);
  float* __restrict__ rec = a.records + static_cast<size_t>(p) * rec_floats;
  const int64_t local = static_cast<int64_t>(static_cast<uint32_t>(key & 0xffffffffLL)) - a.index_offset;
  // a winner on another rank (or nothing found): a blank record - unless it is re-drawn from its index, which any rank can
  if (!a.regenerate && !(local >= 0 && local < a.N)) {
    for (int q = tid; q < rec_floats; q += threads) rec[q] = (q == 2) ? static_cast<float>(nfeas) : 0.0f;
    return;
  }
  const int c = static_cast<int>(local);
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefT;
  const float* __restrict__ x0 = a.x0 + static_cast<size_t>(p) * kDynamicStateFloats;
  float* su = s_rec + 4;
  float* sx = s_rec + 4 + 2 * n;
  float* s_ck = s_rec + ((rec_floats + 3) & ~3);
  float* s_wp = s_ck + 2 * kMaxVehicles;
  float* s_abc = s_wp + n * kCoefT;
  stage_dynamic_tables(coef, n, tid, threads, e.v[0].wheelbase, s_wp, s_abc);
  if (a.regenerate) {
    regenerate_dynamic_controls(a, p, static_cast<uint32_t>(key & 0xffffffffLL), tid, threads, su);
  } else {
    for (int i = tid; i < n; i += threads) load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, c, su[2 * i], su[2 * i + 1]);
  }
  StateD st = start_dynamic<float>(x0, coef);
  constexpr bool kTerms = sizeof...(TM) != 0;
  [[maybe_unused]] TermsState<float> ts;
  if constexpr (kTerms) ts = start_terms<float>(p, tm...);
  [[maybe_unused]] ActuatorState<float> as;   // (the actuator lag: the two positions, a0[p] or step 0's command)
  if constexpr (kActuatorPack<TM...>) as = start_actuator<float>(p, lag_of(tm...));
  const bool writer = (k == 0 && lane == 0);   // vehicle 0's trajectory is the record's
  if (writer) {
    sx[0] = st.t.X + coef[0];
    sx[1] = st.t.Y + coef[1];
    sx[2] = st.t.phi;
  }
  __syncthreads();
  const Vehicle veh = e.v[k];
  const bool exhaustive = w.nn_ahead < 0;
  const int win_w = w.nn_back + w.nn_ahead + 1;
  int j_prev = 0;
  for (int i = 0; i < n; ++i) {
    [[maybe_unused]] RoadRow<float> rr;   // (the road table: the row of the last step's waypoint, loaded like the scales)
    if constexpr (kRoadPack<TM...>) rr = road_row<float>(p, n, j_prev, tm...);
    [[maybe_unused]] SurfaceScales<float> ms;   // (the surface table: j_prev is uniform, a scalar load)
    if constexpr (kSurfacePack<TM...>) ms = surface_scales<float>(p, n, j_prev, tm...);
    const float d = su[2 * i], q = su[2 * i + 1];
    float dx = d, qx = q;   // (what the step is driven on: the command, or what the actuator lag makes of it)
    if constexpr (kActuatorPack<TM...>) actuator_step<float>(i, d, q, as, lag_of(tm...), dx, qx);
    if constexpr (kRoadPack<TM...>) dynamic_advance_fine<float, RoadPeaks<float>>(st, dx, qx, veh, g, g.inv_L[k], road_peaks<float>(aero_peaks(k, tm...), veh, rr));
    else if constexpr (kSurfacePack<TM...>) dynamic_advance_fine<float, AeroPeaks<SurfacePeaks<float>>>(st, dx, qx, veh, g, g.inv_L[k], surface_peaks<float>(aero_peaks(k, tm...), veh, ms));
    else if constexpr (kAeroPack<TM...>) dynamic_advance_fine<float, AeroPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], aero_peaks(k, tm...));
    else if constexpr (kLoadedPack<TM...>) dynamic_advance_fine<float, LoadedPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], loaded_peaks(k, tm...));
    else if constexpr (kCoupledPack<TM...>) dynamic_advance_fine<float, CoupledPeaks<VehiclePeaks>>(st, dx, qx, veh, g, g.inv_L[k], coupled_peaks(tm...));
    else dynamic_control_step<FINE, float>(st, dx, qx, veh, w.dt, g, g.inv_L[k]);
    // finalize_dynamic_kernel's search, within this wave
    const int lo = exhaustive ? 0 : max(min(j_prev - w.nn_back, n - win_w), 0);
    const int hi = exhaustive ? n - 1 : min(lo + win_w, n) - 1;
    float best = __builtin_inff();
    int j = 0x7fffffff;
    for (int m = lo + lane; m <= hi; m += kWave) {
      const float ek = search_key<float>(st.t.X, st.t.Y, s_abc[kKeyStride * m], s_abc[kKeyStride * m + kKeyB],
                                         s_abc[kKeyStride * m + kKeyC]);
      if (ek < best) {
        best = ek;
        j = m;
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
    if constexpr (kTerms) dynamic_terms<float>(st, d, q, i, p, veh, s_wp, j, ts, tm...);
    if (writer) {
      sx[3 * (i + 1)] = st.t.X + coef[0];
      sx[3 * (i + 1) + 1] = st.t.Y + coef[1];
      sx[3 * (i + 1) + 2] = st.t.phi;
    }
  }
  if (lane == 0) {
    if constexpr (kTerms) s_ck[k] = finish_dynamic_terms<float>(st, ts, s_wp, j_prev, p, n, w, tm...);
    else s_ck[k] = finish_temporal<float>(st.t, n, w);
    s_ck[kMaxVehicles + k] = st.t.V;
  }
  __syncthreads();
  if (tid == 0) {
    float J, V;
    ensemble_combine(s_ck, s_ck + kMaxVehicles, 1, e, J, V);
    s_rec[0] = J;
    s_rec[1] = V;
    s_rec[2] = static_cast<float>(nfeas);
    s_rec[3] = 1.0f;
  }
  __syncthreads();
  for (int q = tid; q < rec_floats; q += threads) rec[q] = s_rec[q];
}

// a run-time choice between two instantiations: body(std::true_type{}) or body(std::false_type{})
template <typename Body>
hipError_t with_choice(bool on, Body&& body) {
  return on ? body(std::true_type{}) : body(std::false_type{});
}

// FINE = true for any integration setting but the default (acmpc_dynamic.h: Integration) and, whatever the setting, for
// the kernels with the terms (GENERAL: they have no FINE = false form); FINE = false for the default setting
template <bool GENERAL, typename Body>
hipError_t with_integration_kind(const Integration& g, Body&& body) {
  if constexpr (GENERAL) return body(std::true_type{});
  else return with_choice(is_fine(g), body);
}

bool integration_valid(const Integration& g) { return g.substeps >= 1 && g.substeps <= kMaxSubsteps; }

// The three launchers, written once: `tm` is nothing (the kernels without the terms, acmpc_dynamic.hip) or the pack of the
// unit that calls them (the table above).
template <typename... TM>
hipError_t rollout_dynamic_launch(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles, const Integration& g,
                                  hipStream_t s, const TM&... tm) {
  constexpr bool kGeneral = sizeof...(TM) != 0;
  clear_stale_error();
  if (!integration_valid(g)) return hipErrorInvalidValue;
  if (args.n < 1 || args.n > kDynamicMaxSteps || args.N < 1 || args.P < 1) return hipErrorInvalidValue;
  if (vehicles.K < 1 || vehicles.K > kMaxVehicles || (layout != 0 && layout != 1)) return hipErrorInvalidValue;
  const int K = vehicles.K;
  const int cpt = dynamic_candidates_per_lane(args.P, args.N, K);
  const dim3 grid(dynamic_blocks_per_problem(args.P, args.N, K), args.P);
  const size_t tables = static_cast<size_t>(args.n) * (kCoefT + kKeyStride) * sizeof(float);
  const size_t lds = (K == 1 ? 64 : 2 * static_cast<size_t>(K) * kWave * cpt * sizeof(float)) + tables;
  return with_integration_kind<kGeneral>(g, [&](auto fine) {
    return with_choice(layout == 1, [&](auto step_major) {
      return with_choice(cpt == 2, [&](auto two) {
        constexpr int kLayout = decltype(step_major)::value ? 1 : 0, kCpt = decltype(two)::value ? 2 : 1;
        constexpr bool kFine = decltype(fine)::value;
        if (K == 1)
          return launch_kernel(rollout_dynamic_kernel<kLayout, kCpt, kFine, TM...>, grid, dim3(kDynBlock), lds, s, nullptr,
                               nullptr, args, vehicles.v[0], g, tm...);
        return launch_kernel(rollout_dynamic_ensemble_kernel<kLayout, kCpt, kFine, TM...>, grid, dim3(kWave * K), lds, s,
                             nullptr, nullptr, args, vehicles, g, tm...);
      });
    });
  });
}

template <typename... TM>
hipError_t rollout_dynamic_sampled_launch(const RolloutArgs& args, const SampleArgs& sample, const VehicleEnsemble& vehicles,
                                          const Integration& g, hipStream_t s, const TM&... tm) {
  constexpr bool kGeneral = sizeof...(TM) != 0;
  (void)hipGetLastError();
  if (!integration_valid(g)) return hipErrorInvalidValue;
  if (args.n < 1 || args.n > kDynamicMaxSteps || args.N < 1 || args.P < 1) return hipErrorInvalidValue;
  if (vehicles.K < 1 || vehicles.K > kMaxVehicles) return hipErrorInvalidValue;
  if (sample.P != args.P || sample.N != args.N || sample.n != args.n || sample.index_offset != args.index_offset)
    return hipErrorInvalidValue;
  if (sample.centre == nullptr || sample.spec.segments == nullptr || sample.centre_stride < 2 * args.n) return hipErrorInvalidValue;
  if (sample.u_extra != nullptr || sample.prev_keys != nullptr) return hipErrorInvalidValue;   // (mode D has no candidate 2)
  const SampleSpec& sp = sample.spec;
  const float box_s[4] = {sp.ulo0, sp.ulo1, sp.uhi0, sp.uhi1};
  const float box_w[4] = {args.w.ulo0, args.w.ulo1, args.w.uhi0, args.w.uhi1};
  if (std::memcmp(box_s, box_w, sizeof box_s) != 0) return hipErrorInvalidValue;   // the kernels clip to the Weights' box
  DynamicDraw d{};
  d.centre = sample.centre;
  d.u_ref = sample.u_ref;
  d.segments = sp.segments;
  d.seed_ptr = sp.seed_ptr;
  d.centre_stride = sample.centre_stride;
  d.seed_lo = sp.seed_lo;
  d.seed_hi = sp.seed_hi;
  d.round = sp.round;
  d.sigma_d = sp.sigma_v;
  d.sigma_p = sp.sigma_k;
  const int K = vehicles.K;
  const int cpt = dynamic_candidates_per_lane(args.P, args.N, K);
  const dim3 grid(dynamic_blocks_per_problem(args.P, args.N, K), args.P);
  const size_t tables = static_cast<size_t>(args.n) * (kCoefT + kKeyStride + kDrawFloatsPerStep) * sizeof(float);
  const size_t rows = K == 1 ? kDynBlock : kWave;   // lanes that roll different candidates: kDrawSlots pairs of normals each
  const size_t lds = (K == 1 ? 64 : 2 * static_cast<size_t>(K) * kWave * cpt * sizeof(float)) +
                     kDrawSlots * rows * cpt * sizeof(f32x2) + tables;   // K = 1: <= 60 KB
  return with_integration_kind<kGeneral>(g, [&](auto fine) {
    return with_choice(cpt == 2, [&](auto two) {
      constexpr int kCpt = decltype(two)::value ? 2 : 1;
      constexpr bool kFine = decltype(fine)::value;
      if (K == 1)
        return launch_kernel(rollout_dynamic_sampled_kernel<kCpt, kFine, TM...>, grid, dim3(kDynBlock), lds, s, nullptr,
                             nullptr, args, d, vehicles.v[0], g, tm...);
      return launch_kernel(rollout_dynamic_sampled_ensemble_kernel<kCpt, kFine, TM...>, grid, dim3(kWave * K), lds, s,
                           nullptr, nullptr, args, d, vehicles, g, tm...);
    });
  });
}

template <typename... TM>
hipError_t finalize_dynamic_launch(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles, const Integration& g,
                                   hipStream_t s, const TM&... tm) {
  constexpr bool kGeneral = sizeof...(TM) != 0;
  (void)hipGetLastError();
  if (!integration_valid(g)) return hipErrorInvalidValue;
  if (args.controls_only || args.n < 1 || args.n > kDynamicMaxSteps) return hipErrorInvalidValue;
  if (args.regenerate && (args.centre == nullptr || args.spec.segments == nullptr || args.u_extra != nullptr))
    return hipErrorInvalidValue;
  if (vehicles.K < 1 || vehicles.K > kMaxVehicles || (layout != 0 && layout != 1)) return hipErrorInvalidValue;
  const size_t rec_floats = static_cast<size_t>(4 + 2 * args.n + 3 * (args.n + 1));
  const size_t tables = static_cast<size_t>(args.n) * (kCoefT + kKeyStride);
  const size_t rec_pad = (rec_floats + 3) & ~static_cast<size_t>(3);
  const int K = vehicles.K;
  const size_t lds = (rec_pad + (K == 1 ? 0 : 2 * kMaxVehicles) + tables) * sizeof(float);
  return with_integration_kind<kGeneral>(g, [&](auto fine) {
    return with_choice(layout == 1, [&](auto step_major) {
      constexpr int kLayout = decltype(step_major)::value ? 1 : 0;
      constexpr bool kFine = decltype(fine)::value;
      if (K == 1)
        return launch_kernel(finalize_dynamic_kernel<kLayout, kFine, TM...>, dim3(args.P), dim3(kWave), lds, s, nullptr,
                             nullptr, args, vehicles.v[0], g, tm...);
      return launch_kernel(finalize_dynamic_ensemble_kernel<kLayout, kFine, TM...>, dim3(args.P), dim3(kWave * K), lds, s,
                           nullptr, nullptr, args, vehicles, g, tm...);
    });
  });
}

}  // namespace

// ---- the per-unit launchers: what launch_*_dynamic (acmpc_dynamic.hip) hands over to, by the table above ----------------
// acmpc_dynamic_terms.hip: the kernels of a plain Terms unless has_objective(terms), those of a TermsObjective otherwise
hipError_t launch_rollout_dynamic_terms(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                        const Integration& integration, const TermsObjective& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_terms(const RolloutArgs& args, const SampleArgs& sample,
                                                const VehicleEnsemble& vehicles, const Integration& integration,
                                                const TermsObjective& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_terms(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                         const Integration& integration, const TermsObjective& terms, hipStream_t s);
// acmpc_dynamic_coupled.hip: the kernels of a TermsCoupled, whichever term parts are on
hipError_t launch_rollout_dynamic_coupled(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                          const Integration& integration, const TermsCoupled& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_coupled(const RolloutArgs& args, const SampleArgs& sample,
                                                  const VehicleEnsemble& vehicles, const Integration& integration,
                                                  const TermsCoupled& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_coupled(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                           const Integration& integration, const TermsCoupled& terms, hipStream_t s);
// acmpc_dynamic_loaded.hip: the kernels of a TermsLoaded
hipError_t launch_rollout_dynamic_loaded(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                         const Integration& integration, const TermsLoaded& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_loaded(const RolloutArgs& args, const SampleArgs& sample,
                                                 const VehicleEnsemble& vehicles, const Integration& integration,
                                                 const TermsLoaded& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_loaded(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                          const Integration& integration, const TermsLoaded& terms, hipStream_t s);
// acmpc_dynamic_aero.hip: the kernels of a TermsAero
hipError_t launch_rollout_dynamic_aero(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                       const Integration& integration, const TermsAero& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_aero(const RolloutArgs& args, const SampleArgs& sample,
                                               const VehicleEnsemble& vehicles, const Integration& integration,
                                               const TermsAero& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_aero(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                        const Integration& integration, const TermsAero& terms, hipStream_t s);
// acmpc_dynamic_obstacles.hip: the kernels of a WithObstacles over TermsAero, TermsLoaded, TermsCoupled or TermsObjective.
// hipErrorInvalidValue unless 1 <= K <= kMaxObstacles and terms.P / terms.n are the launch's.
hipError_t launch_rollout_dynamic_obstacles(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                            const Integration& integration, const WithObstacles<TermsSurface>& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_obstacles(const RolloutArgs& args, const SampleArgs& sample,
                                                    const VehicleEnsemble& vehicles, const Integration& integration,
                                                    const WithObstacles<TermsSurface>& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_obstacles(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                             const Integration& integration, const WithObstacles<TermsSurface>& terms, hipStream_t s);

// acmpc_dynamic_surface.hip: the kernels of a TermsSurface, or - while obstacles are set - of a WithObstacles<TermsSurface>.
// hipErrorInvalidValue unless terms.mu is set for the launch's P and n (and the obstacles, if any, likewise).
hipError_t launch_rollout_dynamic_surface(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                          const Integration& integration, const WithObstacles<TermsSurface>& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_surface(const RolloutArgs& args, const SampleArgs& sample,
                                                  const VehicleEnsemble& vehicles, const Integration& integration,
                                                  const WithObstacles<TermsSurface>& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_surface(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                           const Integration& integration, const WithObstacles<TermsSurface>& terms, hipStream_t s);

// acmpc_dynamic_actuator.hip: the kernels of a WithActuator over TermsAero or TermsSurface, each with or without the obstacles'
// pack between.  hipErrorInvalidValue unless the actuator positions, the surface table and the obstacles - whichever are set -
// are the launch's P and n.
hipError_t launch_rollout_dynamic_actuator(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                           const Integration& integration, const WithActuator<WithObstacles<TermsSurface>>& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_actuator(const RolloutArgs& args, const SampleArgs& sample,
                                                   const VehicleEnsemble& vehicles, const Integration& integration,
                                                   const WithActuator<WithObstacles<TermsSurface>>& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_actuator(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                            const Integration& integration, const WithActuator<WithObstacles<TermsSurface>>& terms, hipStream_t s);

// acmpc_dynamic_road.hip, acmpc_dynamic_road_actuator.hip: the kernels of a TermsRoad - under the obstacles' pack while obstacles
// are set - and of a WithActuator over either while the actuator lag is on (the second unit, which the first hands over to).
// hipErrorInvalidValue unless the road table, the surface table, the obstacles and the actuator positions - whichever are set -
// are the launch's P and n.
hipError_t launch_rollout_dynamic_road(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                       const Integration& integration, const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_road(const RolloutArgs& args, const SampleArgs& sample,
                                               const VehicleEnsemble& vehicles, const Integration& integration,
                                               const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_road(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                        const Integration& integration, const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_road_actuator(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                                const Integration& integration, const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);
hipError_t launch_rollout_dynamic_sampled_road_actuator(const RolloutArgs& args, const SampleArgs& sample,
                                                        const VehicleEnsemble& vehicles, const Integration& integration,
                                                        const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);
hipError_t launch_finalize_dynamic_road_actuator(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                                 const Integration& integration, const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);
// the shape check the two units share: nothing is launched unless every table the handle has set is what P and n index
inline bool road_valid(const WithActuator<WithObstacles<TermsRoad>>& tm, int P, int n) {
  if (!has_road(tm) || tm.road_rows == nullptr || tm.road_P != P || tm.road_n != n) return false;
  if (has_surface(tm) && (tm.mu == nullptr || tm.mu_P != P || tm.mu_n != n)) return false;
  if (has_actuator(tm) && tm.lag.a0 != nullptr && tm.lag.a0_P != P) return false;
  if (!has_obstacles(tm)) return true;
  return tm.K >= 1 && tm.K <= kMaxObstacles && tm.obs != nullptr && tm.radii != nullptr && tm.P == P && tm.n == n;
}

}  // namespace acmpc
