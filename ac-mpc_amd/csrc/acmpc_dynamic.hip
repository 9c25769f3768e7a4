// gfx950 kernels of mode D (the dynamic bicycle, acmpc_dynamic.h): a rollout that scores every candidate and a finalize
// that re-rolls the winner into the standard record.  Two plain launches ordered by the stream: nothing crosses
// workgroups inside a launch, every store is a vector store.
//
//   rollout_dynamic_kernel   256 lanes per workgroup, one or two candidates per lane (CPT; two = f32x2, v_pk_*
//                            instructions).  The waypoint rows and the search keys are staged in LDS once per workgroup
//                            (stage_dynamic_tables); the vehicle's constants are a kernel argument (SGPRs).  Each workgroup
//                            writes its candidates' costs and ONE partial (cost, index) key + feasible count.
//   finalize_dynamic_kernel  one wavefront per problem: argmin over the partial keys, then the winner's trajectory on
//                            broadcast operands with the lanes scanning the waypoints side by side for the search.
//
// An ensemble of K > 1 vehicles (VehicleEnsemble, acmpc_dynamic.h) runs two kernels of its own, with ONE WAVEFRONT PER
// VEHICLE: wave k's vehicle index is wave-uniform, so its constants are scalar as one vehicle's are and the step loop is
// the one above.
//   rollout_dynamic_ensemble_kernel   K waves per workgroup over the same 64 CPT candidates; the tables are staged once
//                                     for the K waves; each wave leaves its (c_k, V_k) in LDS, and after one barrier
//                                     wave 0 combines them in k order into the costs, the partial key and the count.
//   finalize_dynamic_ensemble_kernel  K waves per problem: wave k re-rolls the winner under vehicle k (one re-roll of
//                                     latency, not K); the K results are combined as in the rollout; wave 0's
//                                     trajectory is the record's x.
//
// Built with -ffp-contract=off: see acmpc_device.h.
#include "acmpc_dynamic.h"

#include <type_traits>

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "acmpc kernels are written for gfx950 (MI355X)"
#endif

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

template <int LAYOUT, int CPT>
__global__ void __launch_bounds__(kDynBlock) rollout_dynamic_kernel(const RolloutArgs a, const Vehicle veh) {
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
  I nearest = I(0);
  with_search_kind(w, n, [&](auto kind) {
    constexpr int kKind = (decltype(kind)::value == kSearchVerified) ? kSearchExhaustive : decltype(kind)::value;
    for (int i = 0; i < n; ++i) {
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
      dynamic_advance<F>(st, d, q, veh, w.dt);
      nearest = dynamic_nearest<kKind>(st.t.X, st.t.Y, s_xy, n, w, nearest);
      dynamic_settle(st, s_wp, nearest, d, q, w);
    }
  });
  const F cost_v = finish_temporal<F>(st.t, n, w);
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

template <int LAYOUT>
__global__ void __launch_bounds__(kWave) finalize_dynamic_kernel(const FinalizeArgs a, const Vehicle veh) {
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
  if (!(local >= 0 && local < a.N)) {   // the winner lives on another rank (or nothing was found): a blank record
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
  for (int i = lane; i < n; i += kWave) load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, c, su[2 * i], su[2 * i + 1]);
  StateD st = start_dynamic<float>(x0, coef);
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
    const float d = su[2 * i], q = su[2 * i + 1];   // (LDS broadcast: every lane rolls the same state)
    dynamic_advance<float>(st, d, q, veh, w.dt);
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
    if (lane == 0) {
      sx[3 * (i + 1)] = st.t.X + coef[0];
      sx[3 * (i + 1) + 1] = st.t.Y + coef[1];
      sx[3 * (i + 1) + 2] = st.t.phi;
    }
  }
  if (lane == 0) {
    s_rec[0] = finish_temporal<float>(st.t, n, w);
    s_rec[1] = st.t.V;
    s_rec[2] = static_cast<float>(nfeas);
    s_rec[3] = 1.0f;
  }
  __syncthreads();
  for (int e = lane; e < rec_floats; e += kWave) rec[e] = s_rec[e];
}

template <int LAYOUT, int CPT>
__global__ void __launch_bounds__(kWave * kMaxVehicles)
    rollout_dynamic_ensemble_kernel(const RolloutArgs a, const VehicleEnsemble e) {
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
  I nearest = I(0);
  with_search_kind(w, n, [&](auto kind) {
    constexpr int kKind = (decltype(kind)::value == kSearchVerified) ? kSearchExhaustive : decltype(kind)::value;
    for (int i = 0; i < n; ++i) {
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
      dynamic_advance<F>(st, d, q, veh, w.dt);
      nearest = dynamic_nearest<kKind>(st.t.X, st.t.Y, s_xy, n, w, nearest);
      dynamic_settle(st, s_wp, nearest, d, q, w);
    }
  });
  const F cost_v = finish_temporal<F>(st.t, n, w);
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

template <int LAYOUT>
__global__ void __launch_bounds__(kWave * kMaxVehicles)
    finalize_dynamic_ensemble_kernel(const FinalizeArgs a, const VehicleEnsemble e) {
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
  if (!(local >= 0 && local < a.N)) {   // the winner lives on another rank (or nothing was found): a blank record
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
  for (int i = tid; i < n; i += threads) load_dynamic_control<LAYOUT>(a.U, p, a.N, n, i, c, su[2 * i], su[2 * i + 1]);
  StateD st = start_dynamic<float>(x0, coef);
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
    const float d = su[2 * i], q = su[2 * i + 1];
    dynamic_advance<float>(st, d, q, veh, w.dt);
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
    if (writer) {
      sx[3 * (i + 1)] = st.t.X + coef[0];
      sx[3 * (i + 1) + 1] = st.t.Y + coef[1];
      sx[3 * (i + 1) + 2] = st.t.phi;
    }
  }
  if (lane == 0) {
    s_ck[k] = finish_temporal<float>(st.t, n, w);
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

}  // namespace

int dynamic_candidates_per_lane(int P, int N, int K) {
  // 256 CUs x 4 SIMDs x 8 waves x 64 lanes = 524 288 lanes: two candidates per lane once every lane would get two
  // (an ensemble's lanes are P N K: one per vehicle and candidate)
  return (static_cast<int64_t>(P) * N * K >= (int64_t{1} << 20)) ? 2 : 1;
}

int dynamic_blocks_per_problem(int P, int N, int K) {
  const int per_block = (K > 1 ? kWave : kDynBlock) * dynamic_candidates_per_lane(P, N, K);
  return (N + per_block - 1) / per_block;
}

hipError_t launch_rollout_dynamic(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles, hipStream_t s) {
  (void)hipGetLastError();
  if (args.n < 1 || args.n > kDynamicMaxSteps || args.N < 1 || args.P < 1) return hipErrorInvalidValue;
  if (vehicles.K < 1 || vehicles.K > kMaxVehicles || (layout != 0 && layout != 1)) return hipErrorInvalidValue;
  const int K = vehicles.K;
  const int cpt = dynamic_candidates_per_lane(args.P, args.N, K);
  const dim3 grid(dynamic_blocks_per_problem(args.P, args.N, K), args.P);
  const size_t tables = static_cast<size_t>(args.n) * (kCoefT + kKeyStride) * sizeof(float);
  if (K == 1) {
    const Vehicle& vehicle = vehicles.v[0];
    const dim3 block(kDynBlock);
    const size_t lds = 64 + tables;
    if (layout == 0) {
      if (cpt == 2) hipLaunchKernelGGL((rollout_dynamic_kernel<0, 2>), grid, block, lds, s, args, vehicle);
      else hipLaunchKernelGGL((rollout_dynamic_kernel<0, 1>), grid, block, lds, s, args, vehicle);
    } else {
      if (cpt == 2) hipLaunchKernelGGL((rollout_dynamic_kernel<1, 2>), grid, block, lds, s, args, vehicle);
      else hipLaunchKernelGGL((rollout_dynamic_kernel<1, 1>), grid, block, lds, s, args, vehicle);
    }
    return hipGetLastError();
  }
  const dim3 block(kWave * K);
  const size_t lds = 2 * static_cast<size_t>(K) * kWave * cpt * sizeof(float) + tables;
  if (layout == 0) {
    if (cpt == 2) hipLaunchKernelGGL((rollout_dynamic_ensemble_kernel<0, 2>), grid, block, lds, s, args, vehicles);
    else hipLaunchKernelGGL((rollout_dynamic_ensemble_kernel<0, 1>), grid, block, lds, s, args, vehicles);
  } else {
    if (cpt == 2) hipLaunchKernelGGL((rollout_dynamic_ensemble_kernel<1, 2>), grid, block, lds, s, args, vehicles);
    else hipLaunchKernelGGL((rollout_dynamic_ensemble_kernel<1, 1>), grid, block, lds, s, args, vehicles);
  }
  return hipGetLastError();
}

hipError_t launch_finalize_dynamic(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles, hipStream_t s) {
  (void)hipGetLastError();
  if (args.regenerate || args.controls_only || args.n < 1 || args.n > kDynamicMaxSteps) return hipErrorInvalidValue;
  if (vehicles.K < 1 || vehicles.K > kMaxVehicles || (layout != 0 && layout != 1)) return hipErrorInvalidValue;
  const size_t rec_floats = static_cast<size_t>(4 + 2 * args.n + 3 * (args.n + 1));
  const size_t tables = static_cast<size_t>(args.n) * (kCoefT + kKeyStride);
  const size_t rec_pad = (rec_floats + 3) & ~static_cast<size_t>(3);
  if (vehicles.K == 1) {
    const Vehicle& vehicle = vehicles.v[0];
    const size_t lds = (rec_pad + tables) * sizeof(float);
    if (layout == 0) hipLaunchKernelGGL((finalize_dynamic_kernel<0>), dim3(args.P), dim3(kWave), lds, s, args, vehicle);
    else hipLaunchKernelGGL((finalize_dynamic_kernel<1>), dim3(args.P), dim3(kWave), lds, s, args, vehicle);
    return hipGetLastError();
  }
  const size_t lds = (rec_pad + 2 * kMaxVehicles + tables) * sizeof(float);
  const dim3 block(kWave * vehicles.K);
  if (layout == 0) hipLaunchKernelGGL((finalize_dynamic_ensemble_kernel<0>), dim3(args.P), block, lds, s, args, vehicles);
  else hipLaunchKernelGGL((finalize_dynamic_ensemble_kernel<1>), dim3(args.P), block, lds, s, args, vehicles);
  return hipGetLastError();
}

}  // namespace acmpc
