// gfx950 kernels of mode D's grip identification (acmpc_score_grips; DESIGN.md section 2 "Mode D, grip identification",
// restated by tests/grip_spec.py): K hypothetical vehicles - vehicle 0 with its two axle peaks scaled - rolled over a
// logged window of (vx, vy, r) under the logged (delta, pedal), each scored by its prediction error.
//
//   identify_grip_kernel    ONE LANE PER HYPOTHESIS, the controls wave-uniform (every rollout is the other way round: one
//                           lane per control sequence, the vehicle in SGPRs).  The base Vehicle and the Integration are
//                           kernel arguments (SGPRs); the lane's two peak factors sit in two VGPRs and go into the step
//                           through dynamic_advance_fine's peak source (LanePeaks) - the step is the rollouts', not restated.
//                           blockIdx.y is a run of segments; a segment starts from the LOGGED state and rolls open-loop,
//                           adding the weighted squared residual after every control step.  The log is read at
//                           wave-uniform addresses through const __restrict__ pointers: scalar loads.  Writes e [S][K],
//                           coalesced in k.  The pose of the step (X, Y, yaw and sincos_spec(yaw)) is never read here and
//                           the compiler drops it (DESIGN.md section 4.10 has the check).
//                           identify_grip_coupled_kernel: the same under the handle's tyre coupling (acmpc_dynamic.h:
//                           CoupledPeaks), each lane's caps from its own two peaks; launched only while the coupling is on.
//                           identify_grip_loaded_kernel: the same under the handle's load transfer (LoadedPeaks), the base
//                           vehicle's factors on each lane's own peaks; launched only while the load transfer is on.
//                           identify_grip_aero_kernel: the same under the handle's downforce (AeroPeaks); launched only
//                           while the downforce is on.
//   identify_sum_kernel     one lane per hypothesis adds its S segment values IN ORDER (plain float32 adds: the
//                           association is the specification's), writes errors [K], and the workgroup leaves one partial
//                           (E, k) key - the rollouts' reduction: DPP inside the wave, LDS across the waves.
//   identify_best_kernel    one wavefront takes the minimum of the <= 256 partial keys.
//
// Three plain launches ordered by the stream: nothing crosses workgroups inside a launch, every store is a vector store.
// Lanes past K repeat hypothesis K - 1 and report nothing (the rollouts' tail rule): no lane leaves a loop early.
//
// Built with -ffp-contract=off: see acmpc_device.h.
#include "acmpc_identify.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "acmpc kernels are written for gfx950 (MI355X)"
#endif

namespace acmpc {

namespace {

constexpr int kIdBlock = 256;

__global__ void __launch_bounds__(kIdBlock)
    identify_grip_kernel(const float* __restrict__ states, const float* __restrict__ controls,
                         const f32x2* __restrict__ peaks, float* __restrict__ e_out, const int W, const int L, const int S,
                         const int K, const int run, const float w0, const float w1, const float w2, const Vehicle veh,
                         const Integration g) {
  const int k_own = static_cast<int>(blockIdx.x) * kIdBlock + static_cast<int>(threadIdx.x);
  const int k = min(k_own, K - 1);
  const f32x2 pk = peaks[k];
  const LanePeaks lane_peaks{pk[0], pk[1]};
  const int s_first = static_cast<int>(blockIdx.y) * run;
  const int s_last = min(s_first + run, S);
  for (int seg = s_first; seg < s_last; ++seg) {
    const int j_first = seg * L;
    const int j_last = min(j_first + L, W);
    StateD st{};   // (the pose starts at 0 and is never read)
    st.vx = states[3 * j_first];
    st.vy = states[3 * j_first + 1];
    st.r = states[3 * j_first + 2];
    float e = 0.0f;
    for (int j = j_first; j < j_last; ++j) {
      const float d = controls[2 * j], q = controls[2 * j + 1];
      dynamic_advance_fine<float, LanePeaks>(st, d, q, veh, g, g.inv_L[0], lane_peaks);
      const float dvx = st.vx - states[3 * (j + 1)];
      const float dvy = st.vy - states[3 * (j + 1) + 1];
      const float dr = st.r - states[3 * (j + 1) + 2];
      e = fma_(w0 * dvx, dvx, e);
      e = fma_(w1 * dvy, dvy, e);
      e = fma_(w2 * dr, dr, e);
    }
    if (k_own < K) e_out[static_cast<size_t>(seg) * K + k_own] = e;
  }
}

// identify_grip_kernel under the handle's tyre coupling (rho_f, rho_r): the lane's peak source carries the two ratios, and
// its caps are its own peaks times them.  Launched only while the coupling is on.  The same lines but for the source: a body
// shared between the two kernels changes the other's register allocation, and that kernel stays the code it was.
__global__ void __launch_bounds__(kIdBlock)
    identify_grip_coupled_kernel(const float* __restrict__ states, const float* __restrict__ controls,
                                 const f32x2* __restrict__ peaks, float* __restrict__ e_out, const int W, const int L,
                                 const int S, const int K, const int run, const float w0, const float w1, const float w2,
                                 const Vehicle veh, const Integration g, const float rho_f, const float rho_r) {
  const int k_own = static_cast<int>(blockIdx.x) * kIdBlock + static_cast<int>(threadIdx.x);
  const int k = min(k_own, K - 1);
  const f32x2 pk = peaks[k];
  const CoupledPeaks<LanePeaks> lane_peaks{{pk[0], pk[1]}, rho_f, rho_r};
  const int s_first = static_cast<int>(blockIdx.y) * run;
  const int s_last = min(s_first + run, S);
  for (int seg = s_first; seg < s_last; ++seg) {
    const int j_first = seg * L;
    const int j_last = min(j_first + L, W);
    StateD st{};
    st.vx = states[3 * j_first];
    st.vy = states[3 * j_first + 1];
    st.r = states[3 * j_first + 2];
    float e = 0.0f;
    for (int j = j_first; j < j_last; ++j) {
      const float d = controls[2 * j], q = controls[2 * j + 1];
      dynamic_advance_fine<float, CoupledPeaks<LanePeaks>>(st, d, q, veh, g, g.inv_L[0], lane_peaks);
      const float dvx = st.vx - states[3 * (j + 1)];
      const float dvy = st.vy - states[3 * (j + 1) + 1];
      const float dr = st.r - states[3 * (j + 1) + 2];
      e = fma_(w0 * dvx, dvx, e);
      e = fma_(w1 * dvy, dvy, e);
      e = fma_(w2 * dr, dr, e);
    }
    if (k_own < K) e_out[static_cast<size_t>(seg) * K + k_own] = e;
  }
}

// identify_grip_coupled_kernel under the handle's load transfer as well (acmpc_dynamic.h: LoadedPeaks): the base vehicle's six
// scalars applied to each lane's own pair of peaks - the factor phi does not depend on a grip scale - and the ratios +inf while
// the coupling is off.  Launched only while the load transfer is on.  The same lines again, for the same reason.
__global__ void __launch_bounds__(kIdBlock)
    identify_grip_loaded_kernel(const float* __restrict__ states, const float* __restrict__ controls,
                                const f32x2* __restrict__ peaks, float* __restrict__ e_out, const int W, const int L,
                                const int S, const int K, const int run, const float w0, const float w1, const float w2,
                                const Vehicle veh, const Integration g, const float rho_f, const float rho_r,
                                const IdentifyLoad ld) {
  const int k_own = static_cast<int>(blockIdx.x) * kIdBlock + static_cast<int>(threadIdx.x);
  const int k = min(k_own, K - 1);
  const f32x2 pk = peaks[k];
  const LoadedPeaks<LanePeaks> lane_peaks{{{pk[0], pk[1]}, rho_f, rho_r}, ld.c_h, ld.w_max, ld.a1_f, ld.a2_f, ld.a1_r, ld.a2_r};
  const int s_first = static_cast<int>(blockIdx.y) * run;
  const int s_last = min(s_first + run, S);
  for (int seg = s_first; seg < s_last; ++seg) {
    const int j_first = seg * L;
    const int j_last = min(j_first + L, W);
    StateD st{};
    st.vx = states[3 * j_first];
    st.vy = states[3 * j_first + 1];
    st.r = states[3 * j_first + 2];
    float e = 0.0f;
    for (int j = j_first; j < j_last; ++j) {
      const float d = controls[2 * j], q = controls[2 * j + 1];
      dynamic_advance_fine<float, LoadedPeaks<LanePeaks>>(st, d, q, veh, g, g.inv_L[0], lane_peaks);
      const float dvx = st.vx - states[3 * (j + 1)];
      const float dvy = st.vy - states[3 * (j + 1) + 1];
      const float dr = st.r - states[3 * (j + 1) + 2];
      e = fma_(w0 * dvx, dvx, e);
      e = fma_(w1 * dvy, dvy, e);
      e = fma_(w2 * dr, dr, e);
    }
    if (k_own < K) e_out[static_cast<size_t>(seg) * K + k_own] = e;
  }
}

// identify_grip_loaded_kernel under the handle's downforce as well (acmpc_dynamic.h: AeroPeaks): the handle's (k_f, k_r, v_sat)
// and the base vehicle's six scalars (c_h = w_max = 0 while the load transfer is off) applied to each lane's own pair of peaks -
// D cancels in psi and phi, so neither depends on a grip scale.  Launched only while the downforce is on.  The same lines again.
__global__ void __launch_bounds__(kIdBlock)
    identify_grip_aero_kernel(const float* __restrict__ states, const float* __restrict__ controls,
                              const f32x2* __restrict__ peaks, float* __restrict__ e_out, const int W, const int L,
                              const int S, const int K, const int run, const float w0, const float w1, const float w2,
                              const Vehicle veh, const Integration g, const float rho_f, const float rho_r,
                              const IdentifyLoad ld, const IdentifyAero ae) {
  const int k_own = static_cast<int>(blockIdx.x) * kIdBlock + static_cast<int>(threadIdx.x);
  const int k = min(k_own, K - 1);
  const f32x2 pk = peaks[k];
  const AeroPeaks<LanePeaks> lane_peaks{{{{pk[0], pk[1]}, rho_f, rho_r}, ld.c_h, ld.w_max, ld.a1_f, ld.a2_f, ld.a1_r, ld.a2_r},
                                        ae.k_f, ae.k_r, ae.v_sat};
  const int s_first = static_cast<int>(blockIdx.y) * run;
  const int s_last = min(s_first + run, S);
  for (int seg = s_first; seg < s_last; ++seg) {
    const int j_first = seg * L;
    const int j_last = min(j_first + L, W);
    StateD st{};
    st.vx = states[3 * j_first];
    st.vy = states[3 * j_first + 1];
    st.r = states[3 * j_first + 2];
    float e = 0.0f;
    for (int j = j_first; j < j_last; ++j) {
      const float d = controls[2 * j], q = controls[2 * j + 1];
      dynamic_advance_fine<float, AeroPeaks<LanePeaks>>(st, d, q, veh, g, g.inv_L[0], lane_peaks);
      const float dvx = st.vx - states[3 * (j + 1)];
      const float dvy = st.vy - states[3 * (j + 1) + 1];
      const float dr = st.r - states[3 * (j + 1) + 2];
      e = fma_(w0 * dvx, dvx, e);
      e = fma_(w1 * dvy, dvy, e);
      e = fma_(w2 * dr, dr, e);
    }
    if (k_own < K) e_out[static_cast<size_t>(seg) * K + k_own] = e;
  }
}

__global__ void __launch_bounds__(kIdBlock)
    identify_sum_kernel(const float* __restrict__ e_in, float* __restrict__ errors, int64_t* __restrict__ partial_keys,
                        const int S, const int K) {
  __shared__ int64_t s_key[kIdBlock / kWave];
  const int tid = static_cast<int>(threadIdx.x);
  const int k_own = static_cast<int>(blockIdx.x) * kIdBlock + tid;
  const int k = min(k_own, K - 1);
  float E = e_in[k];
  for (int s = 1; s < S; ++s) E = E + e_in[static_cast<size_t>(s) * K + k];
  int64_t key = kKeyMax;
  if (k_own < K) {
    errors[k_own] = E;
    key = pack_key(E, static_cast<uint32_t>(k_own));
  }
  key = wave_min_key(key);
  constexpr int kWaves = kIdBlock / kWave;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int q = 1; q < kWaves; ++q) key = (s_key[q] < key) ? s_key[q] : key;
    partial_keys[blockIdx.x] = key;
  }
}

__global__ void __launch_bounds__(kWave)
    identify_best_kernel(const int64_t* __restrict__ partial_keys, const int blocks, int64_t* __restrict__ best) {
  const int lane = static_cast<int>(threadIdx.x);
  int64_t key = kKeyMax;
  for (int b = lane; b < blocks; b += kWave) {
    const int64_t kb = partial_keys[b];
    key = (kb < key) ? kb : key;
  }
  key = wave_min_key(key);
  if (lane == 0) *best = key;
}

}  // namespace

int identify_segments(int W, int L) { return (W + L - 1) / L; }

int identify_blocks(int K) { return (K + kIdBlock - 1) / kIdBlock; }

// a run of segments per workgroup once the grid would be thousands of one-segment workgroups: about 2 048 in all
IdentifyGrid identify_grid(int S, int K) {
  IdentifyGrid g{};
  g.blocks = identify_blocks(K);   // <= 256
  g.rows = std::min(S, std::max(1, 2048 / g.blocks));
  g.run = (S + g.rows - 1) / g.rows;
  g.grid_y = (S + g.run - 1) / g.run;
  return g;
}

hipError_t launch_identify_grip(const IdentifyArgs& a, const Vehicle& vehicle, const Integration& g, const float* coupling,
                                const IdentifyLoad* load, const IdentifyAero* aero, hipStream_t s) {
  (void)hipGetLastError();
  if (g.substeps < 1 || g.substeps > kMaxSubsteps) return hipErrorInvalidValue;
  if (a.W < 1 || a.W > kIdentifyMaxSteps || a.L < 1 || a.L > a.W || a.K < 1 || a.K > kIdentifyMaxHypotheses)
    return hipErrorInvalidValue;
  const int S = identify_segments(a.W, a.L);
  if (static_cast<int64_t>(S) * a.K > kIdentifyMaxValues) return hipErrorInvalidValue;
  if (a.states == nullptr || a.controls == nullptr || a.peaks == nullptr || a.e == nullptr || a.errors == nullptr ||
      a.partial_keys == nullptr || a.best == nullptr)
    return hipErrorInvalidValue;
  const IdentifyGrid shape = identify_grid(S, a.K);
  const int blocks = shape.blocks, run = shape.run;
  const dim3 grid(blocks, shape.grid_y);
  if (aero != nullptr) {
    if (load == nullptr) return hipErrorInvalidValue;   // (the factors a1, a2 travel with the load transfer's scalars)
    hipLaunchKernelGGL(identify_grip_aero_kernel, grid, dim3(kIdBlock), 0, s, a.states, a.controls,
                       reinterpret_cast<const f32x2*>(a.peaks), a.e, a.W, a.L, S, a.K, run, a.w[0], a.w[1], a.w[2], vehicle, g,
                       coupling != nullptr ? coupling[0] : __builtin_huge_valf(), coupling != nullptr ? coupling[1] : __builtin_huge_valf(),
                       *load, *aero);
  } else if (load != nullptr) {
    hipLaunchKernelGGL(identify_grip_loaded_kernel, grid, dim3(kIdBlock), 0, s, a.states, a.controls,
                       reinterpret_cast<const f32x2*>(a.peaks), a.e, a.W, a.L, S, a.K, run, a.w[0], a.w[1], a.w[2], vehicle, g,
                       coupling != nullptr ? coupling[0] : __builtin_huge_valf(), coupling != nullptr ? coupling[1] : __builtin_huge_valf(),
                       *load);
  } else if (coupling != nullptr) {
    hipLaunchKernelGGL(identify_grip_coupled_kernel, grid, dim3(kIdBlock), 0, s, a.states, a.controls,
                       reinterpret_cast<const f32x2*>(a.peaks), a.e, a.W, a.L, S, a.K, run, a.w[0], a.w[1], a.w[2], vehicle, g,
                       coupling[0], coupling[1]);
  } else {
    hipLaunchKernelGGL(identify_grip_kernel, grid, dim3(kIdBlock), 0, s, a.states, a.controls,
                       reinterpret_cast<const f32x2*>(a.peaks), a.e, a.W, a.L, S, a.K, run, a.w[0], a.w[1], a.w[2], vehicle, g);
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(identify_sum_kernel, dim3(blocks), dim3(kIdBlock), 0, s, a.e, a.errors, a.partial_keys, S, a.K);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(identify_best_kernel, dim3(1), dim3(kWave), 0, s, a.partial_keys, blocks, a.best);
  return hipGetLastError();
}

}  // namespace acmpc
