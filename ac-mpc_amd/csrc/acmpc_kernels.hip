// gfx950 kernels of the ac-mpc rollout-and-cost path that share the finalize's device code:
//
//   finalize_kernel  one wave per problem: min over the partial keys (or takes all-reduced keys), re-rolls the
//                    winning candidate and writes its record [cost, violation, n_feasible, owner, u, x]; its batched
//                    forms; sample_kernel; the tailed and chained rollouts; the four forms of a sampled round.
//
// They stay ONE unit: a unit's device code is optimised as a whole before anything is inlined, and where every caller of
// finalize_problem<MODE, 1> in a unit passes the same constant (the LDS array of a unit with finalize_kernel alone) it is
// propagated into the function and the kernel's instructions change (tools/asm_same.py shows it).  The rollouts over a
// control matrix are in acmpc_rollout.hip and acmpc_kernels_temporal.hip, the one-launch solve in acmpc_solo.hip, softmin_*
// in acmpc_softmin.hip.
#include "acmpc_rollout.h"

namespace acmpc {

namespace {

// ---- candidate sampling ------------------------------------------------------------------------------------
// U_c = clip(centre + a_c * sigma * (smooth noise)), one lane per candidate.  The noise is a raised-cosine blend of
// kSampleKnots x 2 standard normals per candidate (smooth along the horizon), a_c cycles through 8 amplitude
// levels, candidate 0 is the centre itself (so a round can never lose the incumbent) and candidate 1 the reference
// controls.  Philox counters are (global candidate, problem, round, draw): reproducible on any rank.
template <int LAYOUT>
__global__ void __launch_bounds__(256) sample_kernel(const SampleArgs a) {
  const int p = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int n = a.n;
  const SampleSpec sp = a.spec;
  const uint32_t gidx = static_cast<uint32_t>(a.index_offset + c);
  float z[kKnots][2];
  draw_normals(sp, gidx, static_cast<uint32_t>(p), z);
  // candidate 1 = the reference controls, candidate 2 = `u_extra` (the LQ plan), each when given: amplitude 0, own centre
  const float* alt = (gidx == 1u) ? a.u_ref : (gidx == 2u) ? a.u_extra : nullptr;
  const bool use_ref = alt != nullptr;
  const float amp = use_ref ? 0.0f : candidate_amplitude(gidx);
  const float* __restrict__ centre =
      use_ref ? alt + static_cast<size_t>(p) * n * 2 : a.centre + static_cast<size_t>(p) * a.centre_stride;
  // blend weights and the centre sequence -> LDS once per workgroup; the knot boundaries are kernel arguments, so
  // neither the loop bounds nor the per-step operands wait on a dependent scalar/global load (those dependencies used
  // to make this the longest kernel of an optimisation round)
  extern __shared__ __attribute__((aligned(16))) float s_smp[];  // [n] weights, then [n][2] centre
  float* s_w0 = s_smp;
  float* s_centre = s_smp + ((n + 3) & ~3);
  for (int e = threadIdx.x; e < n; e += 256) s_w0[e] = sp.segments[2 * e + 1];
  // candidate 1 of a workgroup that holds it reads u_ref instead; every other lane the centre
  const float* __restrict__ block_centre = a.centre + static_cast<size_t>(p) * a.centre_stride;
  for (int e = threadIdx.x; e < 2 * n; e += 256) s_centre[e] = block_centre[e];
  __syncthreads();
  if (c >= a.N) return;
#pragma unroll
  for (int knot = 0; knot < kKnots - 1; ++knot) {
    for (int i = sp.knot_begin[knot]; i < sp.knot_begin[knot + 1]; ++i) {
      float v, k;
      const float cv = use_ref ? centre[2 * i] : s_centre[2 * i];
      const float ck = use_ref ? centre[2 * i + 1] : s_centre[2 * i + 1];
      blend_control(sp, amp, s_w0[i], cv, ck, z[knot][0], z[knot][1], z[knot + 1][0], z[knot + 1][1], v, k);
      if constexpr (LAYOUT == 1) {
        float* row = a.U + (static_cast<size_t>(p) * n + i) * 2 * static_cast<size_t>(a.N) + c;
        row[0] = v;
        row[a.N] = k;
      } else {
        f32x2 vk;
        vk[0] = v;
        vk[1] = k;
        *reinterpret_cast<f32x2*>(a.U + ((static_cast<size_t>(p) * a.N + c) * n + i) * 2) = vk;
      }
    }
  }
}

// sample_kernel and rollout_kernel fused for the latency-bound closed-loop solve: one lane = one candidate whose
// controls are drawn (same Philox counters, same blend_control arithmetic: bit-identical to sample_kernel) and
// consumed step by step without ever being written to memory.  Output: the per-workgroup partial keys, as usual.
// One wave per workgroup and one workgroup per CU at the closed-loop size (16 384 candidates), so nothing hides a
// wait: what the kernel does about each is said where it is done (operands through LDS, requests before the draws).
//
// `traced`: every lane also leaves what it computed - controls and state of each step, violation, cost - in its column
// of an LDS block [5n + 2][64] at `trace_lds_floats`, and the workgroup copies the column of its best candidate to
// `trace_out` (global, [5n + 2]): the fused finalize then assembles the winner's record out of the winning workgroup's
// trace instead of drawing and rolling that candidate a second time, and a following round finds its centre there.
// Rows: 2i, 2i + 1 = (v, kappa) of step i | 2n + 3i .. + 2 = state after step i | 5n = V | 5n + 1 = cost.
// (The trace is addressed off `s_fused` itself, not through a pointer that may be null: a select of pointers would lose
// the LDS address space.)
constexpr int kStagedSteps = 128;   // steps whose uniform operands travel through registers (longer horizons: the rest by a loop)
constexpr int kStagedPairs = (kStagedSteps + kWave - 1) / kWave;   // (v, kappa) pairs per lane

// ---- what the four forms of a sampled round share -----------------------------------------------------------
// The forms (one wave below; two, four and three waves further down) differ in how a step is shared out over waves.  The
// control side of it is one thing in all of them: StagedControls brings the wave-uniform control operands into LDS,
// CandidateControls reads them back per lane and blends, publish_traced_round ends a traced round.  The two-, four- and
// three-wave forms use all three.  The single-wave body keeps its own lines for the same rules: with the helpers its traced
// round at n = 118 measured 29.36 us against the parent's 28.72, outside the parent's 0.32 us spread (LABNOTES).

// Centre, reference, candidate 2's controls and knot weights of every step on their way into LDS, by the lanes of ONE wave,
// in phases that the wave interleaves with its Philox draws: a request's round trip to memory is what the draws that follow
// it cover, so the requests precede the draws.
struct StagedControls {
  const float* centre;
  const float* ref;           // null: no reference controls (the centre stands in for them)
  const float* extra;         // null: this launch holds no candidate 2
  const float* knot_weight;   // (knot, weight) pairs: the weight is [1]
  bool chained;               // wave-uniform: the centre is the previous launch's winner
  f32x2 g_centre[kStagedPairs], g_ref[kStagedPairs], g_extra[kStagedPairs], g_weight[kStagedPairs];
  int64_t prev_key[kChainBlocks / kWave];

  // the loads that depend on nothing: the first kStagedSteps steps' operands, clamped at the last step, and - chained - the
  // previous launch's partial keys, four per lane
  __device__ __forceinline__ void request(const RolloutArgs& a, const SampleArgs& smp, const int p, const int lane, const int n) {
    centre = smp.centre + static_cast<size_t>(p) * smp.centre_stride;
    ref = (smp.u_ref != nullptr) ? smp.u_ref + static_cast<size_t>(p) * n * 2 : nullptr;
    extra = holds_candidate_2(a, smp) ? smp.u_extra + static_cast<size_t>(p) * n * 2 : nullptr;
    knot_weight = smp.spec.segments;
    chained = smp.prev_keys != nullptr;
#pragma unroll
    for (int q = 0; q < kStagedPairs; ++q) {
      const int j = min(lane + q * kWave, n - 1);
      if (!chained) g_centre[q] = reinterpret_cast<const f32x2*>(centre)[j];
      if (ref != nullptr) g_ref[q] = reinterpret_cast<const f32x2*>(ref)[j];
      if (extra != nullptr) g_extra[q] = reinterpret_cast<const f32x2*>(extra)[j];
      g_weight[q] = reinterpret_cast<const f32x2*>(knot_weight)[j];
    }
    if (chained) {
#pragma unroll
      for (int q = 0; q < kChainBlocks / kWave; ++q)
        prev_key[q] = smp.prev_keys[static_cast<size_t>(p) * smp.prev_blocks + min(lane + q * kWave, smp.prev_blocks - 1)];
    }
  }

  // chained rounds: the previous round's winner is the argmin over its workgroups' keys, and its controls head that
  // workgroup's trace (workgroup b rolled the candidates b * 64 ..: the winner's workgroup follows from its index); the
  // request for THEM is the second round trip
  __device__ __forceinline__ void follow_chain(const RolloutArgs& a, const SampleArgs& smp, const int p, const int lane, const int n) {
    if (!chained) return;
    int64_t best = kKeyMax;
#pragma unroll
    for (int q = 0; q < kChainBlocks / kWave; ++q) {
      const int64_t kb = (lane + q * kWave < smp.prev_blocks) ? prev_key[q] : kKeyMax;
      best = (kb < best) ? kb : best;
    }
    const int64_t winner = wave_min_key(best);
    const int block = static_cast<int>(static_cast<int64_t>(static_cast<uint32_t>(winner & 0xffffffffLL)) - a.index_offset) / kWave;
    centre = smp.prev_trace + (static_cast<size_t>(p) * smp.prev_blocks + block) * smp.prev_pitch;
#pragma unroll
    for (int q = 0; q < kStagedPairs; ++q) g_centre[q] = reinterpret_cast<const f32x2*>(centre)[min(lane + q * kWave, n - 1)];
  }

  // registers -> LDS: [n][2] centre | [n][2] reference (or the centre again) | [n][2] candidate 2's, when given | [n] weights
  __device__ __forceinline__ void store(const int lane, const int n, float* s_centre, float* s_ref, float* s_extra,
                                        float* s_weight) const {
#pragma unroll
    for (int q = 0; q < kStagedPairs; ++q) {
      const int j = lane + q * kWave;
      if (j < n) {
        reinterpret_cast<f32x2*>(s_centre)[j] = g_centre[q];
        reinterpret_cast<f32x2*>(s_ref)[j] = (ref != nullptr) ? g_ref[q] : g_centre[q];
        if (extra != nullptr) reinterpret_cast<f32x2*>(s_extra)[j] = g_extra[q];
        s_weight[j] = g_weight[q][1];
      }
    }
  }

  // horizons beyond the registers' share: plain copies (one more round trip)
  __device__ __forceinline__ void store_beyond(const int lane, const int n, float* s_centre, float* s_ref, float* s_extra,
                                               float* s_weight) const {
    for (int j = lane + kStagedPairs * kWave; j < n; j += kWave) {
      const f32x2 cj = reinterpret_cast<const f32x2*>(centre)[j];
      reinterpret_cast<f32x2*>(s_centre)[j] = cj;
      reinterpret_cast<f32x2*>(s_ref)[j] = (ref != nullptr) ? reinterpret_cast<const f32x2*>(ref)[j] : cj;
      if (extra != nullptr) reinterpret_cast<f32x2*>(s_extra)[j] = reinterpret_cast<const f32x2*>(extra)[j];
      s_weight[j] = knot_weight[2 * j + 1];
    }
  }
};

// Which controls a lane blends its noise round, out of what StagedControls left in LDS.  Candidate 1 = the reference
// controls, candidate 2 = `u_extra` (the LQ plan), each when given: amplitude 0, own centre; every other candidate the centre.
struct CandidateControls {
  struct Step {
    f32x2 centre, ref;
    float weight;
  };
  const f32x2* s_centre;
  const f32x2* s_alt;   // (per lane)
  const float* s_weight;
  bool use_ref;
  float amp;

  __device__ __forceinline__ CandidateControls(const uint32_t gidx, const SampleArgs& smp, const float* centre, const float* ref,
                                               const float* extra, const float* weight)
      : s_centre(reinterpret_cast<const f32x2*>(centre)), s_weight(weight) {
    const bool use_extra = (gidx == 2u) && (smp.u_extra != nullptr);
    use_ref = ((gidx == 1u) && (smp.u_ref != nullptr)) || use_extra;
    s_alt = reinterpret_cast<const f32x2*>(use_extra ? extra : ref);
    amp = use_ref ? 0.0f : candidate_amplitude(gidx);
  }
  // Step i's operands, asked for ahead of the arithmetic.  (The requests behind the last step - one step past the end,
  // two in the form that strides by two - read inside the block, the next array or the padding, and are never used.)
  __device__ __forceinline__ Step at(const int i) const { return Step{s_centre[i], s_alt[i], s_weight[i]}; }
  __device__ __forceinline__ void blend(const SampleSpec& sp, const Step& now, const float (&z)[kKnots][2], const int knot,
                                        float& v, float& k) const {
    const float cv = use_ref ? now.ref[0] : now.centre[0];
    const float ck = use_ref ? now.ref[1] : now.centre[1];
    blend_control(sp, amp, now.weight, cv, ck, z[knot][0], z[knot][1], z[knot + 1][0], z[knot + 1][1], v, k);
  }
};

// The end of a traced round, by the wave that holds the candidates' costs (the only one left of its workgroup): V and cost
// into rows 5n, 5n + 1 of the lane's trace column, the workgroup's best key and feasible count, and the best lane's column
// copied to this workgroup's slot of `fused.trace`.  SHIFT: the X and Y rows (2n + 3i, 2n + 3i + 1) were exchanged in the
// path's own frame - start_temporal() - and leave in the caller's, by the same add as in every other form.
template <bool SHIFT>
__device__ __forceinline__ void publish_traced_round(const RolloutArgs& a, const FusedFinalize& fused, float* s_trace,
                                                     const int p, const int lane, const int c, const float V, const float cost,
                                                     const float ox = 0.0f, const float oy = 0.0f) {
  const int n = a.n;
  const bool active = c < a.N;
  s_trace[(5 * n) * kWave + lane] = V;
  s_trace[(5 * n + 1) * kWave + lane] = cost;
  if (active && a.costs != nullptr) a.costs[static_cast<size_t>(p) * a.N + c] = cost;
  const int64_t own_key = active ? pack_key(cost, static_cast<uint32_t>(a.index_offset + c)) : kKeyMax;
  int best_lane;
  const int64_t key = wave_min_key_by_lane(own_key, best_lane);   // (the index rises with the lane)
  const int nfeas = wave_sum_int((active && V == 0.0f) ? 1 : 0);
  __syncthreads();   // this wave alone by now: orders its column writes before the row reads
  const size_t slot = static_cast<size_t>(p) * gridDim.x + blockIdx.x;
  float* trace_out = fused.trace + slot * fused.trace_pitch;
  for (int e = lane; e < 5 * n + 2; e += kWave) {
    const float value = s_trace[e * kWave + best_lane];
    if constexpr (SHIFT) {
      const int k = e - 2 * n;
      const bool is_x = k >= 0 && k < 3 * n && k % 3 == 0, is_y = k >= 0 && k < 3 * n && k % 3 == 1;
      publish(&trace_out[e], is_x ? value + ox : is_y ? value + oy : value);
    } else {
      publish(&trace_out[e], value);
    }
  }
  if (lane == 0) {
    publish(&a.partial_keys[slot], key);
    publish(&a.partial_feas[slot], nfeas);
  }
}

template <int MODE>
__device__ __forceinline__ void rollout_sampled_body(const RolloutArgs& a, const SampleArgs& smp, float* s_fused,
                                                     const int uniform_lds_floats, const bool traced = false,
                                                     const int trace_lds_floats = 0, float* trace_out = nullptr) {
  float* s_trace = s_fused + trace_lds_floats;
  const int p = blockIdx.y;
  const int lane = threadIdx.x;
  const int c = blockIdx.x * kWave + lane;
  const int n = a.n;
  const Weights w = a.w;
  const SampleSpec sp = smp.spec;
  constexpr int kStride = (MODE == 0) ? kCoefS : kCoefT;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kStride;
  const float* __restrict__ x0 = a.x0 + p * 3;
  const float* __restrict__ centre = smp.centre + static_cast<size_t>(p) * smp.centre_stride;
  const float* __restrict__ ref = (smp.u_ref != nullptr) ? smp.u_ref + static_cast<size_t>(p) * n * 2 : nullptr;
  const float* __restrict__ extra = holds_candidate_2(a, smp) ? smp.u_extra + static_cast<size_t>(p) * n * 2 : nullptr;
  const float* __restrict__ knot_weight = sp.segments;
  float* s_wp = s_fused;
  float* s_xy = s_wp + n * kCoefT;
  if constexpr (MODE == 1) {
    stage_temporal_tables(coef, n, lane, kWave, s_wp, s_xy);
    __syncthreads();
  }

  // The wave-uniform operands of the steps - table rows, centre and reference controls, knot weights: 17 floats per
  // step - go through LDS.  Read where they are needed they are scalar loads that miss this CU's cold scalar cache
  // (58 lines at H = 50), and a lone wave has nothing to hide a miss behind: half of this kernel's wave-cycles were
  // such waits.  Here the lanes fetch them side by side (one round trip, covered by the Philox draws below), and the
  // step loop reads them back as broadcast LDS reads one step ahead of the arithmetic.
  //   s_uni: [n][12] table rows (mode S) | [n][2] centre | [n][2] reference (or the centre again) | [n] knot weights
  float* s_uni = s_fused + uniform_lds_floats;
  float* s_row = s_uni;
  float* s_centre = s_row + ((MODE == 0) ? n * kCoefS : 0);
  float* s_ref = s_centre + 2 * n;
  float* s_extra = s_ref + 2 * n;    // candidate 2's controls (smp.u_extra: the LQ plan), when given
  float* s_weight = s_extra + 2 * n;
  const bool chained = smp.prev_keys != nullptr;   // wave-uniform
  constexpr int kRowQuads = (kStagedSteps * kCoefS / 4 + kWave - 1) / kWave;   // table quads per lane
  constexpr int kPairs = (kStagedSteps + kWave - 1) / kWave;                    // (v, kappa) pairs per lane
  f32x4 g_row[kRowQuads];
  f32x2 g_centre[kPairs], g_ref[kPairs], g_extra[kPairs], g_weight[kPairs];
#pragma unroll
  for (int q = 0; q < kRowQuads; ++q) {
    if constexpr (MODE == 0)
      g_row[q] = reinterpret_cast<const f32x4*>(coef)[min(lane + q * kWave, n * (kCoefS / 4) - 1)];
  }
#pragma unroll
  for (int q = 0; q < kPairs; ++q) {
    const int j = min(lane + q * kWave, n - 1);
    if (!chained) g_centre[q] = reinterpret_cast<const f32x2*>(centre)[j];
    if (ref != nullptr) g_ref[q] = reinterpret_cast<const f32x2*>(ref)[j];
    if (extra != nullptr) g_extra[q] = reinterpret_cast<const f32x2*>(extra)[j];
    g_weight[q] = reinterpret_cast<const f32x2*>(knot_weight)[j];   // (knot, weight) pairs: the weight is [1]
  }
  // chained rounds: the previous launch's partial keys, four per lane, requested with the rest
  int64_t prev_key[kChainBlocks / kWave];
  if (chained) {
#pragma unroll
    for (int q = 0; q < kChainBlocks / kWave; ++q) {
      const int b = lane + q * kWave;
      prev_key[q] = smp.prev_keys[static_cast<size_t>(p) * smp.prev_blocks + min(b, smp.prev_blocks - 1)];
    }
  }

  const bool active = c < a.N;
  float cost = __builtin_inff();
  bool feas = false;
  float z[kKnots][2] = {};
  const uint32_t gidx = static_cast<uint32_t>(a.index_offset + c);
  // first half of the draws (covers the round trip of the requests above), then - chained - the winner of the previous
  // round and the request for ITS controls, which the second half of the draws covers
  if (active) draw_normals<0, kKnots / 4>(sp, gidx, static_cast<uint32_t>(p), z);
  if (chained) {   // the previous round's winner: argmin over its workgroups' keys; its controls head that workgroup's trace
    int64_t best = kKeyMax;
#pragma unroll
    for (int q = 0; q < kChainBlocks / kWave; ++q) {
      const int64_t kb = (lane + q * kWave < smp.prev_blocks) ? prev_key[q] : kKeyMax;
      best = (kb < best) ? kb : best;
    }
    // (workgroup b rolled the candidates b * 64 ..: the winner's workgroup follows from its index)
    const int64_t winner = wave_min_key(best);
    const int block = static_cast<int>(static_cast<int64_t>(static_cast<uint32_t>(winner & 0xffffffffLL)) - a.index_offset) / kWave;
    centre = smp.prev_trace + (static_cast<size_t>(p) * smp.prev_blocks + block) * smp.prev_pitch;
#pragma unroll
    for (int q = 0; q < kPairs; ++q) g_centre[q] = reinterpret_cast<const f32x2*>(centre)[min(lane + q * kWave, n - 1)];
  }
  if (active) draw_normals<kKnots / 4, kKnots / 2>(sp, gidx, static_cast<uint32_t>(p), z);
#pragma unroll
  for (int q = 0; q < kRowQuads; ++q) {
    if constexpr (MODE == 0) {
      const int e = lane + q * kWave;
      if (e < n * (kCoefS / 4)) reinterpret_cast<f32x4*>(s_row)[e] = g_row[q];
    }
  }
#pragma unroll
  for (int q = 0; q < kPairs; ++q) {
    const int j = lane + q * kWave;
    if (j < n) {
      reinterpret_cast<f32x2*>(s_centre)[j] = g_centre[q];
      reinterpret_cast<f32x2*>(s_ref)[j] = (ref != nullptr) ? g_ref[q] : g_centre[q];
      if (extra != nullptr) reinterpret_cast<f32x2*>(s_extra)[j] = g_extra[q];
      s_weight[j] = g_weight[q][1];
    }
  }
  if (n > kStagedSteps) {   // horizons beyond the registers' share: plain copies (a second round trip)
    if constexpr (MODE == 0)
      for (int e = lane + kRowQuads * kWave; e < n * (kCoefS / 4); e += kWave)
        reinterpret_cast<f32x4*>(s_row)[e] = reinterpret_cast<const f32x4*>(coef)[e];
    for (int j = lane + kPairs * kWave; j < n; j += kWave) {
      const f32x2 cj = reinterpret_cast<const f32x2*>(centre)[j];
      reinterpret_cast<f32x2*>(s_centre)[j] = cj;
      reinterpret_cast<f32x2*>(s_ref)[j] = (ref != nullptr) ? reinterpret_cast<const f32x2*>(ref)[j] : cj;
      if (extra != nullptr) reinterpret_cast<f32x2*>(s_extra)[j] = reinterpret_cast<const f32x2*>(extra)[j];
      s_weight[j] = knot_weight[2 * j + 1];
    }
  }
  __syncthreads();   // one wave: orders the staging above before the reads below
  if (active) {
    // candidate 1 = the reference controls, candidate 2 = `u_extra` (the LQ plan), each when given: amplitude 0, own centre
    const bool use_extra = (gidx == 2u) && (smp.u_extra != nullptr);
    const bool use_ref = ((gidx == 1u) && (smp.u_ref != nullptr)) || use_extra;
    const f32x2* s_alt = reinterpret_cast<const f32x2*>(use_extra ? s_extra : s_ref);   // (per lane)
    const float amp = use_ref ? 0.0f : candidate_amplitude(gidx);
    StateS ss{x0[0], x0[1], x0[2], 0.0f, 0.0f};
    StateT ts = start_temporal<float>(x0, coef);
    int nearest = 0;
    struct StepOperands {
      f32x2 centre, ref;
      float weight;
      f32x4 lo, hi;   // table row (mode S): ds, a21, a31, b31 | f3, v_ref, k_ref, ey_lo
      float last;     // ey_hi
    };
    // (the request behind the last step reads inside the block - the next array, or the padding - and is never used)
    auto request = [&](int i) {
      StepOperands o;
      o.centre = reinterpret_cast<const f32x2*>(s_centre)[i];
      o.ref = s_alt[i];
      o.weight = s_weight[i];
      if constexpr (MODE == 0) {
        o.lo = *reinterpret_cast<const f32x4*>(s_row + i * kCoefS);
        o.hi = *reinterpret_cast<const f32x4*>(s_row + i * kCoefS + 4);
        o.last = s_row[i * kCoefS + 8];
      }
      return o;
    };
    StepOperands now = request(sp.knot_begin[0]);
#pragma unroll
    for (int knot = 0; knot < kKnots - 1; ++knot) {
#pragma unroll 2
      for (int i = sp.knot_begin[knot]; i < sp.knot_begin[knot + 1]; ++i) {
        const StepOperands next = request(i + 1);
        float v, k;
        const float cv = use_ref ? now.ref[0] : now.centre[0];
        const float ck = use_ref ? now.ref[1] : now.centre[1];
        blend_control(sp, amp, now.weight, cv, ck, z[knot][0], z[knot][1], z[knot + 1][0], z[knot + 1][1], v, k);
        if constexpr (MODE == 0) {
          const float row[9] = {now.lo[0], now.lo[1], now.lo[2], now.lo[3], now.hi[0],
                                now.hi[1], now.hi[2], now.hi[3], now.last};
          step_spatial<float>(ss, row, v, k, w);
        } else {
          nearest = step_temporal(ts, s_wp, s_xy, n, v, k, w, nearest);
        }
        now = next;
        if (traced) {   // wave-uniform
          float* col = s_trace + lane;
          col[(2 * i) * kWave] = v;
          col[(2 * i + 1) * kWave] = k;
          col[(2 * n + 3 * i) * kWave] = (MODE == 0) ? ss.ey : ts.X + coef[0];       // (poses leave in the caller's frame)
          col[(2 * n + 3 * i + 1) * kWave] = (MODE == 0) ? ss.ep : ts.Y + coef[1];
          col[(2 * n + 3 * i + 2) * kWave] = (MODE == 0) ? ss.t : ts.phi;
        }
      }
    }
    if constexpr (MODE == 0) {
      cost = finish_spatial<float>(ss, w);
      feas = ss.V == 0.0f;
    } else {
      cost = finish_temporal<float>(ts, n, w);
      feas = ts.V == 0.0f;
    }
    if (traced) {
      s_trace[(5 * n) * kWave + lane] = (MODE == 0) ? ss.V : ts.V;
      s_trace[(5 * n + 1) * kWave + lane] = cost;
    }
    if (a.costs != nullptr) a.costs[static_cast<size_t>(p) * a.N + c] = cost;
  }
  const int64_t own_key = active ? pack_key(cost, static_cast<uint32_t>(a.index_offset + c)) : kKeyMax;
  int nfeas = (active && feas) ? 1 : 0;
  int best_lane;
  const int64_t key = wave_min_key_by_lane(own_key, best_lane);   // (the index rises with the lane)
  nfeas = wave_sum_int(nfeas);
  if (traced) {
    __syncthreads();   // one wave: orders the column writes above before the row reads
    for (int e = lane; e < 5 * n + 2; e += kWave) publish(&trace_out[e], s_trace[e * kWave + best_lane]);
  }
  if (lane == 0) {
    const size_t slot = static_cast<size_t>(p) * gridDim.x + blockIdx.x;
    publish(&a.partial_keys[slot], key);
    publish(&a.partial_feas[slot], nfeas);
  }
}

// The same candidate's control at ONE step, for the finalize kernel's lane-per-step regeneration: identical
// arithmetic (blend_control on the same operands), the bracketing knots picked by a select chain.
__device__ __forceinline__ void regenerate_control(const SampleSpec& sp, const float (&z)[kKnots][2], float amp,
                                                   const float* centre, int i, float& v, float& k) {
  const int k0 = static_cast<int>(sp.segments[2 * i]);
  float z0v = z[0][0], z0k = z[0][1], z1v = z[1][0], z1k = z[1][1];
#pragma unroll
  for (int knot = 1; knot < kKnots - 1; ++knot) {
    const bool hit = (k0 == knot);
    z0v = hit ? z[knot][0] : z0v;
    z0k = hit ? z[knot][1] : z0k;
    z1v = hit ? z[knot + 1][0] : z1v;
    z1k = hit ? z[knot + 1][1] : z1k;
  }
  blend_control(sp, amp, sp.segments[2 * i + 1], centre[2 * i], centre[2 * i + 1], z0v, z0k, z1v, z1k, v, k);
}

// One wave per problem.  The winner is re-rolled by the whole wave in lock-step: lane l fetches step l's controls
// and table row (one round of parallel loads), each step's inputs are then broadcast with v_readlane (SGPRs), so
// the sequential chain touches no memory at all; every lane carries the same state and the record image is
// assembled in LDS and written out by all lanes.  Same step functions as the rollout kernel -> same bits.
// `s_rec`: LDS for the record image [4 + 2n + 3(n+1)] and, in mode T, the waypoint table behind it.  Called by one
// whole wave (the only wave of its workgroup).  The partial keys are read with agent-scope atomic loads: when the
// caller is the last workgroup of a fused rollout (below) they were written by other workgroups of the SAME launch.
template <int MODE, int LAYOUT>
__device__ __forceinline__ void finalize_problem(const FinalizeArgs& a, const int p, float* s_rec) {
  const int lane = threadIdx.x;
  const int n = a.n;

  // (mode S) lane l's table row of the first 64 steps and the start state do not depend on who won: requested first,
  // they travel together with the partial keys instead of after the argmin
  float row_first[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float x0_first[3] = {0.0f, 0.0f, 0.0f};
  if constexpr (MODE == 0) {
    if (a.records != nullptr) {
      const float* __restrict__ coef_p = a.coef + static_cast<size_t>(p) * n * kCoefS;
#pragma unroll
      for (int q = 0; q < 9; ++q) row_first[q] = coef_p[min(lane, n - 1) * kCoefS + q];
#pragma unroll
      for (int q = 0; q < 3; ++q) x0_first[q] = a.x0[p * 3 + q];
    }
  }

  int nfeas = 0;
  int64_t key = kKeyMax;
  for (int b = lane; b < a.blocks_per_problem; b += kWave) {
    const size_t slot = static_cast<size_t>(p) * a.blocks_per_problem + b;
    nfeas += __hip_atomic_load(&a.partial_feas[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int64_t kb = __hip_atomic_load(&a.partial_keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
  const bool owner = a.regenerate || (local >= 0 && local < a.N);  // wave-uniform
  if (!owner) {
    for (int e = lane; e < rec_floats; e += kWave) rec[e] = (e == 2) ? static_cast<float>(nfeas) : 0.0f;
    return;
  }

  const Weights w = a.w;
  constexpr int kStride = (MODE == 0) ? kCoefS : kCoefT;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kStride;
  const float* __restrict__ x0 = a.x0 + p * 3;
  const int c = static_cast<int>(local);
  float* su = s_rec + 4;
  float* sx = s_rec + 4 + 2 * n;
  // where the winner's controls come from: the control matrix, or - regenerate - its global index alone
  const uint32_t gidx = static_cast<uint32_t>(key & 0xffffffffLL);
  float z[kKnots][2] = {};
  float amp = 0.0f;
  const float* centre = nullptr;
  if (a.regenerate) {
    draw_normals(a.spec, gidx, static_cast<uint32_t>(p), z);
    const float* alt = (gidx == 1u) ? a.u_ref : (gidx == 2u) ? a.u_extra : nullptr;
    const bool use_ref = alt != nullptr;
    amp = use_ref ? 0.0f : candidate_amplitude(gidx);
    centre = use_ref ? alt + static_cast<size_t>(p) * n * 2 : a.centre + static_cast<size_t>(p) * a.centre_stride;
  }
  auto winner_control = [&](int step, float& v, float& k) {
    if (a.regenerate) {
      regenerate_control(a.spec, z, amp, centre, step, v, k);
    } else {
      float vv[1], kk[1];
      load_controls<LAYOUT, 1>(a.U, p, a.N, n, step, c, vv, kk);
      v = vv[0];
      k = kk[0];
    }
  };

  if (a.controls_only) {
    // between the rounds of an optimisation only the winner's controls are needed (the next round's centre):
    // header = [cost from the key, 0, n_feasible, 1], u block, no re-roll
    for (int step = lane; step < n; step += kWave) {
      float v, k;
      winner_control(step, v, k);
      su[2 * step] = v;
      su[2 * step + 1] = k;
    }
    if (lane == 0) {
      s_rec[0] = key_cost(key);
      s_rec[1] = 0.0f;
      s_rec[2] = static_cast<float>(nfeas);
      s_rec[3] = 1.0f;
    }
    __syncthreads();
    for (int e = lane; e < 4 + 2 * n; e += kWave) rec[e] = s_rec[e];
    return;
  }

  if constexpr (MODE == 0) {
    // Re-roll split by dependence: only the 9-operation state recurrence is sequential (run by the whole wave in
    // lock-step on broadcast inputs); everything that hangs off a state - stage cost, the four bound terms - is
    // evaluated by lane i for step i in parallel, and the partial results are then accumulated in step order so
    // that J and V see exactly the additions of step_spatial(), in the same order.
    float ey = x0_first[0], ep = x0_first[1], t = x0_first[2], J = 0.0f, V = 0.0f;
    for (int base = 0; base < n; base += kWave) {
      const int mine = base + lane;
      const bool valid = mine < n;
      float v[1] = {0.0f}, k[1] = {0.0f};
      float row[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (valid) {
        winner_control(mine, v[0], k[0]);
#pragma unroll
        for (int q = 0; q < 9; ++q) row[q] = (base == 0) ? row_first[q] : coef[mine * kCoefS + q];
        su[2 * mine] = v[0];
        su[2 * mine + 1] = k[0];
      }
      const float dv = v[0] - row[5];
      const float dk = k[0] - row[6];
      const float term_ep = row[0] * dk;   // ds * dk
      const float term_t = row[3] * dv;    // b31 * dv
      float r = quad(w.r0, dv);
      r = r + quad(w.r1, dk);
      const float hu0 = hinge2(w.ulo0 - v[0], v[0] - w.uhi0);
      const float hu1 = hinge2(w.ulo1 - k[0], k[0] - w.uhi1);
      float my_ey = 0.0f, my_ep = 0.0f, my_t = 0.0f, nx_ey = 0.0f, nx_t = 0.0f;
      const int steps = min(kWave, n - base);
      for (int i = 0; i < steps; ++i) {
        const float b_ds = bcast(row[0], i), b_a21 = bcast(row[1], i), b_a31 = bcast(row[2], i);
        const float b_f3 = bcast(row[4], i), b_te = bcast(term_ep, i), b_tt = bcast(term_t, i);
        const float ey_n = ey + b_ds * ep;
        const float ep_n = (ep + b_a21 * ey) + b_te;
        const float t_n = ((t + b_a31 * ey) + b_tt) + b_f3;
        if (lane == i) {
          my_ey = ey;
          my_ep = ep;
          my_t = t;
          nx_ey = ey_n;
          nx_t = t_n;
        }
        ey = ey_n;
        ep = ep_n;
        t = t_n;
      }
      float q = quad(w.q0, my_ey);
      q = q + quad(w.q1, my_ep);
      q = q + quad(w.q2, my_t);
      const float stage = 0.5f * (q + r);
      const float hc = hinge2(row[7] - nx_ey, nx_ey - row[8]);
      const float tv = fmaxf(w.tmin - nx_t, 0.0f);
      const float ht = tv * tv;
      if (valid) {
        sx[3 * mine] = my_ey;
        sx[3 * mine + 1] = my_ep;
        sx[3 * mine + 2] = my_t;
      }
      for (int i = 0; i < steps; ++i) {
        J = J + bcast(stage, i);
        V = V + bcast(hu0, i);
        V = V + bcast(hu1, i);
        V = V + bcast(hc, i);
        V = V + bcast(ht, i);
      }
    }
    if (lane == 0) {
      sx[3 * n] = ey;
      sx[3 * n + 1] = ep;
      sx[3 * n + 2] = t;
      const StateS st{ey, ep, t, J, V};
      s_rec[0] = finish_spatial(st, w);
      s_rec[1] = V;
    }
  } else {
    StateT st = start_temporal<float>(x0, coef);
    // waypoint table -> LDS (behind the record image); each lane also keeps "its" waypoint's (x, y) in registers
    float* s_wp = s_rec + ((rec_floats + 3) & ~3);
    float* s_abc = s_wp + n * kCoefT;
    stage_temporal_tables(coef, n, lane, kWave, s_wp, s_abc);
    if (lane == 0) {
      sx[0] = st.X + coef[0];   // (poses leave in the caller's frame: start_temporal())
      sx[1] = st.Y + coef[1];
      sx[2] = st.phi;
    }
    __syncthreads();
    const int mine_at = kKeyStride * min(lane, n - 1);   // the search key's entries of "this lane's" waypoint
    const float my_a = s_abc[mine_at], my_b = s_abc[mine_at + kKeyB], my_c = s_abc[mine_at + kKeyC];
    int j_prev = 0;
    for (int base = 0; base < n; base += kWave) {
      const int mine = base + lane;
      float v[1] = {0.0f}, k[1] = {0.0f};
      if (mine < n) {
        winner_control(mine, v[0], k[0]);
        su[2 * mine] = v[0];
        su[2 * mine + 1] = k[0];
      }
      const int steps = min(kWave, n - base);
      for (int i = 0; i < steps; ++i) {
        const float vi = bcast(v[0], i), ki = bcast(k[0], i);
        temporal_advance(st, vi, ki, w);
        // nearest waypoint with the lanes scanning the table side by side; (distance, index) keys keep the
        // first minimum exactly like the one-lane scan of the rollout kernel
        // (a search window, when configured, only masks out the waypoints outside it)
        const int win_w = w.nn_back + w.nn_ahead + 1;
        const int win_lo = (w.nn_ahead < 0) ? 0 : max(min(j_prev - w.nn_back, n - win_w), 0);
        const int win_hi = (w.nn_ahead < 0) ? n - 1 : min(win_lo + win_w, n) - 1;
        float best = (lane >= win_lo && lane <= win_hi) ? search_key<float>(st.X, st.Y, my_a, my_b, my_c) : __builtin_inff();
        int j = lane;
        for (int m = lane + kWave; m <= win_hi; m += kWave) {
          const float d = (m >= win_lo) ? search_key<float>(st.X, st.Y, s_abc[kKeyStride * m], s_abc[kKeyStride * m + kKeyB], s_abc[kKeyStride * m + kKeyC])
                                        : __builtin_inff();
          const bool better = d < best;
          best = better ? d : best;
          j = better ? m : j;
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
        j_prev = j;
        temporal_cost(st, s_wp + j * kCoefT, vi, ki, w);
        if (lane == 0) {
          sx[3 * (base + i + 1)] = st.X + coef[0];
          sx[3 * (base + i + 1) + 1] = st.Y + coef[1];
          sx[3 * (base + i + 1) + 2] = st.phi;
        }
      }
    }
    if (lane == 0) {
      s_rec[0] = finish_temporal(st, n, w);
      s_rec[1] = st.V;
    }
  }
  if (lane == 0) {
    s_rec[2] = static_cast<float>(nfeas);
    s_rec[3] = 1.0f;
  }
  __syncthreads();
  for (int e = lane; e < rec_floats; e += kWave) rec[e] = s_rec[e];
}

template <int MODE, int LAYOUT>
__global__ void __launch_bounds__(kWave) finalize_kernel(const FinalizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_finalize[];
  finalize_problem<MODE, LAYOUT>(a, blockIdx.x, s_finalize);
}

constexpr int kGroupFinalizeProblems = 256;   // from this many problems the batched finalize runs sixteen lanes per problem

// The batched solve's finalize, mode S, from 256 problems up (round 4): SIXTEEN LANES PER PROBLEM, four problems per
// wavefront.  finalize_kernel gives every problem a wavefront, which re-rolls its winner in lock-step on broadcast inputs - a
// fine use of a wave when there is one problem, and 4 096 lone-wave walks when there are 4 096: 29 us behind the headline's
// 1.0 ms rollout.  (A LANE per problem - the argmin, the winner's controls and table rows fetched seven steps ahead,
// step_spatial() per lane - was built first: 1/64 of the instructions, but every load and store of a wave goes to 64
// different cache lines and step_spatial's ~45 instructions per step run on 64 lone waves: 20.5 us.)
// finalize_problem()'s decomposition does better on a quarter of a wave per problem:
//   A  lane l of the problem's sixteen prepares steps l, l + 16, ...: the winner's controls (re-drawn - the four Philox
//      blocks of its normals drawn by four of the lanes and shared through LDS - or loaded), the table row, everything of
//      the step that does not depend on the state; the record's u block
//   B  the 9-operation state recurrence, the only sequential part, on operands read from LDS eight steps ahead
//   C  lane l again: stage cost and the two state-dependent bound terms of its steps from the states B left in LDS
//   D  J and V accumulated in step order: the additions of step_spatial(), in its order - the same bits
// and the four record images, contiguous in LDS as the four records are in memory, leave in 16-byte stores: 13.8 us.
// Fewer problems leave the CUs idle either way and keep the wave-per-problem form, whose latency is the shorter.
constexpr int kGroupLanes = 16;
constexpr int kGroupProblems = kWave / kGroupLanes;
constexpr int kGroupRow = 8;     // floats per step in each of the two LDS tables
constexpr int kGroupAhead = 8;   // steps whose LDS operands are requested together in B and D (the kernel of its own)
constexpr int kGroupPass = 4;    // steps per lane whose memory operands are requested together in A (the kernel of its own)

__device__ __forceinline__ int group_finalize_floats_device(int n) {   // one problem per wavefront
  return ((4 + 2 * n + 3 * (n + 1) + 3) & ~3) + 16 + 2 * n * kGroupRow;
}
inline size_t group_finalize_floats(int n, int problems = kGroupProblems) {   // LDS floats of ONE wavefront
  const size_t records = (static_cast<size_t>(problems) * (4 + 2 * n + 3 * (n + 1)) + 3) & ~static_cast<size_t>(3);
  return records + problems * (16 + 2 * static_cast<size_t>(n) * kGroupRow);
}

// finalize_group runs on ONE wavefront: what its lanes hand each other through LDS needs no workgroup barrier (a wave's LDS
// instructions execute in order), only the compiler kept from moving the accesses across the hand-off - so the function
// is the same inside a 256-thread workgroup whose other waves have retired (rollout_chained_kernel)
__device__ __forceinline__ void wave_lds_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wavefront's four problems: threadIdx.x < 64 are its lanes, `group` its place in the batch.  kPass / kAhead: how far
// ahead operands are requested (registers: 116 with 4 / 8, under 64 with 1 / 4 - what a launch shared with the rollout,
// rollout_chained_kernel, can afford).
template <int LAYOUT, int kPass, int kAhead, int kLanes = kGroupLanes>
__device__ __forceinline__ void finalize_group(const FinalizeArgs& a, const int group, float* s_group) {
  constexpr int kProblems = kWave / kLanes;   // problems of this wavefront
  const int lane = static_cast<int>(threadIdx.x) & (kWave - 1);
  const int q = lane / kLanes, sub = lane % kLanes;
  const int n = a.n;
  const int rec_floats = 4 + 2 * n + 3 * (n + 1);
  const int p_first = group * kProblems;
  const int p = p_first + q;
  const bool live = p < a.P;
  const int pl = live ? p : a.P - 1;   // a quarter without a problem repeats the last one's work and writes nothing
  const float* __restrict__ x0 = a.x0 + pl * 3;
  float ey = 0.0f, ep = 0.0f, t = 0.0f;
  float rows_ahead[kPass][9] = {}, seg_ahead[kPass][2] = {}, cen_ahead[kPass][2] = {};
  if (a.records != nullptr) {   // what does not depend on who won travels with the partial keys
    ey = x0[0], ep = x0[1], t = x0[2];
    const float* __restrict__ coef_ahead = a.coef + static_cast<size_t>(pl) * n * kCoefS;
#pragma unroll
    for (int j = 0; j < kPass; ++j) {
      const int i = min(j * kLanes + sub, n - 1);
#pragma unroll
      for (int e = 0; e < 9; ++e) rows_ahead[j][e] = coef_ahead[i * kCoefS + e];
      if (a.regenerate) {   // (the centre every winner but candidates 1 and 2 is drawn round: those two fetch theirs below)
        seg_ahead[j][0] = a.spec.segments[2 * i];
        seg_ahead[j][1] = a.spec.segments[2 * i + 1];
        cen_ahead[j][0] = a.centre[static_cast<size_t>(pl) * a.centre_stride + 2 * i];
        cen_ahead[j][1] = a.centre[static_cast<size_t>(pl) * a.centre_stride + 2 * i + 1];
      }
    }
  }

  int nfeas = 0;
  int64_t key = kKeyMax;
  for (int b = sub; b < a.blocks_per_problem; b += kLanes) {
    const size_t slot = static_cast<size_t>(pl) * a.blocks_per_problem + b;
    nfeas += a.partial_feas[slot];
    const int64_t kb = a.partial_keys[slot];
    key = (kb < key) ? kb : key;
  }
#pragma unroll
  for (int m = kLanes / 2; m >= 1; m >>= 1) {
    nfeas += __shfl_xor(nfeas, m, kLanes);
    const int64_t other = static_cast<int64_t>(__shfl_xor(static_cast<long long>(key), m, kLanes));
    key = (other < key) ? other : key;
  }
  if (a.keys_in != nullptr) key = a.keys_in[pl];
  if (a.keys_out != nullptr && live && sub == 0) a.keys_out[p] = key;
  if (a.records == nullptr) return;

  float* s_rec = s_group + q * rec_floats;
  float* s_tables = s_group + ((kProblems * rec_floats + 3) & ~3);
  float* s_z = s_tables + q * 16;
  float* s_rows = s_tables + kProblems * 16 + q * n * kGroupRow;                      // ds a21 a31 f3 | ds dk, b31 dv, lo, hi
  float* s_terms = s_tables + kProblems * 16 + (kProblems + q) * n * kGroupRow;   // stage (r), hu0, hu1, hc | ht
  float* su = s_rec + 4;
  float* sx = s_rec + 4 + 2 * n;
  const int64_t local = static_cast<int64_t>(static_cast<uint32_t>(key & 0xffffffffLL)) - a.index_offset;
  const bool owner = a.regenerate || (local >= 0 && local < a.N);
  const int c = owner ? static_cast<int>(local) : 0;
  const uint32_t gidx = static_cast<uint32_t>(key & 0xffffffffLL);
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(pl) * n * kCoefS;
  float amp = 0.0f;
  const float* centre = nullptr;
  bool use_alt = false;
  if (a.regenerate) {
    if (sub < kKnots / 2) {
      float four[4];
      draw_normal_block(a.spec, gidx, static_cast<uint32_t>(pl), static_cast<uint32_t>(sub), four);
      *reinterpret_cast<f32x4*>(s_z + 4 * sub) = f32x4{four[0], four[1], four[2], four[3]};
    }
    const float* alt = (gidx == 1u) ? a.u_ref : (gidx == 2u) ? a.u_extra : nullptr;
    use_alt = alt != nullptr;
    amp = use_alt ? 0.0f : candidate_amplitude(gidx);
    centre = use_alt ? alt + static_cast<size_t>(pl) * n * 2 : a.centre + static_cast<size_t>(pl) * a.centre_stride;
  }
  wave_lds_handoff();

  // A: everything of a step that does not depend on the state, four steps per lane and pass; a pass's operands are all
  // requested before the first is used (the first pass's table rows before the keys: rows_ahead above)
  for (int base = 0; base < n; base += kPass * kLanes) {
    float rows[kPass][9], v[kPass], k[kPass], seg[kPass][2], cen[kPass][2];
#pragma unroll
    for (int j = 0; j < kPass; ++j) {
      const int i = min(base + j * kLanes + sub, n - 1);
      if (a.regenerate) {
        if (base == 0) {
          seg[j][0] = seg_ahead[j][0];
          seg[j][1] = seg_ahead[j][1];
        } else {
          seg[j][0] = a.spec.segments[2 * i];
          seg[j][1] = a.spec.segments[2 * i + 1];
        }
        if (base == 0 && !use_alt) {   // (per lane: a quarter whose winner is candidate 1 or 2 fetches its own centre)
          cen[j][0] = cen_ahead[j][0];
          cen[j][1] = cen_ahead[j][1];
        } else {
          cen[j][0] = centre[2 * i];
          cen[j][1] = centre[2 * i + 1];
        }
      } else {
        float vv[1], kk[1];
        load_controls<LAYOUT, 1>(a.U, pl, a.N, n, i, c, vv, kk);
        v[j] = vv[0];
        k[j] = kk[0];
      }
#pragma unroll
      for (int e = 0; e < 9; ++e) rows[j][e] = (base == 0) ? rows_ahead[j][e] : coef[i * kCoefS + e];
    }
#pragma unroll
    for (int j = 0; j < kPass; ++j) {
      const int i = base + j * kLanes + sub;
      if (i < n) {
        if (a.regenerate) {   // regenerate_control()'s operands, the bracketing knots read from LDS
          const int k0 = static_cast<int>(seg[j][0]);
          const int knot = (k0 >= 1 && k0 <= kKnots - 2) ? k0 : 0;
          const float* z = s_z + 2 * knot;
          blend_control(a.spec, amp, seg[j][1], cen[j][0], cen[j][1], z[0], z[1], z[2], z[3], v[j], k[j]);
        }
        const float* row = rows[j];
        const float dv = v[j] - row[5];
        const float dk = k[j] - row[6];
        const float term_ep = row[0] * dk;
        const float term_t = row[3] * dv;
        float r = quad(w.r0, dv);
        r = r + quad(w.r1, dk);
        const float hu0 = hinge2(w.ulo0 - v[j], v[j] - w.uhi0);
        const float hu1 = hinge2(w.ulo1 - k[j], k[j] - w.uhi1);
        *reinterpret_cast<f32x4*>(s_rows + i * kGroupRow) = f32x4{row[0], row[1], row[2], row[4]};
        *reinterpret_cast<f32x4*>(s_rows + i * kGroupRow + 4) = f32x4{term_ep, term_t, row[7], row[8]};
        *reinterpret_cast<f32x4*>(s_terms + i * kGroupRow) = f32x4{r, hu0, hu1, 0.0f};
        su[2 * i] = v[j];
        su[2 * i + 1] = k[j];
      }
    }
  }
  wave_lds_handoff();

  // B: the recurrence (every lane of the quarter runs it on the same LDS words; lane 0 of the quarter leaves the states)
  for (int base = 0; base < n; base += kAhead) {
    f32x4 lo[kAhead];
    float te[kAhead], tt[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      const int i = min(base + j, n - 1);
      lo[j] = *reinterpret_cast<const f32x4*>(s_rows + i * kGroupRow);
      te[j] = s_rows[i * kGroupRow + 4];
      tt[j] = s_rows[i * kGroupRow + 5];
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      const int i = base + j;
      if (i < n) {
        if (sub == 0) {
          sx[3 * i] = ey;
          sx[3 * i + 1] = ep;
          sx[3 * i + 2] = t;
        }
        const float ey_n = ey + lo[j][0] * ep;
        const float ep_n = (ep + lo[j][1] * ey) + te[j];
        const float t_n = ((t + lo[j][2] * ey) + tt[j]) + lo[j][3];
        ey = ey_n;
        ep = ep_n;
        t = t_n;
      }
    }
  }
  if (sub == 0) {
    sx[3 * n] = ey;
    sx[3 * n + 1] = ep;
    sx[3 * n + 2] = t;
  }
  wave_lds_handoff();

  // C: what hangs off a state
  for (int base = 0; base < n; base += kLanes) {
    const int i = base + sub;
    if (i < n) {
      const float my_ey = sx[3 * i], my_ep = sx[3 * i + 1], my_t = sx[3 * i + 2];
      const float nx_ey = sx[3 * i + 3], nx_t = sx[3 * i + 5];
      float s = quad(w.q0, my_ey);
      s = s + quad(w.q1, my_ep);
      s = s + quad(w.q2, my_t);
      const float stage = 0.5f * (s + s_terms[i * kGroupRow]);
      const float hc = hinge2(s_rows[i * kGroupRow + 6] - nx_ey, nx_ey - s_rows[i * kGroupRow + 7]);
      const float tv = fmaxf(w.tmin - nx_t, 0.0f);
      s_terms[i * kGroupRow] = stage;
      s_terms[i * kGroupRow + 3] = hc;
      s_terms[i * kGroupRow + 4] = tv * tv;
    }
  }
  wave_lds_handoff();

  // D: step_spatial()'s additions in its order
  float J = 0.0f, V = 0.0f;
  for (int base = 0; base < n; base += kAhead) {
    f32x4 first[kAhead];
    float ht[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      const int i = min(base + j, n - 1);
      first[j] = *reinterpret_cast<const f32x4*>(s_terms + i * kGroupRow);
      ht[j] = s_terms[i * kGroupRow + 4];
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      if (base + j < n) {
        J = J + first[j][0];
        V = V + first[j][1];
        V = V + first[j][2];
        V = V + first[j][3];
        V = V + ht[j];
      }
    }
  }
  wave_lds_handoff();   // (the terms are read: a problem whose winner lives on another rank may now blank its image)
  if (owner) {
    if (sub == 0) {
      const StateS st{ey, ep, t, J, V};
      s_rec[0] = finish_spatial(st, w);
      s_rec[1] = V;
      s_rec[2] = static_cast<float>(nfeas);
      s_rec[3] = 1.0f;
    }
  } else {
    for (int e = sub; e < rec_floats; e += kLanes) s_rec[e] = (e == 2) ? static_cast<float>(nfeas) : 0.0f;
  }
  wave_lds_handoff();
  const int count = min(kProblems, a.P - p_first) * rec_floats;
  float* __restrict__ out = a.records + static_cast<size_t>(p_first) * rec_floats;
  const int whole = ((reinterpret_cast<uintptr_t>(out) & 15u) == 0) ? (count & ~3) : 0;
  for (int e = 4 * lane; e < whole; e += 4 * kWave) *reinterpret_cast<f32x4*>(out + e) = *reinterpret_cast<const f32x4*>(s_group + e);
  for (int e = whole + lane; e < count; e += kWave) out[e] = s_group[e];
}

template <int LAYOUT>
__global__ void __launch_bounds__(kWave) finalize_groups_kernel(const FinalizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_group[];
  finalize_group<LAYOUT, kGroupPass, kGroupAhead>(a, static_cast<int>(blockIdx.x), s_group);
}

// The same with a whole wavefront per problem and four wavefronts per workgroup (A/B: ACMPC_FINALIZE_WAVES=1; and the
// form the finalize takes inside rollout_chained_kernel): a lane per step in A and C - one pass up to 64 steps, every
// operand requested before the keys are reduced -, B and D as before.
constexpr int kFinalizeWaves = 4;

template <int LAYOUT>
__global__ void __launch_bounds__(kFinalizeWaves * kWave) finalize_waves_kernel(const FinalizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_group[];
  const int wave = static_cast<int>(threadIdx.x) / kWave;
  const int p = static_cast<int>(blockIdx.x) * kFinalizeWaves + wave;
  if (p >= a.P) return;
  finalize_group<LAYOUT, 1, kGroupAhead, kWave>(a, p, s_group + wave * group_finalize_floats_device(a.n));
}

// A STREAM of batches (acmpc_solve_stream_device): batch k's rollout and batch k - 1's finalize in ONE launch.  Behind
// the headline's rollout the finalize of its 4 096 problems is 13-14 us of lone waves plus a launch boundary - 1.7 % of the
// step - and no form of it is fast enough to vanish (a lone wave issues an instruction every 4.2 cycles: finalize_group's
// ~2 400 are 5 us before the first cache miss).  So it runs where nobody waits for it: the LAST rows of the next rollout's
// grid are rows of finalize workgroups - four wavefronts, a problem each, a lane per step (finalize_group<..., 64>: one
// pass, every operand requested before the keys are reduced, two trips to memory).  Rows are dispatched in order, so these
// start when the grid has no rollout workgroup left to hand out, in the wave slots the rollout's last generation leaves
// empty as it drains, and are done before it is.  Measured on the headline's batch (tools/archive/chained_ab.py, launches
// alternating with the plain kernel in one process; tools/archive/finalize_ab.sh, interleaved bench runs): the kernel is as long
// as the plain one or up to 10 us longer (by the box: how ragged the rollout's tail is), the step 2-15 us shorter than
// with two launches in every pair.  What did NOT work, same tools: the
// sixteen-lane form on ONE wave per finalize workgroup in the same last rows, +11.5 us on the kernel (its six dependent
// trips to memory outlast the tail: the step as long as with two launches); the same rows spread evenly through the grid
// (one in seventeen), +25 us - every finalize workgroup then displaces a rollout workgroup for its ~40 us under a saturated
// memory system, 1 024 of them 19 us of the 2 048 resident workgroups' time; raising the lone waves' priority (s_setprio)
// changed nothing, looking further ahead for operands (more registers: spills under the rollout's 64) made it worse.  The
// two batches' partial keys live in different halves of the handle's buffer.
#ifndef ACMPC_CHAINED_PASS
#define ACMPC_CHAINED_PASS 1    // (A/B builds) finalize_group's look-ahead inside the shared launch
#endif
#ifndef ACMPC_CHAINED_AHEAD
#define ACMPC_CHAINED_AHEAD 4
#endif
template <int LAYOUT, int CPT, int BLOCK, int PACK>
__global__ void __launch_bounds__(BLOCK, 8) rollout_chained_kernel(const RolloutArgs a, const FinalizeArgs f) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int y = static_cast<int>(blockIdx.y);
  if (y >= a.P) {
    static_assert(BLOCK == kFinalizeWaves * kWave, "a finalize workgroup is four wavefronts, a problem each");
    const int wave = static_cast<int>(threadIdx.x) / kWave;
    const int p = ((y - a.P) * static_cast<int>(gridDim.x) + static_cast<int>(blockIdx.x)) * kFinalizeWaves + wave;
    if (p >= f.P) return;
    finalize_group<1, ACMPC_CHAINED_PASS, ACMPC_CHAINED_AHEAD, kWave>(
        f, p, reinterpret_cast<float*>(smem) + wave * group_finalize_floats_device(f.n));
    return;
  }
  rollout_block<0, LAYOUT, CPT, BLOCK, PACK, false>(a, smem, y);
}

// Record of problem p out of the winning workgroup's trace (see rollout_sampled_body): argmin over the partial keys,
// then a copy - no arithmetic, so the record holds exactly the bits the winning lane computed, which are the bits a
// re-roll of that candidate computes.  One wave.
__device__ __forceinline__ void finalize_from_trace(const RolloutArgs& a, const FusedFinalize& fused, const int p) {
  const int lane = threadIdx.x;
  const int n = a.n;
  const int blocks = static_cast<int>(gridDim.x);
  // every key is requested before the first is looked at (a load per loop iteration with its compare behind it is one
  // round trip per 64 workgroups: 3 us of a 256-workgroup round's tail); launches beyond the batch go round the loop
  constexpr int kBatch = 4;
  int nfeas = 0;
  int64_t key = kKeyMax;
  for (int b0 = 0; b0 < blocks; b0 += kBatch * kWave) {
    int64_t kb[kBatch];
    int fb[kBatch];
#pragma unroll
    for (int q = 0; q < kBatch; ++q) {
      kb[q] = kKeyMax;
      fb[q] = 0;
      if (b0 + q * kWave < blocks) {   // (wave-uniform)
        const size_t slot = static_cast<size_t>(p) * blocks + min(b0 + q * kWave + lane, blocks - 1);
        kb[q] = observe(&a.partial_keys[slot]);
        fb[q] = observe(&a.partial_feas[slot]);
      }
    }
#pragma unroll
    for (int q = 0; q < kBatch; ++q) {
      const bool mine = b0 + q * kWave + lane < blocks;   // (a clamped lane re-read the last workgroup's slot)
      key = (mine && kb[q] < key) ? kb[q] : key;
      nfeas += mine ? fb[q] : 0;
    }
  }
  nfeas = wave_sum_int(nfeas);
  const int64_t best = wave_min_key(key);
  // workgroup b holds the candidates b * 64 ..: the winner's workgroup follows from its index
  const int block = static_cast<int>(static_cast<int64_t>(static_cast<uint32_t>(best & 0xffffffffLL)) - a.index_offset) / kWave;
  const float* trace = fused.trace + (static_cast<size_t>(p) * blocks + block) * fused.trace_pitch;
  const int rec_floats = 4 + 2 * n + 3 * (n + 1);
  float* __restrict__ rec = fused.records + static_cast<size_t>(p) * rec_floats;
  const float* __restrict__ x0 = a.x0 + p * 3;
  const int count = fused.controls_only ? 4 + 2 * n : rec_floats;
  // every entry but three is ONE load from an address that depends on the entry alone: all of a pass requested, then stored
  constexpr int kSlots = 8;
  for (int e0 = 0; e0 < count; e0 += kSlots * kWave) {
    float value[kSlots];
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      if (e0 + q * kWave < count) {   // (wave-uniform)
        const int e = min(e0 + q * kWave + lane, count - 1);
        const float* src = trace + (e - 7);                               // states: 2n + (e - 4 - 2n - 3)
        src = (e < 4 + 2 * n + 3) ? x0 + (e - (4 + 2 * n)) : src;         // start state
        src = (e < 4 + 2 * n) ? trace + (e - 4) : src;                    // controls
        src = (e < 4) ? trace + 5 * n + (1 - min(e, 1)) : src;            // cost, violation
        value[q] = observe(src);
      }
    }
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      const int e = e0 + q * kWave + lane;
      if (e0 + q * kWave < count) {
        float out = value[q];
        // between rounds the cost is read back from the key (non-finite -> +inf), as the separate finalize does; the
        // last record carries the lane's own
        if (fused.controls_only) out = (e == 0) ? key_cost(best) : (e == 1) ? 0.0f : out;
        out = (e == 2) ? static_cast<float>(nfeas) : (e == 3) ? 1.0f : out;
        if (e < count) rec[e] = out;
      }
    }
  }
}

// rollout_kernel with the finalize in its own launch (round 4): the workgroup that finishes a problem LAST (tickets, as in
// the fused rounds) also takes the argmin over the problem's partial keys and writes the winner's record - re-rolled by
// its first wave with the step functions of the rollout, as finalize_kernel does (finalize_problem: the same bits).  The
// batched solve (4 096 problems x 4 096 candidates) used to follow its 1.09 ms rollout with a finalize_kernel of 4 096
// single-wave workgroups: 29 us + a launch gap, 3.4 % of the step.  Here the re-rolls of all problems but the last few
// run in the shadow of other workgroups' streaming (the kernel is HBM-bound: the vector pipes have room), and only the
// final ones - ~9 us of a lone wave - are exposed.  Mode S, step-major, 256-thread workgroups; one candidate's states per
// lane would not fit the headline kernel's 46 registers, so no trace: the winner is rolled again.
// LDS: [64 bytes: wave keys, counts] [record image 4 + 2n + 3(n + 1) floats].
#ifndef ACMPC_TAILED_WAVES
#define ACMPC_TAILED_WAVES 8   // waves per SIMD asked for: caps the allocation at 64 VGPRs (the tail's re-roll would take 78)
#endif
template <int MODE, int LAYOUT, int CPT, int BLOCK, int PACK>
__global__ void __launch_bounds__(BLOCK, ACMPC_TAILED_WAVES) rollout_tailed_kernel(const RolloutArgs a, const FinalizeArgs f, int* tickets) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  rollout_block<MODE, LAYOUT, CPT, BLOCK, PACK, true>(a, smem, static_cast<int>(blockIdx.y));
  if (threadIdx.x >= kWave) return;   // the tail is the first wave's (the one that published the workgroup's partials)
  const int p = blockIdx.y;
  if (!last_workgroup_of_problem(tickets + static_cast<size_t>(p) * (kTicketGroups + 1) * kTicketStride, kTicketGroups)) return;
  finalize_problem<MODE, LAYOUT>(f, p, reinterpret_cast<float*>(smem + 64));
}

// Optional tail of a fused round (one wave, threadIdx.x = its lanes): see FusedFinalize.
template <int MODE>
__device__ __forceinline__ void fused_tail(const RolloutArgs& a, const SampleArgs& smp, const FusedFinalize& fused,
                                           const bool traced, float* s_finalize) {
  const int p = blockIdx.y;
  if (fused.tickets == nullptr) return;
  if (!last_workgroup_of_problem(fused.tickets + static_cast<size_t>(p) * (kTicketGroups + 1) * kTicketStride, kTicketGroups)) return;
  auto signal_done = [&]() {   // the record (written by all lanes) before the flag (lane 0), both on their way to the host
    if (fused.done == nullptr || p != 0) return;
    __threadfence_system();
    if (threadIdx.x == 0) __hip_atomic_store(fused.done, fused.done_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  if (traced) {
    finalize_from_trace(a, fused, p);
    signal_done();
    return;
  }
  FinalizeArgs f{};
  f.x0 = a.x0;
  f.coef = a.coef;
  f.partial_keys = a.partial_keys;
  f.partial_feas = a.partial_feas;
  f.records = fused.records;
  f.regenerate = true;
  f.controls_only = fused.controls_only;
  f.centre = smp.centre;
  f.u_ref = smp.u_ref;
  f.u_extra = smp.u_extra;
  f.centre_stride = smp.centre_stride;
  f.spec = smp.spec;
  f.blocks_per_problem = static_cast<int>(gridDim.x);
  f.P = a.P;
  f.N = a.N;
  f.n = a.n;
  f.index_offset = a.index_offset;
  f.w = a.w;
  finalize_problem<MODE, 1>(f, p, s_finalize);
  signal_done();
}

// LDS: [rollout part: mode T tables] [trace [5n + 2][64], or - no trace - the finalize's record image (+ mode T table)]
//      [uniform operands of the steps: sampled_uniform_floats()]
template <int MODE>
__global__ void __launch_bounds__(kWave) rollout_sampled_kernel(const RolloutArgs a, const SampleArgs smp,
                                                                const FusedFinalize fused, const int rollout_lds_floats,
                                                                const int uniform_lds_floats) {
  extern __shared__ __attribute__((aligned(16))) float s_fused[];
  const int p = blockIdx.y;
  const bool traced = fused.trace != nullptr;
  rollout_sampled_body<MODE>(a, smp, s_fused, uniform_lds_floats, traced, rollout_lds_floats,
                             fused.trace + (static_cast<size_t>(p) * gridDim.x + blockIdx.x) * fused.trace_pitch);
  fused_tail<MODE>(a, smp, fused, traced, s_fused + rollout_lds_floats);
}

// The traced mode-S round on TWO waves per workgroup.  A round at the closed-loop size is one wave per CU walking a serial
// stream of ~5 700 instructions, three SIMDs of its CU idle, and the stream falls into two parts that only meet in
// (v, kappa): drawing the normals and blending them into the controls of each step, and rolling those controls.  Here
// wave 1 - the producer - draws and blends, running ahead through the horizon and handing (v, kappa) per step and lane
// over through LDS in chunks of kPairChunk steps, two buffers; wave 0 - the consumer - rolls them (step_spatial, the
// same call) one chunk behind, one barrier per chunk, and then reduces, publishes and runs the tail as the single-wave
// kernel does.  Same operations on the same operands: same bits (test_optimize_forms_agree).
// LDS: [trace [5n + 2][64]] [uniform operands] [exchange [2][kPairChunk][2][64]].
constexpr int kPairChunk = 7;
constexpr int kPairValues = 2;

__global__ void __launch_bounds__(2 * kWave) rollout_sampled_pair_kernel(const RolloutArgs a, const SampleArgs smp,
                                                                         const FusedFinalize fused,
                                                                         const int uniform_lds_floats,
                                                                         const int exchange_lds_floats) {
  extern __shared__ __attribute__((aligned(16))) float s_fused[];
  float* s_trace = s_fused;
  float* s_row = s_fused + uniform_lds_floats;
  const int p = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1);
  const bool consumer = threadIdx.x < kWave;   // wave 0 (so that the tail's threadIdx.x are its lanes)
  const int n = a.n;
  float* s_centre = s_row + n * kCoefS;
  float* s_ref = s_centre + 2 * n;
  float* s_extra = s_ref + 2 * n;    // candidate 2's controls (smp.u_extra: the LQ plan), when given
  float* s_weight = s_extra + 2 * n;
  float* s_exchange = s_fused + exchange_lds_floats + lane;   // [buffer][step of the chunk][v | kappa][lane]
  constexpr int kStepFloats = kPairValues * kWave, kBufferFloats = kPairChunk * kStepFloats;
  const int c = blockIdx.x * kWave + lane;
  const Weights w = a.w;

  if (!consumer) {
    // ---- producer: requests, draws, the uniform operands of ITS half into LDS, then the controls chunk by chunk ----
    const SampleSpec sp = smp.spec;
    StagedControls staged;
    staged.request(a, smp, p, lane, n);
    float z[kKnots][2] = {};
    const uint32_t gidx = static_cast<uint32_t>(a.index_offset + c);
    draw_normals<0, kKnots / 4>(sp, gidx, static_cast<uint32_t>(p), z);
    staged.follow_chain(a, smp, p, lane, n);
    draw_normals<kKnots / 4, kKnots / 2>(sp, gidx, static_cast<uint32_t>(p), z);
    staged.store(lane, n, s_centre, s_ref, s_extra, s_weight);
    staged.store_beyond(lane, n, s_centre, s_ref, s_extra, s_weight);
    __syncthreads();   // (0) the consumer has put the table rows in, this wave the rest
    const CandidateControls controls(gidx, smp, s_centre, s_ref, s_extra, s_weight);
    CandidateControls::Step now = controls.at(sp.knot_begin[0]);
    float* out = s_exchange;          // slot of the step being produced
    float* u_out = s_trace + lane;    // its place in the trace (rows 2i, 2i + 1)
    int in_chunk = 0, buffer = 0;
#pragma unroll
    for (int knot = 0; knot < kKnots - 1; ++knot) {
      for (int i = sp.knot_begin[knot]; i < sp.knot_begin[knot + 1]; ++i) {
        const CandidateControls::Step next = controls.at(i + 1);
        float v, k;
        controls.blend(sp, now, z, knot, v, k);
        out[0] = v;
        out[kWave] = k;
        u_out[0] = v;
        u_out[kWave] = k;
        now = next;
        out += kStepFloats;
        u_out += 2 * kWave;
        if (++in_chunk == kPairChunk || i == n - 1) {   // chunk handed over (wave-uniform)
          __syncthreads();
          in_chunk = 0;
          buffer ^= 1;
          out = s_exchange + buffer * kBufferFloats;
        }
      }
    }
    return;
  }

  // ---- consumer: table rows into LDS, then the rollout one chunk behind the producer ----
  {
    const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefS;
    for (int q = lane; q < n * (kCoefS / 4); q += kWave)
      reinterpret_cast<f32x4*>(s_row)[q] = reinterpret_cast<const f32x4*>(coef)[q];
  }
  const float* __restrict__ x0 = a.x0 + p * 3;
  StateS st{x0[0], x0[1], x0[2], 0.0f, 0.0f};
  __syncthreads();   // (0)
  struct StepInputs {
    float v, k;
    f32x4 lo, hi;
    float last;
  };
  auto inputs_of = [&](const float* in, int i) {
    StepInputs s;
    s.v = in[0];
    s.k = in[kWave];
    const float* t = s_row + i * kCoefS;
    s.lo = *reinterpret_cast<const f32x4*>(t);
    s.hi = *reinterpret_cast<const f32x4*>(t + 4);
    s.last = t[8];
    return s;
  };
  auto advance = [&](int i, const StepInputs& in) {
    const float row[9] = {in.lo[0], in.lo[1], in.lo[2], in.lo[3], in.hi[0], in.hi[1], in.hi[2], in.hi[3], in.last};
    step_spatial<float>(st, row, in.v, in.k, w);
    s_trace[(2 * n + 3 * i) * kWave + lane] = st.ey;
    s_trace[(2 * n + 3 * i + 1) * kWave + lane] = st.ep;
    s_trace[(2 * n + 3 * i + 2) * kWave + lane] = st.t;
  };
  for (int first = 0, buffer = 0; first < n; first += kPairChunk, buffer ^= 1) {
    __syncthreads();   // this chunk is in its buffer (and the producer may start on the other one)
    const float* in = s_exchange + buffer * kBufferFloats;
    if (first + kPairChunk <= n) {   // a full chunk, straight-line: every step's reads can move ahead of the arithmetic
      StepInputs steps[kPairChunk];
#pragma unroll
      for (int j = 0; j < kPairChunk; ++j) steps[j] = inputs_of(in + j * kStepFloats, first + j);
#pragma unroll
      for (int j = 0; j < kPairChunk; ++j) advance(first + j, steps[j]);
    } else {
      for (int j = 0; first + j < n; ++j) advance(first + j, inputs_of(in + j * kStepFloats, first + j));
    }
  }
  publish_traced_round<false>(a, fused, s_trace, p, lane, c, st.V, finish_spatial<float>(st, w));
  fused_tail<0>(a, smp, fused, true, nullptr);
}

// The traced mode-S round on FOUR waves per workgroup.  The two-wave form above splits drawing from rolling.  Measured with
// either side stubbed out, its pace (0.144 us per step) was the DRAWING wave's blend - 124 ns per step - not the rolling
// wave's.  Of a mode S step only the 9-operation recurrence is sequential: the blend of step i needs nothing of step
// i - 1, and the bound violations read the state AFTER the step and the controls and feed nothing back (J never reads V,
// V never reads J: the split of rollout_solo_kernel).  So, one wave per SIMD of the CU:
//   waves 2, 3 (controls):       blend and leave (v, kappa) of every step in the lane's trace column - the even steps one
//                                wave, the odd steps the other;
//   wave 1 (recurrence + cost):  step_spatial_cost on those controls, one chunk behind: J, and the states into the trace;
//   wave 0 (bounds):             V += the four hinges from the trace, two chunks behind; takes J over at the end,
//                                finishes the cost, reduces, publishes and runs the tail.
// Every accumulation sees the operands of step_spatial() in its order: same bits (test_tick_forms_agree).  The Philox
// draws - a quarter of the normals each - are shared out over the four waves and exchanged through LDS, so the round's
// fixed part shrinks too.  A software pipeline over chunks of kQuadChunk steps, one workgroup barrier per chunk; every
// wave's chunk is straight-line code with all its LDS reads in front of the arithmetic.  (A fifth wave - cost and
// recurrence apart - shares a SIMD with another and set the pace there: 10.2 us per round against this form's.)
// LDS: [trace [5n + 2][64]] [table rows n x 12 | centre | reference | knot weights] [normals 16 x 64] [J 64].
#ifndef ACMPC_QUAD_CHUNK
#define ACMPC_QUAD_CHUNK 7
#endif
constexpr int kQuadChunk = ACMPC_QUAD_CHUNK;

constexpr int kQuadWaves = 4;   // bounds; recurrence + cost; two control waves

__global__ void __launch_bounds__(kQuadWaves * kWave) rollout_sampled_quad_kernel(const RolloutArgs a, const SampleArgs smp,
                                                                         const FusedFinalize fused, const int uniform_lds_floats,
                                                                         const int normals_lds_floats) {
  extern __shared__ __attribute__((aligned(16))) float s_fused[];
  float* s_trace = s_fused;
  float* s_row = s_fused + uniform_lds_floats;
  const int p = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  const int n = a.n;
  float* s_centre = s_row + n * kCoefS;
  float* s_ref = s_centre + 2 * n;
  float* s_extra = s_ref + 2 * n;    // candidate 2's controls (smp.u_extra: the LQ plan), when given
  float* s_weight = s_extra + 2 * n;
  float* s_z = s_fused + normals_lds_floats;          // [knot][component][lane]
  float* s_j = s_z + 2 * kKnots * kWave;
  const int c = blockIdx.x * kWave + lane;
  const Weights w = a.w;
  const SampleSpec sp = smp.spec;
  const uint32_t gidx = static_cast<uint32_t>(a.index_offset + c);
  const int chunks = (n + kQuadChunk - 1) / kQuadChunk;
  float* col = s_trace + lane;   // rows 2i, 2i + 1 = (v, kappa) of step i; 2n + 3i .. + 2 = state after step i
  const float* __restrict__ x0 = a.x0 + p * 3;

  // this wave's quarter of the candidate's normals (Philox call `wave`: knots 2 wave, 2 wave + 1) -> LDS
  auto draw_quarter = [&](auto quarter) {
    constexpr int Q = decltype(quarter)::value;
    float z[kKnots][2] = {};
    draw_normals<Q, Q + 1>(sp, gidx, static_cast<uint32_t>(p), z);
#pragma unroll
    for (int knot = 2 * Q; knot < 2 * Q + 2; ++knot) {
      s_z[(2 * knot) * kWave + lane] = z[knot][0];
      s_z[(2 * knot + 1) * kWave + lane] = z[knot][1];
    }
  };
  static_assert(kKnots == 8, "four Philox calls per candidate, one per wave");

  // the controls of the steps i = parity, parity + 2, ... (every step with one control wave's worth of work halved): blend,
  // leave (v, kappa) in the trace; one barrier per chunk, taken by both control waves
  auto produce_controls = [&](const float (&z)[kKnots][2], const int parity) {
    const CandidateControls controls(gidx, smp, s_centre, s_ref, s_extra, s_weight);
    // (Broadcasting the operands out of the registers they were fetched into with v_readlane, instead of reading them
    // back from LDS one step ahead: 187 ns per step against 144 - measured, not kept.)
    CandidateControls::Step now = controls.at(parity);
    int in_chunk = 0;
#pragma unroll
    for (int knot = 0; knot < kKnots - 1; ++knot) {
      for (int i = sp.knot_begin[knot]; i < sp.knot_begin[knot + 1]; ++i) {
        if ((i & 1) == parity) {   // (wave-uniform)
          const CandidateControls::Step next = controls.at(i + 2);   // one own step ahead of the arithmetic
          float v, k;
          controls.blend(sp, now, z, knot, v, k);
          col[(2 * i) * kWave] = v;
          col[(2 * i + 1) * kWave] = k;
          now = next;
        }
        if (++in_chunk == kQuadChunk || i == n - 1) {   // chunk handed on (wave-uniform)
          __syncthreads();
          in_chunk = 0;
        }
      }
    }
  };

  if (wave == 3) {
    // ---- the second control wave: its quarter of the draws, nothing to stage; the odd steps of every chunk ----
    draw_quarter(std::integral_constant<int, 3>{});
    __syncthreads();   // (S)
    float z[kKnots][2];
#pragma unroll
    for (int knot = 0; knot < kKnots; ++knot) {
      z[knot][0] = s_z[(2 * knot) * kWave + lane];
      z[knot][1] = s_z[(2 * knot + 1) * kWave + lane];
    }
    produce_controls(z, 1);
    return;
  }
  if (wave == 2) {
    // ---- controls: requests, its quarter of the draws, the uniform operands of the control waves into LDS, then chunk by chunk ----
    StagedControls staged;
    staged.request(a, smp, p, lane, n);
    draw_quarter(std::integral_constant<int, 2>{});
    staged.follow_chain(a, smp, p, lane, n);
    staged.store(lane, n, s_centre, s_ref, s_extra, s_weight);
    staged.store_beyond(lane, n, s_centre, s_ref, s_extra, s_weight);
    __syncthreads();   // (S) every wave's normals and the table rows are in
    float z[kKnots][2];
#pragma unroll
    for (int knot = 0; knot < kKnots; ++knot) {
      z[knot][0] = s_z[(2 * knot) * kWave + lane];
      z[knot][1] = s_z[(2 * knot + 1) * kWave + lane];
    }
    produce_controls(z, 0);
    return;
  }

  // ---- the other two waves: table rows into LDS, their quarters of the draws ----
  {
    const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefS;
    for (int q = threadIdx.x; q < n * (kCoefS / 4); q += 2 * kWave)
      reinterpret_cast<f32x4*>(s_row)[q] = reinterpret_cast<const f32x4*>(coef)[q];
  }
  if (wave == 0) draw_quarter(std::integral_constant<int, 0>{});
  if (wave == 1) draw_quarter(std::integral_constant<int, 1>{});
  __syncthreads();   // (S)

  if (wave == 1) {
    // ---- recurrence + cost: one chunk behind the controls ----
    StateS st{x0[0], x0[1], x0[2], 0.0f, 0.0f};
    auto roll = [&](int i, float v, float k, const f32x4& lo, const f32x4& hi) {
      const float cr[7] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2]};
      step_spatial_cost(st, cr, v, k, w);
      col[(2 * n + 3 * i) * kWave] = st.ey;
      col[(2 * n + 3 * i + 1) * kWave] = st.ep;
      col[(2 * n + 3 * i + 2) * kWave] = st.t;
    };
    __syncthreads();   // chunk 0 of the controls is in
    for (int t = 1; t <= chunks; ++t) {
      const int first = (t - 1) * kQuadChunk;
      if (first + kQuadChunk <= n) {   // a full chunk, straight-line: every step's reads move ahead of the arithmetic
        float v[kQuadChunk], k[kQuadChunk];
        f32x4 lo[kQuadChunk], hi[kQuadChunk];
#pragma unroll
        for (int q = 0; q < kQuadChunk; ++q) {
          v[q] = col[(2 * (first + q)) * kWave];
          k[q] = col[(2 * (first + q) + 1) * kWave];
          lo[q] = *reinterpret_cast<const f32x4*>(s_row + (first + q) * kCoefS);
          hi[q] = *reinterpret_cast<const f32x4*>(s_row + (first + q) * kCoefS + 4);
        }
#pragma unroll
        for (int q = 0; q < kQuadChunk; ++q) roll(first + q, v[q], k[q], lo[q], hi[q]);
      } else {
        for (int i = first; i < n; ++i)
          roll(i, col[(2 * i) * kWave], col[(2 * i + 1) * kWave], *reinterpret_cast<const f32x4*>(s_row + i * kCoefS),
               *reinterpret_cast<const f32x4*>(s_row + i * kCoefS + 4));
      }
      if (t == chunks) s_j[lane] = st.J;   // (ordered before the bounds wave's read by the two barriers that follow there)
      __syncthreads();   // chunk t - 1 rolled (and, while t < chunks, chunk t of the controls is in)
    }
    return;
  }

  // ---- bounds (wave 0): two chunks behind the controls ----
  StateS st{x0[0], x0[1], x0[2], 0.0f, 0.0f};
  __syncthreads();   // chunk time 0
  __syncthreads();   // chunk time 1: chunk 0 rolled
  {
    auto account = [&](float v, float k, float ey_lo, float ey_hi, float ey_after, float t_after) {
      st.V = st.V + hinge2<float>(w.ulo0 - v, v - w.uhi0);
      st.V = st.V + hinge2<float>(w.ulo1 - k, k - w.uhi1);
      st.V = st.V + hinge2<float>(ey_lo - ey_after, ey_after - ey_hi);
      const float tv = vmax(w.tmin - t_after, 0.0f);
      st.V = st.V + tv * tv;
    };
    for (int t = 2; t <= chunks + 1; ++t) {
      const int first = (t - 2) * kQuadChunk;
      if (first + kQuadChunk <= n) {
        float v[kQuadChunk], k[kQuadChunk], ey[kQuadChunk], tt[kQuadChunk], lo[kQuadChunk], hi[kQuadChunk];
#pragma unroll
        for (int q = 0; q < kQuadChunk; ++q) {
          const int i = first + q;
          v[q] = col[(2 * i) * kWave];
          k[q] = col[(2 * i + 1) * kWave];
          ey[q] = col[(2 * n + 3 * i) * kWave];
          tt[q] = col[(2 * n + 3 * i + 2) * kWave];
          lo[q] = s_row[i * kCoefS + 7];
          hi[q] = s_row[i * kCoefS + 8];
        }
#pragma unroll
        for (int q = 0; q < kQuadChunk; ++q) account(v[q], k[q], lo[q], hi[q], ey[q], tt[q]);
      } else {
        for (int i = first; i < n; ++i)
          account(col[(2 * i) * kWave], col[(2 * i + 1) * kWave], s_row[i * kCoefS + 7], s_row[i * kCoefS + 8],
                  col[(2 * n + 3 * i) * kWave], col[(2 * n + 3 * i + 2) * kWave]);
      }
      __syncthreads();   // (the last one: J handed over)
    }
    // the state after the last step, for the terminal cost
    st.ey = col[(2 * n + 3 * (n - 1)) * kWave];
    st.ep = col[(2 * n + 3 * (n - 1) + 1) * kWave];
    st.t = col[(2 * n + 3 * (n - 1) + 2) * kWave];
  }
  st.J = s_j[lane];
  // (st.ey / ep / t: the state after the last step)
  publish_traced_round<false>(a, fused, s_trace, p, lane, c, st.V, finish_spatial<float>(st, w));
  fused_tail<0>(a, smp, fused, true, nullptr);
}

// The traced mode-T round on THREE waves per workgroup.  On one wave a mode T step is a serial stream of ~110 instructions
// with two dependent LDS gathers in it (the window's keys, then the nearest waypoint's row): 0.6 us per step, 29 us per
// round.  But the pose does not depend on the search - only the cost does - so the step falls into three stages that
// meet in LDS, in the trace the round keeps anyway:
//   wave 2 (poses):  draws and blends the controls, integrates the pose (temporal_advance), leaves (v, kappa) and
//                    (X, Y, phi) of every step in the lane's trace column;
//   wave 1 (search): reads (X, Y), finds the nearest waypoint from the previous step's (the one sequential chain left),
//                    leaves the index;
//   wave 0 (costs):  reads pose, controls and index, gathers the waypoint's row, accumulates the cost terms
//                    (temporal_cost) - independent from step to step, so its gathers overlap - then reduces, publishes
//                    and runs the tail as the single-wave kernel does.
// A software pipeline over chunks of kTrioChunk steps, one workgroup barrier per chunk: at chunk time t wave 2 works on
// chunk t, wave 1 on chunk t - 1, wave 0 on chunk t - 2.  The search wave sets the pace (~0.2 us per step: its keys are a
// dependent LDS gather per step), so the chunk only decides how long the pipeline takes to fill and drain: measured tick
// p50 at chunks of 10 / 7 / 4 / 3 / 2 steps: 67.1 / 65.5 / 63.0 / 61.8 / 62.7 us (one wave per workgroup: 86.3).  Same operations on the same operands: same bits
// (test_tick_forms_agree with ACMPC_NO_TRIO_ROUNDS).
// LDS: [waypoint rows n x 8 | key table n x 3] [trace [5n + 2][64]] [uniform operands: centre, reference, knot weights]
//      [nearest indices [n][64], 16-bit].
#ifndef ACMPC_TRIO_CHUNK
#define ACMPC_TRIO_CHUNK 3
#endif
constexpr int kTrioChunk = ACMPC_TRIO_CHUNK;

__global__ void __launch_bounds__(3 * kWave) rollout_sampled_trio_kernel(const RolloutArgs a, const SampleArgs smp,
                                                                         const FusedFinalize fused, const int trace_lds_floats,
                                                                         const int uniform_lds_floats,
                                                                         const int index_lds_floats) {
  extern __shared__ __attribute__((aligned(16))) float s_fused[];
  const int p = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  const int n = a.n;
  const Weights w = a.w;
  float* s_wp = s_fused;
  float* s_abc = s_wp + n * kCoefT;
  float* s_trace = s_fused + trace_lds_floats;
  float* s_centre = s_fused + uniform_lds_floats;
  float* s_ref = s_centre + 2 * n;
  float* s_extra = s_ref + 2 * n;    // candidate 2's controls (smp.u_extra: the LQ plan), when given
  float* s_weight = s_extra + 2 * n;
  // (16-bit entries: horizons go to 1 025 steps; as 32-bit ones the frames of the verified search stopped fitting beside the
  // trace at the mapping controller's horizon of 100 once the key table grew to 32 bytes per waypoint)
  unsigned short* s_index = reinterpret_cast<unsigned short*>(s_fused + index_lds_floats);
  const int c = blockIdx.x * kWave + lane;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefT;
  const float* __restrict__ x0 = a.x0 + p * 3;
  const int chunks = (n + kTrioChunk - 1) / kTrioChunk;
  float* col = s_trace + lane;   // this lane's trace column: rows 2i, 2i + 1 = (v, kappa); 2n + 3i .. + 2 = pose after step i

  if (wave == 2) {
    // ---- poses: requests, draws, uniform operands into LDS, then controls and poses chunk by chunk ----
    const SampleSpec sp = smp.spec;
    StagedControls staged;
    staged.request(a, smp, p, lane, n);
    float z[kKnots][2] = {};
    const uint32_t gidx = static_cast<uint32_t>(a.index_offset + c);
    draw_normals<0, kKnots / 4>(sp, gidx, static_cast<uint32_t>(p), z);
    staged.follow_chain(a, smp, p, lane, n);
    draw_normals<kKnots / 4, kKnots / 2>(sp, gidx, static_cast<uint32_t>(p), z);
    staged.store(lane, n, s_centre, s_ref, s_extra, s_weight);
    staged.store_beyond(lane, n, s_centre, s_ref, s_extra, s_weight);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // this wave reads what its own lanes staged
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const CandidateControls controls(gidx, smp, s_centre, s_ref, s_extra, s_weight);
    StateT pose = start_temporal<float>(x0, coef);
    CandidateControls::Step now = controls.at(sp.knot_begin[0]);
    int in_chunk = 0;
#pragma unroll
    for (int knot = 0; knot < kKnots - 1; ++knot) {
      for (int i = sp.knot_begin[knot]; i < sp.knot_begin[knot + 1]; ++i) {
        const CandidateControls::Step next = controls.at(i + 1);
        float v, k;
        controls.blend(sp, now, z, knot, v, k);
        now = next;
        temporal_advance<float>(pose, v, k, w);
        col[(2 * i) * kWave] = v;
        col[(2 * i + 1) * kWave] = k;
        col[(2 * n + 3 * i) * kWave] = pose.X;
        col[(2 * n + 3 * i + 1) * kWave] = pose.Y;
        col[(2 * n + 3 * i + 2) * kWave] = pose.phi;
        if (++in_chunk == kTrioChunk || i == n - 1) {   // chunk handed on (wave-uniform)
          __syncthreads();
          in_chunk = 0;
        }
      }
    }
    return;
  }

  // ---- the other two waves put the waypoint tables into LDS (the pose wave does not read them) ----
  stage_temporal_tables(coef, n, static_cast<int>(threadIdx.x), 2 * kWave, s_wp, s_abc);
  float* s_frames = s_wp + ((n * (kCoefT + kKeyStride) + 3) & ~3);   // exhaustive search: its frames, when given
  if (a.nn_frames != nullptr) {
    const float* __restrict__ frames = a.nn_frames + static_cast<size_t>(p) * verified_frame_floats(n);
    for (int e = static_cast<int>(threadIdx.x); e < verified_frame_floats(n); e += 2 * kWave) s_frames[e] = frames[e];
  }
  if (wave == 1) {
    // ---- search: one chunk behind the poses ----
    int j_prev = 0;
    __syncthreads();   // chunk 0 of the poses is in (and - a barrier orders all LDS writes before it - the tables)
    with_search_kind(w, n, [&](auto kind) {
      for (int t = 1; t <= chunks; ++t) {
        const int first = (t - 1) * kTrioChunk;
        // the chunk's positions first (they do not depend on the search): one round trip, not one per step
        float X[kTrioChunk], Y[kTrioChunk];
#pragma unroll
        for (int q = 0; q < kTrioChunk; ++q) {
          const int i = min(first + q, n - 1);
          X[q] = col[(2 * n + 3 * i) * kWave];
          Y[q] = col[(2 * n + 3 * i + 1) * kWave];
        }
#pragma unroll
        for (int q = 0; q < kTrioChunk; ++q) {
          if (first + q < n) {   // (wave-uniform)
            if constexpr (decltype(kind)::value == kSearchVerified) {
              j_prev = propose_nearest(X[q], Y[q], s_abc, n, j_prev);   // (confirmed by the cost wave)
            } else {
              j_prev = search_temporal_as<decltype(kind)::value>(X[q], Y[q], s_abc, n, w, j_prev);
            }
            s_index[(first + q) * kWave + lane] = static_cast<unsigned short>(j_prev);
          }
        }
        __syncthreads();   // chunk t - 1 searched (and, while t < chunks, chunk t of the poses is in)
      }
    }, a.nn_frames != nullptr);
    return;
  }

  // ---- costs: two chunks behind the poses ----
  const bool confirm = search_kind(w, n, a.nn_frames != nullptr) == kSearchVerified;
  StateT st = start_temporal<float>(x0, coef);
  __syncthreads();   // chunk time 0
  __syncthreads();   // chunk time 1: chunk 0 searched
  for (int t = 2; t <= chunks + 1; ++t) {
    const int last = min((t - 1) * kTrioChunk, n);
#pragma unroll
    for (int q = 0; q < kTrioChunk; ++q) {
      const int i = (t - 2) * kTrioChunk + q;
      if (i < last) {   // (wave-uniform)
        st.X = col[(2 * n + 3 * i) * kWave];
        st.Y = col[(2 * n + 3 * i + 1) * kWave];
        st.phi = col[(2 * n + 3 * i + 2) * kWave];
        int j = s_index[i * kWave + lane];
        if (confirm) {   // (wave-uniform) the search wave's proposal, held against the frame of its window
          const int before = (i == 0) ? 0 : s_index[(i - 1) * kWave + lane];
          j = confirm_nearest(st.X, st.Y, s_abc, s_frames, n, before, j);
        }
        temporal_cost(st, s_wp + j * kCoefT, col[(2 * i) * kWave], col[(2 * i + 1) * kWave], w);
      }
    }
    if (t <= chunks) __syncthreads();   // (the last chunk times have no partner left to wait for)
  }
  publish_traced_round<true>(a, fused, s_trace, p, lane, c, st.V, finish_temporal<float>(st, n, w), coef[0], coef[1]);
  fused_tail<1>(a, smp, fused, true, nullptr);
}

}  // namespace

bool tailed_rollout_fits(int mode, int layout, const LaunchShape& shape, int n) {
  const size_t rec_floats = static_cast<size_t>(4 + 2 * n + 3 * (n + 1));
  return mode == 0 && layout == 1 && !shape.tile && shape.block == 256 && (shape.cpt == 1 || shape.cpt == 2 || shape.cpt == 4) &&
         64 + rec_floats * sizeof(float) <= 64 * 1024;
}

hipError_t launch_rollout_tailed(int layout, const LaunchShape& shape, const RolloutArgs& args, const FinalizeArgs& fin,
                                 int* tickets, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  clear_stale_error();
  if (!tailed_rollout_fits(0, layout, shape, args.n) || tickets == nullptr) return hipErrorInvalidValue;
  const dim3 grid(shape.blocks_per_problem, args.P);
  const size_t lds = 64 + static_cast<size_t>(4 + 2 * args.n + 3 * (args.n + 1)) * sizeof(float);
  if (shape.cpt == 1) return launch_kernel(rollout_tailed_kernel<0, 1, 1, 256, 1>, grid, dim3(256), lds, s, e0, e1, args, fin, tickets);
  if (shape.cpt == 2) return launch_kernel(rollout_tailed_kernel<0, 1, 2, 256, 2>, grid, dim3(256), lds, s, e0, e1, args, fin, tickets);
  return launch_kernel(rollout_tailed_kernel<0, 1, 4, 256, 2>, grid, dim3(256), lds, s, e0, e1, args, fin, tickets);
}

// rollout of one batch + finalize of the batch before it in one launch (rollout_chained_kernel): mode S, step-major
// rollout on the 256-thread shapes; a pending finalize of the many-problem kind whose winners are re-drawn or read from a
// step-major matrix, and whose LDS image leaves the rollout its eight workgroups per CU
bool chained_rollout_fits(int mode, int layout, const LaunchShape& shape, int P, const FinalizeArgs& fin, int fin_layout) {
  const int fin_groups = (fin.P + kFinalizeWaves - 1) / kFinalizeWaves;
  const int rows = (fin_groups + std::max(shape.blocks_per_problem, 1) - 1) / std::max(shape.blocks_per_problem, 1);
  return rows <= P && static_cast<long long>(P) + rows <= 65535 && mode == 0 && layout == 1 && !shape.tile && shape.block == 256 && (shape.cpt == 1 || shape.cpt == 2 || shape.cpt == 4) &&
         !fin.controls_only && fin.records != nullptr && fin.keys_in == nullptr && fin.P >= 1 && (fin.regenerate || fin_layout == 1) &&
         kFinalizeWaves * group_finalize_floats(fin.n, 1) * sizeof(float) <= 20 * 1024;
}

hipError_t launch_rollout_chained(int layout, const LaunchShape& shape, const RolloutArgs& args, const FinalizeArgs& fin,
                                  int fin_layout, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  clear_stale_error();
  if (!chained_rollout_fits(0, layout, shape, args.P, fin, fin_layout)) return hipErrorInvalidValue;
  const int groups = (fin.P + kFinalizeWaves - 1) / kFinalizeWaves;
  const int fin_rows = (groups + shape.blocks_per_problem - 1) / shape.blocks_per_problem;
  const dim3 grid(shape.blocks_per_problem, args.P + fin_rows);
  const size_t lds = std::max<size_t>(64, kFinalizeWaves * group_finalize_floats(fin.n, 1) * sizeof(float));
  if (shape.cpt == 1) return launch_kernel(rollout_chained_kernel<1, 1, 256, 1>, grid, dim3(256), lds, s, e0, e1, args, fin);
  if (shape.cpt == 2) return launch_kernel(rollout_chained_kernel<1, 2, 256, 2>, grid, dim3(256), lds, s, e0, e1, args, fin);
  return launch_kernel(rollout_chained_kernel<1, 4, 256, 2>, grid, dim3(256), lds, s, e0, e1, args, fin);
}

hipError_t launch_finalize(int mode, int layout, const FinalizeArgs& args, hipStream_t s, const LaunchOptions& opt) {
  clear_stale_error();
  if (mode == 0 && !args.controls_only && args.P >= kGroupFinalizeProblems && !opt.no_group_finalize &&
      (layout == 0 || layout == 1) && group_finalize_floats(args.n) * sizeof(float) <= 64 * 1024) {
    if (opt.finalize_waves && kFinalizeWaves * group_finalize_floats(args.n, 1) * sizeof(float) <= 64 * 1024) {
      const dim3 waves_grid((args.P + kFinalizeWaves - 1) / kFinalizeWaves);
      const size_t waves_lds = kFinalizeWaves * group_finalize_floats(args.n, 1) * sizeof(float);
      const dim3 waves_block(kFinalizeWaves * kWave);
      if (layout == 0) return launch_kernel(finalize_waves_kernel<0>, waves_grid, waves_block, waves_lds, s, nullptr, nullptr, args);
      return launch_kernel(finalize_waves_kernel<1>, waves_grid, waves_block, waves_lds, s, nullptr, nullptr, args);
    }
    // many problems: sixteen lanes per problem, four problems per wavefront (finalize_groups_kernel)
    const dim3 groups_grid((args.P + kGroupProblems - 1) / kGroupProblems);
    const size_t groups_lds = group_finalize_floats(args.n) * sizeof(float);
    if (layout == 0) return launch_kernel(finalize_groups_kernel<0>, groups_grid, dim3(kWave), groups_lds, s, nullptr, nullptr, args);
    return launch_kernel(finalize_groups_kernel<1>, groups_grid, dim3(kWave), groups_lds, s, nullptr, nullptr, args);
  }
  const dim3 grid(args.P), block(kWave);
  // record image, then (mode T) the waypoint table
  const size_t rec_floats = static_cast<size_t>(4 + 2 * args.n + 3 * (args.n + 1));
  const size_t lds = (((rec_floats + 3) & ~static_cast<size_t>(3)) + (mode == 1 ? args.n * (kCoefT + kKeyStride) : 0)) * sizeof(float);
  if (mode == 0 && layout == 0) return launch_kernel(finalize_kernel<0, 0>, grid, block, lds, s, nullptr, nullptr, args);
  if (mode == 0 && layout == 1) return launch_kernel(finalize_kernel<0, 1>, grid, block, lds, s, nullptr, nullptr, args);
  if (mode == 1 && layout == 0) return launch_kernel(finalize_kernel<1, 0>, grid, block, lds, s, nullptr, nullptr, args);
  if (mode == 1 && layout == 1) return launch_kernel(finalize_kernel<1, 1>, grid, block, lds, s, nullptr, nullptr, args);
  return hipErrorInvalidValue;
}

hipError_t launch_sample(int layout, const SampleArgs& args, hipStream_t s) {
  clear_stale_error();
  const dim3 grid((args.N + 255) / 256, args.P);
  const size_t sample_lds = (((static_cast<size_t>(args.n) + 3) & ~static_cast<size_t>(3)) + 2 * args.n) * sizeof(float);
  if (layout == 0) return launch_kernel(sample_kernel<0>, grid, dim3(256), sample_lds, s, nullptr, nullptr, args);
  if (layout == 1) return launch_kernel(sample_kernel<1>, grid, dim3(256), sample_lds, s, nullptr, nullptr, args);
  return hipErrorInvalidValue;
}

namespace {
size_t sampled_rollout_floats(int mode, int n) {
  return (mode == 1) ? ((static_cast<size_t>(n) * (kCoefT + kKeyStride) + 3) & ~static_cast<size_t>(3)) : 0;
}
// uniform operands of the steps staged in LDS: [n][12] table rows (mode S), centre, reference, candidate 2's controls, knot weights (+ padding
// for the read one step past the end)
size_t sampled_uniform_floats(int mode, int n) {
  return static_cast<size_t>(n) * ((mode == 0 ? kCoefS : 0) + 7) + 4;
}
size_t sampled_finalize_floats(int mode, int n) {
  const size_t rec_floats = static_cast<size_t>(4 + 2 * n + 3 * (n + 1));
  return ((rec_floats + 3) & ~static_cast<size_t>(3)) + (mode == 1 ? static_cast<size_t>(n) * (kCoefT + kKeyStride) : 0);
}
}  // namespace

bool fused_finalize_fits(int mode, int n) {
  return (sampled_rollout_floats(mode, n) + sampled_finalize_floats(mode, n) + sampled_uniform_floats(mode, n)) *
             sizeof(float) <= 64 * 1024;
}

int trace_floats(int n) { return 5 * n + 2; }

// The traced form keeps [5n + 2][64] floats in LDS per workgroup (63 kB at H = 50): up to the CU's 160 kB.
bool traced_finalize_fits(int mode, int n) {
  return (sampled_rollout_floats(mode, n) + static_cast<size_t>(trace_floats(n)) * kWave +
          sampled_uniform_floats(mode, n)) * sizeof(float) <= 160 * 1024;
}

// Which kernel one sampled round runs and how its LDS is laid out: THE place where that is decided - the launch below
// takes what this returns, and so does acmpc_describe_rounds.
SampledForm choose_sampled_form(int mode, int n, bool traced, bool tail, bool frames, const LaunchOptions& opt) {
  constexpr size_t kBudget = 160u * 1024u;
  SampledForm form{};
  // one wave per workgroup: mode T tables | trace, or the record image of the re-rolling tail | uniform operands
  const size_t rollout_floats = sampled_rollout_floats(mode, n);
  const size_t trace = static_cast<size_t>(trace_floats(n)) * kWave;
  const size_t finalize_floats = traced ? trace : tail ? sampled_finalize_floats(mode, n) : 0;
  const size_t uniform_floats = sampled_uniform_floats(mode, n);
  form.kernel = kSampledSingle;
  form.lds = (rollout_floats + finalize_floats + uniform_floats) * sizeof(float);
  form.offset[0] = static_cast<int>(rollout_floats);
  form.offset[1] = static_cast<int>(rollout_floats + finalize_floats);
  if (form.lds > kBudget) return form;  // no form fits (callers check *_fits() first)
  if (mode == 1 && traced && !opt.no_trio_rounds) {
    // three waves per workgroup: tables | trace | uniform operands (centre, reference, weights) | nearest indices
    const size_t plain_tables = (static_cast<size_t>(n) * (kCoefT + kKeyStride) + 3) & ~static_cast<size_t>(3);
    const size_t uniform = (static_cast<size_t>(n) * 7 + 4 + 3) & ~static_cast<size_t>(3);
    const size_t index = (static_cast<size_t>(n) * kWave / 2 + 3) & ~static_cast<size_t>(3);   // 16-bit entries
    // the frames of the verified search ride along when they fit beside the rest (they do up to n = 106); a longer
    // horizon keeps the three waves and scans every waypoint, as it did before there were frames
    bool with_frames = frames && n >= kVerifiedWindow;
    size_t tables = plain_tables + (with_frames ? static_cast<size_t>(verified_frame_floats(n)) : 0);
    if ((tables + trace + uniform + index) * sizeof(float) > kBudget) {
      with_frames = false;
      tables = plain_tables;
    }
    const size_t trio_lds = (tables + trace + uniform + index) * sizeof(float);
    if (trio_lds <= kBudget) {
      form.kernel = kSampledTrio;
      form.frames = with_frames;
      form.lds = trio_lds;
      form.offset[0] = static_cast<int>(tables);
      form.offset[1] = static_cast<int>(tables + trace);
      form.offset[2] = static_cast<int>(tables + trace + uniform);
      return form;
    }
  }
  if (mode == 0 && traced && !opt.no_quad_rounds && !opt.no_pair_rounds) {
    // four waves per workgroup: trace | uniform operands (table rows, centre, reference, weights) | normals | J
    const size_t uniform = (uniform_floats + 3) & ~static_cast<size_t>(3);
    const size_t quad_lds = (trace + uniform + static_cast<size_t>(2 * kKnots + 1) * kWave) * sizeof(float);
    if (quad_lds <= kBudget) {
      form.kernel = kSampledQuad;
      form.lds = quad_lds;
      form.offset[0] = static_cast<int>(trace);
      form.offset[1] = static_cast<int>(trace + uniform);
      return form;
    }
  }
  if (mode == 0 && traced && !opt.no_pair_rounds) {
    // two waves per workgroup: trace | uniform operands | exchange buffers (no mode T tables, no record image)
    const size_t exchange = static_cast<size_t>(2) * kPairChunk * kPairValues * kWave;
    const size_t pair_lds = (trace + uniform_floats + exchange) * sizeof(float);
    if (pair_lds <= kBudget) {
      form.kernel = kSampledPair;
      form.lds = pair_lds;
      form.offset[0] = static_cast<int>(trace);
      form.offset[1] = static_cast<int>(trace + uniform_floats);
      return form;
    }
  }
  return form;
}

// whether the frames of the verified search fit beside the three-wave mode T round's tables, trace, operands and indices
// (the round drops them otherwise and the search wave scans every waypoint): they do up to n = 106
bool trio_frames_fit(int n) { return choose_sampled_form(1, n, true, true, true, LaunchOptions()).frames; }

hipError_t launch_rollout_sampled(int mode, const RolloutArgs& rollout, const SampleArgs& sample,
                                  const FusedFinalize& fused, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                                  const LaunchOptions& opt) {
  clear_stale_error();
  const int n = rollout.n;
  const dim3 grid((rollout.N + kWave - 1) / kWave, rollout.P);
  const bool traced = fused.trace != nullptr;
  if (mode != 0 && mode != 1) return hipErrorInvalidValue;
  const SampledForm form = choose_sampled_form(mode, n, traced, fused.tickets != nullptr, rollout.nn_frames != nullptr, opt);
  if (form.lds > 160u * 1024u) return hipErrorInvalidValue;  // callers check *_fits() first
  if (traced && fused.trace_pitch < trace_floats(n)) return hipErrorInvalidValue;
  if (form.kernel == kSampledTrio) {
    RolloutArgs rollout_trio = rollout;
    if (!form.frames) rollout_trio.nn_frames = nullptr;
    return launch_kernel_lds<&rollout_sampled_trio_kernel>(grid, dim3(3 * kWave), form.lds, s, e0, e1, rollout_trio, sample,
                                                           fused, form.offset[0], form.offset[1], form.offset[2]);
  }
  if (form.kernel == kSampledQuad)
    return launch_kernel_lds<&rollout_sampled_quad_kernel>(grid, dim3(kQuadWaves * kWave), form.lds, s, e0, e1, rollout,
                                                           sample, fused, form.offset[0], form.offset[1]);
  if (form.kernel == kSampledPair)
    return launch_kernel_lds<&rollout_sampled_pair_kernel>(grid, dim3(2 * kWave), form.lds, s, e0, e1, rollout, sample,
                                                           fused, form.offset[0], form.offset[1]);
  if (mode == 0)
    return launch_kernel_lds<&rollout_sampled_kernel<0>>(grid, dim3(kWave), form.lds, s, e0, e1, rollout, sample, fused,
                                                         form.offset[0], form.offset[1]);
  return launch_kernel_lds<&rollout_sampled_kernel<1>>(grid, dim3(kWave), form.lds, s, e0, e1, rollout, sample, fused,
                                                       form.offset[0], form.offset[1]);
}

}  // namespace acmpc
