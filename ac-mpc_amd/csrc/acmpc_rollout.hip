// The rollouts over a caller's control matrix, with the library's flags: rollout_kernel's instantiations (acmpc_rollout.h),
// the candidate-major LDS-tile kernel, choose_shape.  Those built with -fno-slp-vectorize: acmpc_kernels_temporal.hip; the
// tailed and chained rollouts, which share their launch with a finalize: acmpc_kernels.hip.
#include "acmpc_rollout.h"

namespace acmpc {

namespace {

// Candidate-major control matrix U[P][N][n][2] (what NumPy host code holds): a wave's 64 candidates are 64
// consecutive rows = ONE contiguous span of 64 * 8n bytes.  The wave copies that span into LDS with 16-byte loads
// (every HBM line fetched exactly once, fully coalesced) and then walks the steps reading its own row with
// ds_read_b64: the row pitch is 2n dwords, which for odd n (every horizon the reference uses) lands the 32 lanes
// of a read group on 32 distinct bank pairs - conflict-free without padding.  One wave per workgroup, so the LDS
// budget (8n * 64 bytes = 25 KB at H = 50) sets the occupancy: 6 waves per CU, each with its whole tile in flight.
// Measured 3.2 TB/s at H = 50 (a chunked, software-pipelined variant with 16 waves per CU and 8-byte row-wise loads
// measured 2.9 TB/s, plain per-lane strided loads 3.0 TB/s): the step-major layout is the fast path.
template <int MODE>
__global__ void __launch_bounds__(kWave) rollout_tile_kernel(const RolloutArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_tile[];  // [64][2n] then (mode T) the waypoint table
  const int p = blockIdx.y;
  const int lane = threadIdx.x;
  const int c0 = blockIdx.x * kWave;
  const int rows = min(kWave, a.N - c0);
  const int n = a.n;
  const int row_floats = 2 * n;
  const Weights w = a.w;
  constexpr int kStride = (MODE == 0) ? kCoefS : kCoefT;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kStride;
  const float* __restrict__ x0 = a.x0 + p * 3;
  float* s_wp = s_tile + ((kWave * row_floats + 3) & ~3);

  const size_t first = (static_cast<size_t>(p) * a.N + c0) * row_floats;  // float index of the span
  const float* __restrict__ src = a.U + first;
  const int total = rows * row_floats;
  if ((first & 3) == 0) {
    const f32x4* __restrict__ src4 = reinterpret_cast<const f32x4*>(src);
    f32x4* dst4 = reinterpret_cast<f32x4*>(s_tile);
    const int quads = total >> 2;
#pragma unroll 8
    for (int q = lane; q < quads; q += kWave) dst4[q] = __builtin_nontemporal_load(src4 + q);
    for (int e = (quads << 2) + lane; e < total; e += kWave) s_tile[e] = src[e];
  } else {  // span starts on an 8-byte boundary only (odd p * N): 8-byte copies
    const f32x2* __restrict__ src2 = reinterpret_cast<const f32x2*>(src);
    f32x2* dst2 = reinterpret_cast<f32x2*>(s_tile);
#pragma unroll 8
    for (int q = lane; q < (total >> 1); q += kWave) dst2[q] = __builtin_nontemporal_load(src2 + q);
  }
  float* s_xy = s_wp + n * kCoefT;
  if constexpr (MODE == 1) {
    stage_temporal_tables(coef, n, lane, kWave, s_wp, s_xy);
  }
  __syncthreads();

  const bool active = lane < rows;
  float cost = __builtin_inff();
  bool feas = false;
  if (active) {
    const f32x2* row = reinterpret_cast<const f32x2*>(s_tile + lane * row_floats);
    if constexpr (MODE == 0) {
      StateS st{x0[0], x0[1], x0[2], 0.0f, 0.0f};
#pragma unroll 7
      for (int i = 0; i < n; ++i) {
        const f32x2 vk = row[i];
        step_spatial(st, coef + i * kCoefS, vk[0], vk[1], w);
      }
      cost = finish_spatial(st, w);
      feas = st.V == 0.0f;
    } else {
      StateT st = start_temporal<float>(x0, coef);
      int nearest = 0;
      for (int i = 0; i < n; ++i) {
        const f32x2 vk = row[i];
        nearest = step_temporal(st, s_wp, s_xy, n, vk[0], vk[1], w, nearest);
      }
      cost = finish_temporal(st, n, w);
      feas = st.V == 0.0f;
    }
    if (a.costs != nullptr) a.costs[static_cast<size_t>(p) * a.N + c0 + lane] = cost;
  }
  int64_t key = active ? pack_key(cost, static_cast<uint32_t>(a.index_offset + c0 + lane)) : kKeyMax;
  int nfeas = (active && feas) ? 1 : 0;
  key = wave_min_key(key);
  nfeas = wave_sum_int(nfeas);
  if (lane == 0) {
    const size_t slot = static_cast<size_t>(p) * gridDim.x + blockIdx.x;
    a.partial_keys[slot] = key;
    a.partial_feas[slot] = nfeas;
  }
}

template <int MODE>
hipError_t launch_rollout_tile(const LaunchShape& shape, const RolloutArgs& args, hipStream_t s, hipEvent_t e0,
                               hipEvent_t e1) {
  const dim3 grid(shape.blocks_per_problem, args.P);
  const size_t lds = tile_lds_bytes(MODE, args.n);
  return launch_kernel(rollout_tile_kernel<MODE>, grid, dim3(kWave), lds, s, e0, e1, args);
}

template <int MODE, int LAYOUT>
hipError_t launch_rollout_ml(const LaunchShape& shape, const RolloutArgs& args, hipStream_t s, hipEvent_t e0,
                             hipEvent_t e1) {
  if constexpr (MODE == 1 && LAYOUT == 1) {
    // plain float32 arithmetic, one state per candidate: built in its own translation unit (acmpc_kernels_temporal.hip)
    if (shape.pack == 1) return launch_rollout_temporal_plain(shape, args, s, e0, e1);
  }
  if constexpr (LAYOUT == 0) {
    if constexpr (MODE == 0) {
      // (the rows kernel moves 16-byte pieces: a control matrix that does not start on a 16-byte boundary - a view
      // into a caller's buffer - takes the other kernel)
      if (shape.tile && shape.tile_waves == 4 && (reinterpret_cast<uintptr_t>(args.U) & 15u) == 0)
        return launch_rollout_tile_rows_plain(shape, args, s, e0, e1);
    }
    if (shape.tile) return launch_rollout_tile<MODE>(shape, args, s, e0, e1);
  }
  if (shape.block == 64 && shape.cpt == 1) return launch_rollout_t<MODE, LAYOUT, 1, 64>(shape, args, s, e0, e1);
  if (shape.block == 256 && shape.cpt == 1) return launch_rollout_t<MODE, LAYOUT, 1, 256>(shape, args, s, e0, e1);
  if constexpr (LAYOUT == 1) {
    if (shape.block == 256 && shape.cpt == 2) return launch_rollout_t<MODE, LAYOUT, 2, 256>(shape, args, s, e0, e1);
    if (shape.block == 256 && shape.cpt == 4) return launch_rollout_t<MODE, LAYOUT, 4, 256>(shape, args, s, e0, e1);
  }
  return hipErrorInvalidConfiguration;
}

}  // namespace

int max_blocks_per_problem(int N) { return (N + kWave - 1) / kWave; }

size_t tile_lds_bytes(int mode, int n) {
  const size_t tile = (static_cast<size_t>(kWave) * 2 * n + 3) & ~static_cast<size_t>(3);
  return (tile + (mode == 1 ? static_cast<size_t>(n) * (kCoefT + kKeyStride) : 0)) * sizeof(float);
}

LaunchShape choose_shape(int P, int N, int layout, int mode, int n, const LaunchOptions& opt) {
  // Fill 256 CUs first (small batches: 64-thread workgroups, one candidate per lane), then widen the
  // per-lane work so that each wave load moves 16 B per lane (large step-major batches).
  LaunchShape s;
  s.tile = false;
  s.tile_waves = 0;
  s.pack = (mode == 1) ? 1 : 2;  // mode T: plain float32 states (see launch_rollout_temporal_plain)
  if (mode == 1 && opt.temporal_pack != 0) s.pack = opt.temporal_pack;   // (mode S's launches are packed pairs whatever it says)
  s.tile_table = opt.tile_table;
  const long long total = static_cast<long long>(P) * N;
  if (layout == 0 && tile_lds_bytes(mode, n) <= 64 * 1024 && !opt.no_tile) {
    // candidate-major: one wave per workgroup stages its 64 rows in LDS (rollout_tile_kernel)
    s.tile = true;
    s.block = kWave;
    s.cpt = 1;
    s.blocks_per_problem = (N + kWave - 1) / kWave;
    // mode S up to kTileRowsMaxSteps steps: rows in registers, the LDS tile shared by the waves of a workgroup in turn
    // (needs every problem's span on a 16-byte boundary)
    // - from 2 048 tiles up: below that the four-wave workgroups leave CUs idle (16 x 320 x 49: 19 us against 12)
    if (mode == 0 && n <= kTileRowsMaxSteps && (P == 1 || (2LL * N * n) % 4 == 0) &&
        static_cast<long long>(P) * s.blocks_per_problem >= 2048) {
      s.tile_waves = 4;
      if (opt.tile_rows >= 0) s.tile_waves = (opt.tile_rows == 4) ? 4 : 0;
    }
    return s;
  }
  // tuning override for experiments: ACMPC_SHAPE="<block>,<cpt>"
  int fb = opt.shape_block, fc = opt.shape_cpt;
  if (!((fb == 64 && fc == 1) || (fb == 256 && (fc == 1 || (layout == 1 && (fc == 2 || fc == 4) && N % fc == 0)))))
    fb = fc = 0;
  if (fb != 0) {
    s.block = fb;
    s.cpt = fc;
  } else if (total <= 256LL * 64 * 8) {
    s.block = 64;
    s.cpt = 1;
  } else if (mode == 1 && layout == 1 && N % 2 == 0) {
    // mode T waits on LDS gathers: two candidates per lane keep twice the waves in flight that four would at the same
    // batch size (1 M candidates: 155 us against 175 us at the 8-waypoint window)
    s.block = 256;
    s.cpt = 2;
  } else if (layout == 1 && N % 4 == 0 && total >= 256LL * 4096) {
    // from 1 M candidates up: four candidates per lane as two packed pairs (v_pk_* arithmetic, 16-byte loads).
    // Same-box A/B on 256 x 4 096 x 49 / 1 024 x 4 096 x 49: one per lane 72 / 290 us, two 85 / 285 us, four 68 / 283 us.
    s.block = 256;
    s.cpt = 4;
  } else {
    s.block = 256;
    s.cpt = 1;
  }
  const int per_block = s.block * s.cpt;
  s.blocks_per_problem = (N + per_block - 1) / per_block;
  return s;
}

hipError_t launch_rollout(int mode, int layout, const LaunchShape& shape, const RolloutArgs& args, hipStream_t s,
                          hipEvent_t e0, hipEvent_t e1) {
  clear_stale_error();
  if (mode == 0 && layout == 0) return launch_rollout_ml<0, 0>(shape, args, s, e0, e1);
  if (mode == 0 && layout == 1) return launch_rollout_ml<0, 1>(shape, args, s, e0, e1);
  if (mode == 1 && layout == 0) return launch_rollout_ml<1, 0>(shape, args, s, e0, e1);
  if (mode == 1 && layout == 1) return launch_rollout_ml<1, 1>(shape, args, s, e0, e1);
  return hipErrorInvalidValue;
}

}  // namespace acmpc
