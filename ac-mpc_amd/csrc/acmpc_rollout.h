// The rollout templates that two units instantiate: acmpc_rollout.hip with the library's flags, acmpc_kernels_temporal.hip
// with -fno-slp-vectorize (launch_rollout_temporal_plain there has the measurement); acmpc_kernels.hip takes rollout_block.
//   rollout_kernel   one lane = one candidate (or CPT adjacent candidates), steps sequential; the per-step
//                    table is wave-uniform, so in mode S it is read with scalar loads (SGPRs, no LDS traffic)
//                    and in mode T - where every lane gathers "its" nearest waypoint - it is staged in LDS once
//                    per workgroup.  Controls are streamed from HBM exactly once; costs are written once.
//                    Each workgroup reduces its (cost, index) keys with wave shuffles + LDS and writes ONE
//                    partial key: no atomics, no pre-zeroed buffers, bitwise reproducible.
#pragma once
#include "acmpc_kernels_impl.h"

namespace acmpc {

namespace {

// PACK = candidates per arithmetic state: 2 = pairs in v_pk_* instructions, 1 = plain float32 instructions.
// Mode T with two candidates per lane needs 67 VGPRs as the compiler allocates it freely: seven waves per SIMD, where a
// launch of 1 M candidates is eight - the eighth workgroup of every CU then runs alone after the others (a second
// generation of lone waves: +15 % on the launch).  Asking for eight waves per SIMD caps the allocation at 64.
// WAVES = 8 asks for that many waves per SIMD, which caps the allocation at 64 VGPRs.  Measured, 1 M candidates (256 poses
// x 4 096), same box, 67 VGPRs / capped: verified 16-waypoint search 331 / 283 us, 4-waypoint window 102.5 / 92.8 us -
// but the 8-waypoint window 134.9 / 141.3 us (its waves already queue for the LDS: an eighth wave per SIMD adds to the
// queue what it saves on the tail), so the launcher caps every search but that one.  (The verified search, since round 3
// an 8-waypoint window + its certificate: 190 us capped, 225 us uncapped.)
template <int MODE, int LAYOUT, int CPT, int BLOCK, int PACK, bool PUBLISH>
__device__ __forceinline__ void rollout_block(const RolloutArgs& a, unsigned char* smem, const int p) {
  // carve: [0,32) wave keys | [32,48) wave feasible counts | [64, ...) mode-T waypoint table
  int64_t* s_key = reinterpret_cast<int64_t*>(smem);
  int* s_feas = reinterpret_cast<int*>(smem + 32);
  float* s_wp = reinterpret_cast<float*>(smem + 64);

  const int tid = threadIdx.x;
  const int c0 = (blockIdx.x * BLOCK + tid) * CPT;
  const bool active = c0 < a.N;  // N % CPT == 0 is guaranteed by the launcher
  const int n = a.n;
  const Weights w = a.w;
  constexpr int kStride = (MODE == 0) ? kCoefS : kCoefT;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kStride;
  const float* __restrict__ x0 = a.x0 + p * 3;

  ACMPC_T_STAMP(0);
  if (a.start_clock != nullptr && threadIdx.x == 0)   // (wave-uniform: a scalar compare when the diagnostic is off)
    a.start_clock[static_cast<size_t>(p) * gridDim.x + blockIdx.x] = wall_clock64();
  float* s_xy = s_wp + n * kCoefT;  // the nearest-waypoint search's key table: (a, b, c) per waypoint (search_entry)
  float* s_frames = s_xy + ((kKeyStride * n + 3) & ~3);  // frames of the verified search (exhaustive semantics), when given
  if constexpr (MODE == 1) {
    stage_temporal_tables(coef, n, tid, BLOCK, s_wp, s_xy);
    if (a.nn_frames != nullptr) {
      const float* __restrict__ frames = a.nn_frames + static_cast<size_t>(p) * verified_frame_floats(n);
      for (int e = tid; e < verified_frame_floats(n); e += BLOCK) s_frames[e] = frames[e];
    }
    __syncthreads();
  }
  ACMPC_T_STAMP(1);

  float cost[CPT];
  bool feas[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    cost[j] = __builtin_inff();
    feas[j] = false;
  }

  // Mode T's verified nearest-waypoint search has a wave-cooperative fallback that every lane must reach, so there
  // the tail lanes of the last workgroup roll a valid dummy (the problem's last candidates) instead of idling.
  const bool run = active || (MODE == 1 && a.nn_frames != nullptr);
  const int c_run = active ? c0 : max(a.N - CPT, 0);
  if (run) {
    constexpr int kPack = PACK;
    static_assert(CPT % PACK == 0, "a lane's candidates split evenly into arithmetic states");
    constexpr int kGroups = CPT / kPack;
    using F = typename std::conditional<kPack == 2, f32x2, float>::type;
    using I = typename IndexOf<F>::type;
    auto pack = [](const float (&src)[CPT], int g) {
      if constexpr (kPack == 2) {
        F out;
        out[0] = src[2 * g];
        out[1] = src[2 * g + 1];
        return out;
      } else {
        return src[g];
      }
    };
    auto unpack_to = [](F value, float (&dst)[CPT], int g) {
      if constexpr (kPack == 2) {
        dst[2 * g] = value[0];
        dst[2 * g + 1] = value[1];
      } else {
        dst[g] = value;
      }
    };
    float viol[CPT];
    if constexpr (MODE == 0) {
      StateS_<F> st[kGroups];
#pragma unroll
      for (int g = 0; g < kGroups; ++g)
        st[g] = StateS_<F>{splat<F>(x0[0]), splat<F>(x0[1]), splat<F>(x0[2]), splat<F>(0.0f), splat<F>(0.0f)};
#pragma unroll 7
      for (int i = 0; i < n; ++i) {
        float v[CPT], k[CPT];
        load_controls<LAYOUT, CPT>(a.U, p, a.N, n, i, c_run, v, k);
        const float* __restrict__ c = coef + i * kCoefS;  // wave-uniform -> scalar loads
#pragma unroll
        for (int g = 0; g < kGroups; ++g) step_spatial<F>(st[g], c, pack(v, g), pack(k, g), w);
      }
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        unpack_to(finish_spatial<F>(st[g], w), cost, g);
        unpack_to(st[g].V, viol, g);
      }
    } else {
      StateT_<F> st[kGroups];
      I nearest[kGroups];
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        st[g] = start_temporal<F>(x0, coef);
        nearest[g] = I(0);
      }
      with_search_kind(w, n, [&](auto kind) {
        for (int i = 0; i < n; ++i) {
          // A launch of ONE generation (a.even_progress, set by the launcher): the hardware issues from the oldest wave
          // first, so the eight waves of a SIMD finish one after the other - the first after half the launch, the last
          // alone, with nothing to hide its latencies behind - and the launch ends a quarter later than the SIMD's
          // instructions take.  A wave that is ahead yields instead: priority 3 in the first quarter of the horizon down to
          // 0 in the last; the waves stay within a quarter of each other and leave together (1 M candidates, one box:
          // resident share of the launch 0.57-0.73 -> 0.89, 110 -> 98 us; tools/modeT_stamps.py).  With several
          // generations the staggered ends are what overlaps a new workgroup's staging with its neighbours' arithmetic:
          // there the flag stays off (16.8 M: 1 % slower with it).
          if (a.even_progress != 0 && (i & 3) == 0) {
            const int quarter = (4 * i) / n;
            if (quarter == 0) __builtin_amdgcn_s_setprio(3);
            else if (quarter == 1) __builtin_amdgcn_s_setprio(2);
            else if (quarter == 2) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
          }
          float v[CPT], k[CPT];
          load_controls<LAYOUT, CPT>(a.U, p, a.N, n, i, c_run, v, k);
          if constexpr (decltype(kind)::value == kSearchVerified) {
            // phases across the lane's candidates: advance + window search of all (straight-line code), then the
            // wave-wide fallback for whatever was not certified, then rows and costs
            int uncertified[kGroups];
#pragma unroll
            for (int g = 0; g < kGroups; ++g) {
              temporal_advance<F>(st[g], pack(v, g), pack(k, g), w);
              nearest[g] = verified_window(st[g], s_xy, s_frames, n, nearest[g], uncertified[g]);
            }
            int any = 0;
#pragma unroll
            for (int g = 0; g < kGroups; ++g) any |= uncertified[g];
            if (__ballot(any != 0) != 0ull) {
#pragma unroll
              for (int g = 0; g < kGroups; ++g) nearest[g] = verified_fix(st[g], s_xy, n, nearest[g], uncertified[g]);
            }
#pragma unroll
            for (int g = 0; g < kGroups; ++g) temporal_settle(st[g], s_wp, nearest[g], pack(v, g), pack(k, g), w);
          } else {
#pragma unroll
            for (int g = 0; g < kGroups; ++g)
              nearest[g] = step_temporal_as<decltype(kind)::value>(st[g], s_wp, s_xy, n, pack(v, g), pack(k, g), w,
                                                                   nearest[g], s_frames);
          }
        }
      }, a.nn_frames != nullptr);
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        unpack_to(finish_temporal<F>(st[g], n, w), cost, g);
        unpack_to(st[g].V, viol, g);
      }
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) feas[j] = viol[j] == 0.0f;
    if (a.costs != nullptr && active) {
      using V = typename VecOf<CPT>::type;
      float* out = a.costs + static_cast<size_t>(p) * a.N + c0;
      if constexpr (CPT == 1) {
        out[0] = cost[0];
      } else {
        V packed;
#pragma unroll
        for (int j = 0; j < CPT; ++j) packed[j] = cost[j];
        *reinterpret_cast<V*>(out) = packed;
      }
    }
  }

  ACMPC_T_STAMP(2);
  // (cost, index) argmin: thread -> wave (shuffles) -> workgroup (LDS) -> one partial per workgroup
  int64_t key = kKeyMax;
  int nfeas = 0;
  if (active) {
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int64_t kj = pack_key(cost[j], static_cast<uint32_t>(a.index_offset + c0 + j));
      key = (kj < key) ? kj : key;
      nfeas += feas[j] ? 1 : 0;
    }
  }
  key = wave_min_key(key);
  nfeas = wave_sum_int(nfeas);
  constexpr int kWaves = BLOCK / kWave;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  if constexpr (kWaves > 1) {
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
    }
  }
  if (tid == 0) {
    const size_t slot = static_cast<size_t>(p) * gridDim.x + blockIdx.x;
    if constexpr (PUBLISH) {   // read by another workgroup of THIS launch (rollout_tailed_kernel): to the coherence point
      publish(&a.partial_keys[slot], key);
      publish(&a.partial_feas[slot], nfeas);
    } else {
      a.partial_keys[slot] = key;
      a.partial_feas[slot] = nfeas;
    }
  }
  ACMPC_T_STAMP(3);
}

template <int MODE, int LAYOUT, int CPT, int BLOCK, int PACK = (CPT >= 2 ? 2 : 1), int WAVES = 1>
__global__ void __launch_bounds__(BLOCK, WAVES) rollout_kernel(const RolloutArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  rollout_block<MODE, LAYOUT, CPT, BLOCK, PACK, false>(a, smem, static_cast<int>(blockIdx.y));
}

template <int MODE, int LAYOUT, int CPT, int BLOCK, int PACK = (CPT >= 2 ? 2 : 1), int WAVES = 1>
hipError_t launch_rollout_t(const LaunchShape& shape, const RolloutArgs& args, hipStream_t s, hipEvent_t e0,
                            hipEvent_t e1) {
  const dim3 grid(shape.blocks_per_problem, args.P);
  const size_t lds = 64 + (MODE == 1 ? (static_cast<size_t>(args.n) * (kCoefT + kKeyStride) + 3 +
                                        (args.nn_frames != nullptr ? verified_frame_floats(args.n) : 0)) * sizeof(float)
                                     : 0);
  return launch_kernel(rollout_kernel<MODE, LAYOUT, CPT, BLOCK, PACK, WAVES>, grid, dim3(BLOCK), lds, s, e0, e1, args);
}

// Candidate-major, mode S, horizons of at most NMAX steps: the tile is only PASSED THROUGH the LDS.  rollout_tile_kernel
// keeps its 8n * 64 bytes of LDS for the whole walk, which caps a CU at six waves on four SIMDs.  Here a wave loads its
// span into registers (16-byte pieces, every line once), and the WAVES waves of a workgroup take turns at ONE tile
// buffer: write the pieces, read the own row back (ds_read_b64, conflict-free for odd n) into 2n registers, hand the
// buffer on.  The walk then runs out of registers with no LDS instruction in it, at the occupancy the registers allow
// (four waves per SIMD at H = 50), while other waves of the CU are still loading.
template <int NMAX, int WAVES, bool LDS_TABLE>
__global__ void __launch_bounds__(WAVES * kWave) rollout_tile_rows_kernel(const RolloutArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_tile[];  // ONE [64][2n] tile, used by the waves in turn
  const int p = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  const int tiles = (a.N + kWave - 1) / kWave;
  const int tile = blockIdx.x * WAVES + wave;
  const bool live = tile < tiles;  // (wave-uniform; a workgroup's spare waves still take their turns at the barrier)
  const int c0 = tile * kWave;
  const int rows = live ? min(kWave, a.N - c0) : 0;
  const int n = a.n;
  const int row_floats = 2 * n;
  const Weights w = a.w;
  const float* __restrict__ coef = a.coef + static_cast<size_t>(p) * n * kCoefS;
  const float* __restrict__ x0 = a.x0 + p * 3;

  // the span starts on a 16-byte boundary (the launcher checks 2 N n % 4 == 0 or P == 1)
  const float* __restrict__ src = a.U + (static_cast<size_t>(p) * a.N + c0) * row_floats;
  const f32x4* __restrict__ src4 = reinterpret_cast<const f32x4*>(src);
  const int total = rows * row_floats;
  const int quads = total >> 2;
  constexpr int kQuads = (2 * NMAX + 3) / 4;  // 16-byte pieces per lane of a [64][2 NMAX] tile
  f32x4 raw[kQuads];
#pragma unroll
  for (int k = 0; k < kQuads; ++k) {
    const int q = lane + k * kWave;
    if (q < quads) raw[k] = __builtin_nontemporal_load(src4 + q);
  }
  f32x2 rest = {0.0f, 0.0f};
  const bool has_rest = (total & 2) != 0 && lane == 0;  // rows * n odd: one (v, kappa) pair past the last full piece
  if (has_rest) rest = *reinterpret_cast<const f32x2*>(src + (quads << 2));

  // turns at the one buffer: wave t goes after t barriers and leaves WAVES - 1 - t behind it (every wave passes the
  // same WAVES - 1 barriers; the loads above are in flight while a wave waits for its turn)
  auto handover = []() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  // The workgroup's four tiles belong to ONE problem: its table ([n][12] floats) goes into LDS once, behind the tile,
  // and the walk reads its rows from there one step ahead (every lane the same address: a broadcast).  A scalar load
  // per step misses the scalar cache (the tables of 256 problems do not fit it) and a wave then waits longer than it
  // computes: 59 % of the wave-cycles of the scalar-load form are waits.
  float* const s_table = s_tile + ((kWave * row_floats + 3) & ~3);
  if constexpr (LDS_TABLE) {
    const f32x4* __restrict__ coef4 = reinterpret_cast<const f32x4*>(coef);
    f32x4* table4 = reinterpret_cast<f32x4*>(s_table);
    for (int q = threadIdx.x; q < 3 * n; q += WAVES * kWave) table4[q] = coef4[q];
    handover();
  }
  for (int t = 0; t < wave; ++t) handover();
  {
    f32x4* dst4 = reinterpret_cast<f32x4*>(s_tile);
#pragma unroll
    for (int k = 0; k < kQuads; ++k) {
      const int q = lane + k * kWave;
      if (q < quads) dst4[q] = raw[k];
    }
    if (has_rest) *reinterpret_cast<f32x2*>(s_tile + (quads << 2)) = rest;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  f32x2 u[NMAX];
  {
    const f32x2* row = reinterpret_cast<const f32x2*>(s_tile + lane * row_floats);
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
      if (i < n) u[i] = row[i];
  }
  for (int t = wave; t < WAVES - 1; ++t) handover();

  const bool active = lane < rows;
  float cost = __builtin_inff();
  bool feas = false;
  if (active) {
    StateS st{x0[0], x0[1], x0[2], 0.0f, 0.0f};
    if constexpr (LDS_TABLE) {
      constexpr int kRowUsed = 9;
      float row_now[kRowUsed], row_next[kRowUsed];
      auto fetch = [&](float (&dst)[kRowUsed], int i) {   // (rows past n: whatever the LDS holds there, never used)
#pragma unroll
        for (int j = 0; j < kRowUsed; ++j) dst[j] = s_table[i * kCoefS + j];
      };
      fetch(row_now, 0);
#pragma unroll
      for (int i = 0; i < NMAX; ++i) {
        if (i + 1 < NMAX) fetch(row_next, i + 1);
        if (i < n) step_spatial(st, row_now, u[i][0], u[i][1], w);
#pragma unroll
        for (int j = 0; j < kRowUsed; ++j) row_now[j] = row_next[j];
      }
    } else {
#pragma unroll
      for (int i = 0; i < NMAX; ++i)
        if (i < n) step_spatial(st, coef + i * kCoefS, u[i][0], u[i][1], w);
    }
    cost = finish_spatial(st, w);
    feas = st.V == 0.0f;
    if (a.costs != nullptr) a.costs[static_cast<size_t>(p) * a.N + c0 + lane] = cost;
  }
  int64_t key = active ? pack_key(cost, static_cast<uint32_t>(a.index_offset + c0 + lane)) : kKeyMax;
  int nfeas = (active && feas) ? 1 : 0;
  key = wave_min_key(key);
  nfeas = wave_sum_int(nfeas);
  if (lane == 0 && live) {
    const size_t slot = static_cast<size_t>(p) * tiles + tile;
    a.partial_keys[slot] = key;
    a.partial_feas[slot] = nfeas;
  }
}

template <int NMAX, int WAVES, bool LDS_TABLE>
hipError_t launch_rollout_tile_rows(const LaunchShape& shape, const RolloutArgs& args, hipStream_t s, hipEvent_t e0,
                                    hipEvent_t e1) {
  const dim3 grid((shape.blocks_per_problem + WAVES - 1) / WAVES, args.P);
  // the tile, then (LDS_TABLE) the problem's table with room for NMAX rows (the walk's look-ahead reads that far)
  const size_t lds = tile_lds_bytes(0, args.n) + (LDS_TABLE ? static_cast<size_t>(NMAX + 1) * kCoefS * sizeof(float) : 0);
  return launch_kernel(rollout_tile_rows_kernel<NMAX, WAVES, LDS_TABLE>, grid, dim3(WAVES * kWave), lds, s, e0, e1, args);
}

}  // namespace

}  // namespace acmpc
