// What the translation units of the gfx950 rollout-and-cost kernels share: the architecture guard, small device helpers,
// the phase-stamp macros of the A/B tools, and the host side's launch plumbing.  Internal: included only by those units
// (acmpc_rollout / _kernels_temporal / _kernels / _solo / _softmin .hip; which holds what: DESIGN.md section 4), directly or
// through acmpc_rollout.h, and by mode D's (acmpc_dynamic*.hip) through acmpc_dynamic_kernels.h for the launch plumbing.  Built with -ffp-contract=off: see acmpc_device.h.
#pragma once
#include "acmpc_kernels.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#pragma clang fp contract(off)

// gfx950 (MI355X) only, on purpose.  Three things in these units lean on what that hardware does rather than on what HIP
// promises, and must not be compiled for anything else without being revisited:
//   - the multi-wave rounds and the one-launch solve let waves of a workgroup END while the others keep meeting at
//     s_barrier (rollout_sampled_trio / quad / pair kernels in acmpc_kernels.hip, rollout_solo_kernel<SPLIT> in
//     acmpc_solo.hip): the hardware takes a terminated wave out of the barrier's count, HIP leaves a barrier that not
//     every thread reaches undefined;
//   - values that cross workgroups inside a launch are published with relaxed agent-scope atomics ordered by s_waitcnt
//     vmcnt(0) (publish / observe / published / last_workgroup_of_problem below): sound because an sc1
//     store is acknowledged at the memory-side coherence point on gfx942 / gfx950, a data race under the HSA memory model;
//   - the DPP reductions spell out the wait states the hazard recogniser would insert (acmpc_device.h).
// Every unit with device code includes this header, so every one of them refuses another architecture.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "acmpc kernels are written for gfx950 (MI355X): see the note above before building for another architecture"
#endif

namespace acmpc {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Phase stamps for tools/archive/solo_probe.hip (a standalone build of acmpc_solo.hip with -DACMPC_STAMPS); nothing in the library.
#ifdef ACMPC_STAMPS
__device__ unsigned long long g_stamps[4096 * 16];
#define ACMPC_STAMP(slot)                                                                                         \
  do {                                                                                                            \
    if ((threadIdx.x & 63) == 0)                                                                                  \
      g_stamps[((blockIdx.y * gridDim.x + blockIdx.x) * 2 + (threadIdx.x >> 6)) * 16 + (slot)] = wall_clock64(); \
  } while (0)
#else
#define ACMPC_STAMP(slot) \
  do {                    \
  } while (0)
#endif

template <int CPT>
struct VecOf;
template <>
struct VecOf<1> {
  using type = float;
};
template <>
struct VecOf<2> {
  using type = f32x2;
};
template <>
struct VecOf<4> {
  using type = f32x4;
};

template <int CPT>
__device__ __forceinline__ void unpack(const typename VecOf<CPT>::type& v, float (&out)[CPT]) {
  if constexpr (CPT == 1) {
    out[0] = v;
  } else {
#pragma unroll
    for (int j = 0; j < CPT; ++j) out[j] = v[j];
  }
}

// Controls of CPT adjacent candidates at step i.
template <int LAYOUT, int CPT>
__device__ __forceinline__ void load_controls(const float* __restrict__ U, int p, int N, int n, int i, int c0,
                                              float (&v)[CPT], float (&k)[CPT]) {
  if constexpr (LAYOUT == 1) {
    // U[p][i][0|1][c]: lanes read consecutive candidates -> one fully coalesced wave access per component
    using V = typename VecOf<CPT>::type;
    const float* row = U + (static_cast<size_t>(p) * n + i) * 2 * static_cast<size_t>(N) + c0;
    unpack<CPT>(__builtin_nontemporal_load(reinterpret_cast<const V*>(row)), v);
    unpack<CPT>(__builtin_nontemporal_load(reinterpret_cast<const V*>(row + N)), k);
  } else {
    // U[p][c][i][0|1]: 8-byte (v, kappa) pairs at a row stride of 8n bytes
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const f32x2 vk = *reinterpret_cast<const f32x2*>(U + ((static_cast<size_t>(p) * N + c0 + j) * n + i) * 2);
      v[j] = vk[0];
      k[j] = vk[1];
    }
  }
}

// Publishing between workgroups of ONE launch without fences.  An agent-scope fence is an L2 write-back (release) or an
// L2 invalidate (acquire) on this multi-die part - microseconds each, and the fused finalize needed three per
// workgroup.  Instead the few values that cross workgroups (partial keys, traces, tickets) are written and read with
// agent-scope atomic stores / loads, which go to the memory-side coherence point past the per-die L2, and a writer
// only has to wait until its stores have been acknowledged (vmcnt = 0) before it takes its ticket.
template <typename T>
__device__ __forceinline__ void publish(T* where, T value) {
  __hip_atomic_store(where, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ T observe(const T* where) {
  return __hip_atomic_load(where, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void published() {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): every store of this wave has been acknowledged
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// Last-workgroup-done, in two levels: a workgroup publishes its partials (and trace) device-wide and takes a ticket of
// its group (workgroup index mod `groups`); the last of a group takes a ticket of the problem; the last of those knows
// every workgroup's results are at the coherence point (each waited for its stores before its increment) and
// finalizes.  Two levels because a device-scope atomic on one address takes ~13 ns and they serialise: 256 workgroups
// finishing together would queue for 3 us on one counter, and queue for 0.5 us on 8 + 1.  `tickets` - this problem's
// [groups + 1] counters, kTicketStride ints apart - is zero before the launch and after it.  Called by one whole wave whose threadIdx.x are its
// lanes; true (wave-uniform) on the wave that may read what the others published.
//
// Memory model: the values that cross workgroups are written and read with relaxed agent-scope atomics and ordered by
// s_waitcnt vmcnt(0) on the writer's side (published()) and by the ticket's data dependence on the reader's.  That
// relies on gfx942 / gfx950 hardware - an agent-scope (sc1) store is acknowledged only once it is at the memory-side
// coherence point, and agent-scope loads are served from there - not on the HSA memory model, under which it is a
// data race.  The signal fences keep the COMPILER from moving the reader's loads above the ticket.  On any other
// architecture: ACMPC_NO_CHAINED_ROUNDS / ACMPC_NO_TRACED_FINALIZE / ACMPC_NO_SOLO select the forms without it.
__device__ __forceinline__ bool last_workgroup_of_problem(int* tickets, const int groups_cfg) {
  const int blocks = static_cast<int>(gridDim.x);
  const int group = static_cast<int>(blockIdx.x) & (groups_cfg - 1);   // groups_cfg is a power of two
  const int group_size = (blocks - group + groups_cfg - 1) / groups_cfg;
  const int groups = min(blocks, groups_cfg);
  published();   // partial key, feasible count and trace of this workgroup are at the coherence point
  ACMPC_STAMP(5);
  int ticket = 0;
  if (threadIdx.x == 0) ticket = atomicAdd(&tickets[group * kTicketStride], 1);
  ticket = __builtin_amdgcn_readfirstlane(ticket);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  if (ticket != group_size - 1) return false;
  ACMPC_STAMP(6);
  if (threadIdx.x == 0) {
    publish(&tickets[group * kTicketStride], 0);
    ticket = atomicAdd(&tickets[groups_cfg * kTicketStride], 1);
  }
  ticket = __builtin_amdgcn_readfirstlane(ticket);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  if (ticket != groups - 1) return false;
  ACMPC_STAMP(7);
  if (threadIdx.x == 0) publish(&tickets[groups_cfg * kTicketStride], 0);  // the launch leaves the counters as it found them
  return true;
}

// Candidate 2 of a sampled round is the LQ plan (SampleArgs::u_extra) - ONE candidate of the launch, in one workgroup.
// The plan is read in place from pinned HOST memory (the tick's host computes it while the first round runs): only the
// workgroup that holds global index 2 fetches it.  With every workgroup staging it the last round of a tick moved
// 256 x 392 B over PCIe for one lane's sake - two microseconds of its fourteen.
__device__ __forceinline__ bool holds_candidate_2(const RolloutArgs& a, const SampleArgs& smp) {
  const int64_t first = a.index_offset + static_cast<int64_t>(blockIdx.x) * kWave;
  return smp.u_extra != nullptr && first <= 2 && 2 < first + kWave;
}

// Phase stamps of the mode T rollout for tools/modeT_stamps.py (a scratch build of the library with -DACMPC_T_STAMPS,
// tools/ab_build.sh): lane 0 of every wave stamps the 100 MHz wall clock at entry, after the tables are staged, after the
// step loop and at its end, and leaves its place on the chip (XCC_ID, HW_ID) beside them.  Nothing in the library.
#ifdef ACMPC_T_STAMPS
constexpr int kStampWaves = 1 << 17;
__device__ unsigned long long g_t_stamps[kStampWaves * 6];
#define ACMPC_T_STAMP(slot)                                                                                      \
  do {                                                                                                           \
    if constexpr (MODE == 1) {                                                                                   \
      const unsigned wave_ = (blockIdx.y * gridDim.x + blockIdx.x) * (BLOCK / kWave) + (threadIdx.x / kWave);   \
      if ((threadIdx.x & (kWave - 1)) == 0 && wave_ < kStampWaves) {                                             \
        g_t_stamps[wave_ * 6 + (slot)] = wall_clock64();                                                         \
        if ((slot) == 0) {                                                                                       \
          g_t_stamps[wave_ * 6 + 4] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);   /* HW_ID */         \
          g_t_stamps[wave_ * 6 + 5] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);   /* XCC_ID */        \
        }                                                                                                        \
      }                                                                                                          \
    }                                                                                                            \
  } while (0)
#else
#define ACMPC_T_STAMP(slot) \
  do {                      \
  } while (0)
#endif

// lane `lane`'s value in every lane (v_readlane: an SGPR)
__device__ __forceinline__ float bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__device__ __forceinline__ float key_cost(int64_t key) {
  const int32_t hi = static_cast<int32_t>(key >> 32);
  union {
    int32_t i;
    float f;
  } b;
  b.i = (hi >= 0) ? hi : (hi ^ 0x7fffffff);
  return b.f;
}

// hipGetLastError() returns (and clears) the last error of ANY earlier runtime call of the thread - a failed
// allocation of this or another library minutes ago included.  Launch status is read with it, so clear it first:
// once at the top of every public launcher.
inline void clear_stale_error() { (void)hipGetLastError(); }

// One dispatch and its status.  With `e0` and `e1` (both or neither) the events are attached to the dispatch itself
// (hipExtLaunchKernelGGL): the kernel's own begin and end timestamps, with no marker packets added to the stream.
template <typename Kernel, typename... Args>
hipError_t launch_kernel(Kernel kernel, const dim3 grid, const dim3 block, const size_t lds, hipStream_t s, hipEvent_t e0,
                         hipEvent_t e1, const Args&... args) {
  if (e0 != nullptr && e1 != nullptr) {
    hipExtLaunchKernelGGL(kernel, grid, block, static_cast<std::uint32_t>(lds), s, e0, e1, 0, args...);
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  }
  return hipGetLastError();
}

// More dynamic LDS than a kernel gets by default (64 kB): raise the limit, once per kernel (its own `raised`) and device.
template <auto kKernel>
hipError_t raise_lds_limit(const size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  static bool raised[64] = {};
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  if (device < 0 || device >= 64) return hipErrorInvalidDevice;
  if (!raised[device]) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    raised[device] = true;
  }
  return hipSuccess;
}

// launch_kernel for the kernels whose LDS image may be beyond the default limit
template <auto kKernel, typename... Args>
hipError_t launch_kernel_lds(const dim3 grid, const dim3 block, const size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                             const Args&... args) {
  const hipError_t e = raise_lds_limit<kKernel>(lds);
  if (e != hipSuccess) return e;
  return launch_kernel(kKernel, grid, block, lds, s, e0, e1, args...);
}

}  // namespace

}  // namespace acmpc
