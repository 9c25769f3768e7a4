// Particle filter, everything but the scoring: the kinematic particle step (localiser.py:66-95), the weighted-mean
// estimate with its convergence numbers (localiser.py:561-579), and the device-resident filter's resampling - each with
// its launcher.
#include <hip/hip_runtime.h>

#include "acmpc_device.h"  // Philox4x32-10, uniform_open, box_muller: the sampler's generator
#include "acmpc_pf.h"

using namespace acmpc::pf;

namespace {

// states += x_dot * dt, x_dot = (v cos phi, v sin phi, v tan delta / L) in float32 as the reference computes it
// (localiser.py:66-95: float32 state array, per-particle delta and v)
__global__ void pf_advance_kernel(float* states, const float* delta, const float* velocity, int P, float wheelbase,
                                  float dt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float phi = states[3 * p + 2], v = velocity[p];
  states[3 * p] += (v * cosf(phi)) * dt;
  states[3 * p + 1] += (v * sinf(phi)) * dt;
  states[3 * p + 2] += (v * tanf(delta[p]) / wheelbase) * dt;
}

// sum(state * score) / sum(score) with the NaN -> uniform fallback, then max distance / max |yaw difference| to the
// estimate (localiser.py:561-579).  One workgroup; float64 accumulation in a fixed order.
__global__ void __launch_bounds__(kBlock) pf_estimate_kernel(const float* states, const float* scores, int P,
                                                             double* out /*[5]: x, y, yaw, max_dist, max_angle*/,
                                                             const int* live = nullptr, int* counts_out = nullptr) {
  __shared__ double s[4][kBlock];
  const int tid = threadIdx.x;
  if (live != nullptr) P = live[0];
  double acc[4] = {0, 0, 0, 0}, plain[3] = {0, 0, 0};
  for (int p = tid; p < P; p += kBlock) {
    const double w = scores[p];
    for (int c = 0; c < 3; ++c) {
      acc[c] += static_cast<double>(states[3 * p + c]) * w;
    }
    acc[3] += w;
  }
  for (int c = 0; c < 4; ++c) s[c][tid] = acc[c];
  __syncthreads();
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if (tid < half)
      for (int c = 0; c < 4; ++c) s[c][tid] += s[c][tid + half];
    __syncthreads();
  }
  double est[3] = {s[0][0] / s[3][0], s[1][0] / s[3][0], s[2][0] / s[3][0]};
  __syncthreads();
  if (est[0] != est[0] || est[1] != est[1] || est[2] != est[2]) {  // NaN: uniform weights
    for (int p = tid; p < P; p += kBlock)
      for (int c = 0; c < 3; ++c) plain[c] += static_cast<double>(states[3 * p + c]);
    for (int c = 0; c < 3; ++c) s[c][tid] = plain[c];
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
      if (tid < half)
        for (int c = 0; c < 3; ++c) s[c][tid] += s[c][tid + half];
      __syncthreads();
    }
    for (int c = 0; c < 3; ++c) est[c] = s[c][0] / static_cast<double>(P);
    __syncthreads();
  }
  double md = 0.0, ma = 0.0;
  for (int p = tid; p < P; p += kBlock) {
    const double dx = states[3 * p] - est[0], dy = states[3 * p + 1] - est[1];
    md = fmax(md, sqrt(dx * dx + dy * dy));
    ma = fmax(ma, fabs(states[3 * p + 2] - est[2]));
  }
  s[0][tid] = md;
  s[1][tid] = ma;
  __syncthreads();
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if (tid < half) {
      s[0][tid] = fmax(s[0][tid], s[0][tid + half]);
      s[1][tid] = fmax(s[1][tid], s[1][tid + half]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (counts_out != nullptr && live != nullptr)   // (the device-resident filter: its four counts beside the estimate)
      for (int e = 0; e < 4; ++e) counts_out[e] = live[e];
    out[0] = est[0];
    out[1] = est[1];
    out[2] = est[2];
    out[3] = s[0][0];
    out[4] = s[1][0];
  }
}


// ---- device-resident filter (one host round trip per update) ----------------------------------------------------------
// The reference's update cycle (localiser.py:41-77,234-239,420-579) with its random part restated on counter-based
// draws, so that it can run where the particles live:
//   step      every particle moves with its own noisy control (yaw noise on the tyre angle, |velocity + noise|)
//   update    score -> keep the valid particles in order -> too few left: reset along the centre line; otherwise top up
//             to the desired count with copies of kept particles drawn in proportion to their score (inverse CDF on a
//             prefix sum) plus Gaussian noise -> score-weighted estimate and the two convergence numbers
// The reference draws from NumPy's global Mersenne Twister in a fixed call order, which a parallel kernel cannot
// follow; `particle_filter.ParticleFilter` (NumPy resampling, the reference's draw order) therefore stays the parity
// mode, and this path is pinned by its own restatement (oracle pf_resample_counter_based): the weights are integers
// (floor(score * 2^40)), so the prefix sums, the draws (mulhi of a 64-bit Philox word with the total) and the picked
// indices are exact in any summation order.
constexpr uint32_t kTagResample = 0x52534d50u;  // "RSMP"
constexpr uint32_t kTagControl = 0x4354524cu;   // "CTRL"

__device__ __forceinline__ unsigned long long weight_of(double score) {
  // floor(score * 2^40) for finite positive scores, 0 otherwise (NaN, negative); scores are <= 1 by construction
  if (!(score > 0.0)) return 0ull;
  const double scaled = score * 1099511627776.0;
  return scaled >= 1.8446744073709552e19 ? 0xffffffffffffffffull : static_cast<unsigned long long>(scaled);
}

// exclusive prefix sum of one value per thread over the workgroup (kScanBlock threads); returns the offset, *total
__device__ unsigned long long block_exclusive_scan(unsigned long long v, unsigned long long* s_scan,
                                                   unsigned long long* total) {
  const int tid = threadIdx.x;
  s_scan[tid] = v;
  __syncthreads();
  for (int off = 1; off < kScanBlock; off <<= 1) {
    const unsigned long long add = (tid >= off) ? s_scan[tid - off] : 0ull;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  *total = s_scan[kScanBlock - 1];
  const unsigned long long inclusive = s_scan[tid];
  __syncthreads();
  return inclusive - v;
}

__global__ void __launch_bounds__(kScanBlock) pf_resample_kernel(const FilterArgs a) {
  __shared__ unsigned long long s_scan[kScanBlock];
  const int tid = threadIdx.x;
  const int n = a.counts[0];
  const int chunk = (n + kScanBlock - 1) / kScanBlock;
  const int begin = min(tid * chunk, n), end = min(begin + chunk, n);
  // 1. stable compaction of the valid particles
  unsigned long long local = 0ull, total = 0ull;
  for (int p = begin; p < end; ++p) local += a.valid[p] ? 1ull : 0ull;
  unsigned long long offset = block_exclusive_scan(local, s_scan, &total);
  const int n_valid = static_cast<int>(total);
  for (int p = begin; p < end; ++p)
    if (a.valid[p]) a.kept[offset++] = p;
  __syncthreads();
  __threadfence_block();
  if (n_valid < a.minimum_particles) {
    // _reset_filter (localiser.py:468-485): spread evenly along the centre line, heading along it, uniform scores
    const int count = a.capacity;
    for (int k = tid; k < count; k += kScanBlock) {
      // np.linspace(0, m - 3, count).astype(int32)
      const double pos = (count > 1) ? static_cast<double>(k) * (static_cast<double>(a.m_centre - 3) / static_cast<double>(count - 1))
                                     : 0.0;
      int idx = static_cast<int>((k == count - 1 && count > 1) ? static_cast<double>(a.m_centre - 3) : pos);
      const double x = a.centre[2 * idx], y = a.centre[2 * idx + 1];
      const double yaw = atan2(a.centre[2 * (idx + 1) + 1] - y, a.centre[2 * (idx + 1)] - x);
      a.states_out[3 * k] = static_cast<float>(x);
      a.states_out[3 * k + 1] = static_cast<float>(y);
      a.states_out[3 * k + 2] = static_cast<float>(yaw);
      a.scores_out[k] = 1.0f / static_cast<float>(count);
    }
    if (tid == 0) {
      a.counts[0] = count;
      a.counts[1] = n_valid;
      a.counts[2] = 1;
    }
    return;
  }
  // 2. integer weights of the kept particles and their inclusive prefix sums (exact: order does not matter)
  const int kchunk = (n_valid + kScanBlock - 1) / kScanBlock;
  const int kb = min(tid * kchunk, n_valid), ke = min(kb + kchunk, n_valid);
  local = 0ull;
  for (int k = kb; k < ke; ++k) local += weight_of(a.score[a.kept[k]]);
  unsigned long long wtotal = 0ull;
  offset = block_exclusive_scan(local, s_scan, &wtotal);
  const bool uniform = wtotal == 0ull;   // all scores zero / NaN: uniform weights (localiser.py:523-526)
  if (uniform) {
    offset = static_cast<unsigned long long>(kb);
    wtotal = static_cast<unsigned long long>(n_valid);
  }
  for (int k = kb; k < ke; ++k) {
    offset += uniform ? 1ull : weight_of(a.score[a.kept[k]]);
    a.cdf[k] = offset;
  }
  __syncthreads();
  __threadfence_block();
  // 3. kept particles first, in order
  for (int k = tid; k < n_valid; k += kScanBlock) {
    const int p = a.kept[k];
    a.states_out[3 * k] = a.states_in[3 * p];
    a.states_out[3 * k + 1] = a.states_in[3 * p + 1];
    a.states_out[3 * k + 2] = a.states_in[3 * p + 2];
    a.scores_out[k] = a.scores_in[p];
  }
  // 4. top up: new particle j = kept[upper_bound(cdf, mulhi(r, total))] + noise
  const int n_new = max(0, min(a.n_desired, a.capacity) - n_valid);
  const uint32_t key[2] = {a.seed_lo, a.seed_hi};
  for (int j = tid; j < n_new; j += kScanBlock) {
    const uint32_t c_pick[4] = {static_cast<uint32_t>(j), a.counter, kTagResample, 0u};
    const uint32_t c_noise[4] = {static_cast<uint32_t>(j), a.counter, kTagResample, 1u};
    uint32_t r[4], q[4];
    acmpc::philox4x32_10(c_pick, key, r);
    acmpc::philox4x32_10(c_noise, key, q);
    const unsigned long long word = (static_cast<unsigned long long>(r[0]) << 32) | r[1];
    const unsigned long long target = __umul64hi(word, wtotal);   // uniform in [0, total)
    int lo = 0, hi = n_valid - 1;                                   // first k with cdf[k] > target
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    const int p = a.kept[lo];
    float z0, z1, z2, z3;
    acmpc::box_muller(acmpc::uniform_open(q[0]), acmpc::uniform_open(q[1]), z0, z1);
    acmpc::box_muller(acmpc::uniform_open(q[2]), acmpc::uniform_open(q[3]), z2, z3);
    (void)z3;
    const int k = n_valid + j;
    a.states_out[3 * k] = static_cast<float>(static_cast<double>(a.states_in[3 * p]) + a.sigma_x * static_cast<double>(z0));
    a.states_out[3 * k + 1] =
        static_cast<float>(static_cast<double>(a.states_in[3 * p + 1]) + a.sigma_y * static_cast<double>(z1));
    a.states_out[3 * k + 2] =
        static_cast<float>(static_cast<double>(a.states_in[3 * p + 2]) + a.sigma_yaw * static_cast<double>(z2));
    a.scores_out[k] = a.scores_in[p];
  }
  if (tid == 0) {
    a.counts[0] = n_valid + n_new;
    a.counts[1] = n_valid;
    a.counts[2] = 0;
  }
}

// ---- the same update for many particles (capacity >= kWideFilter): pf_resample_kernel and pf_estimate_kernel are ONE
// workgroup each, which is what the reference's hundreds of particles want (8 us) and what 100 000 do not (607 + 214 us: a
// thread walks ~100 particles of its own, a cache line apart from its neighbour's).  Here every step is a launch over tiles
// of kScanBlock particles, a particle per thread:
//   tiles    per tile: how many valid particles, the sum of their integer weights
//   plan     one workgroup: exclusive prefix sums of the tiles' counts and weights; reset or not; the new counts
//   scatter  per tile: the kept particles' places (stable: tile offset + rank inside the tile) and their inclusive weight sums
//   emit     a thread per output particle: kept ones copied in order, new ones drawn (same draws, same binary search)
// The integers - ranks, prefix sums, picks - are those of the one-workgroup kernel exactly; so are the particles.
__global__ void __launch_bounds__(kScanBlock) pf_resample_tiles_kernel(const FilterArgs a, const WideScratch w) {
  __shared__ unsigned long long s_scan[kScanBlock];
  const int n = a.counts[0];
  const int p = blockIdx.x * kScanBlock + threadIdx.x;
  const bool keep = p < n && a.valid[p] != 0;
  unsigned long long count = 0ull, weight = 0ull;
  (void)block_exclusive_scan(keep ? 1ull : 0ull, s_scan, &count);
  (void)block_exclusive_scan(keep ? weight_of(a.score[p]) : 0ull, s_scan, &weight);
  if (threadIdx.x == 0) {
    w.tile_count[blockIdx.x] = count;
    w.tile_weight[blockIdx.x] = weight;
  }
}

// (tiles <= kScanBlock: capacities up to 2^20 particles; beyond, the one-workgroup kernels serve)
__global__ void __launch_bounds__(kScanBlock) pf_resample_plan_kernel(const FilterArgs a, const WideScratch w, const int tiles) {
  __shared__ unsigned long long s_scan[kScanBlock];
  const int tid = threadIdx.x;
  const unsigned long long count = tid < tiles ? w.tile_count[tid] : 0ull;
  const unsigned long long weight = tid < tiles ? w.tile_weight[tid] : 0ull;
  unsigned long long n_valid = 0ull, total = 0ull;
  const unsigned long long count_before = block_exclusive_scan(count, s_scan, &n_valid);
  const unsigned long long weight_before = block_exclusive_scan(weight, s_scan, &total);
  if (tid < tiles) {
    w.tile_count[tid] = count_before;
    w.tile_weight[tid] = weight_before;
  }
  if (tid == 0) {
    const bool reset = static_cast<int>(n_valid) < a.minimum_particles;
    const bool uniform = total == 0ull;   // all scores zero / NaN: uniform weights (localiser.py:523-526)
    const int n_new = reset ? 0 : max(0, min(a.n_desired, a.capacity) - static_cast<int>(n_valid));
    w.meta[0] = static_cast<unsigned long long>(a.counts[0]);
    w.meta[1] = n_valid;
    w.meta[2] = uniform ? n_valid : total;
    w.meta[3] = uniform ? 1ull : 0ull;
    w.meta[4] = reset ? 1ull : 0ull;
    w.meta[5] = static_cast<unsigned long long>(n_new);
    a.counts[0] = reset ? a.capacity : static_cast<int>(n_valid) + n_new;
    a.counts[1] = static_cast<int>(n_valid);
    a.counts[2] = reset ? 1 : 0;
  }
}

__global__ void __launch_bounds__(kScanBlock) pf_resample_scatter_kernel(const FilterArgs a, const WideScratch w) {
  __shared__ unsigned long long s_scan[kScanBlock];
  if (w.meta[4] != 0ull) return;   // reset: nothing is kept
  const int n = static_cast<int>(w.meta[0]);
  const bool uniform = w.meta[3] != 0ull;
  const int p = blockIdx.x * kScanBlock + threadIdx.x;
  const bool keep = p < n && a.valid[p] != 0;
  const unsigned long long weight = keep ? weight_of(a.score[p]) : 0ull;
  unsigned long long unused = 0ull;
  const unsigned long long rank = block_exclusive_scan(keep ? 1ull : 0ull, s_scan, &unused);
  const unsigned long long before = block_exclusive_scan(weight, s_scan, &unused);
  if (keep) {
    const unsigned long long k = w.tile_count[blockIdx.x] + rank;
    a.kept[k] = p;
    a.cdf[k] = uniform ? k + 1ull : w.tile_weight[blockIdx.x] + before + weight;
  }
}

__global__ void __launch_bounds__(256) pf_resample_emit_kernel(const FilterArgs a, const WideScratch w) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (w.meta[4] != 0ull) {
    // _reset_filter (localiser.py:468-485): spread evenly along the centre line, heading along it, uniform scores
    const int count = a.capacity;
    if (idx >= count) return;
    const int k = idx;
    const double pos = (count > 1) ? static_cast<double>(k) * (static_cast<double>(a.m_centre - 3) / static_cast<double>(count - 1))
                                   : 0.0;
    const int at = static_cast<int>((k == count - 1 && count > 1) ? static_cast<double>(a.m_centre - 3) : pos);
    const double x = a.centre[2 * at], y = a.centre[2 * at + 1];
    const double yaw = atan2(a.centre[2 * (at + 1) + 1] - y, a.centre[2 * (at + 1)] - x);
    a.states_out[3 * k] = static_cast<float>(x);
    a.states_out[3 * k + 1] = static_cast<float>(y);
    a.states_out[3 * k + 2] = static_cast<float>(yaw);
    a.scores_out[k] = 1.0f / static_cast<float>(count);
    return;
  }
  const int n_valid = static_cast<int>(w.meta[1]), n_new = static_cast<int>(w.meta[5]);
  const unsigned long long wtotal = w.meta[2];
  if (idx < n_valid) {   // kept particles first, in order
    const int p = a.kept[idx];
    a.states_out[3 * idx] = a.states_in[3 * p];
    a.states_out[3 * idx + 1] = a.states_in[3 * p + 1];
    a.states_out[3 * idx + 2] = a.states_in[3 * p + 2];
    a.scores_out[idx] = a.scores_in[p];
  }
  if (idx < n_new) {   // top up: new particle j = kept[upper_bound(cdf, mulhi(r, total))] + noise
    const int j = idx;
    const uint32_t key[2] = {a.seed_lo, a.seed_hi};
    const uint32_t c_pick[4] = {static_cast<uint32_t>(j), a.counter, kTagResample, 0u};
    const uint32_t c_noise[4] = {static_cast<uint32_t>(j), a.counter, kTagResample, 1u};
    uint32_t r[4], q[4];
    acmpc::philox4x32_10(c_pick, key, r);
    acmpc::philox4x32_10(c_noise, key, q);
    const unsigned long long word = (static_cast<unsigned long long>(r[0]) << 32) | r[1];
    const unsigned long long target = __umul64hi(word, wtotal);   // uniform in [0, total)
    int lo = 0, hi = n_valid - 1;                                   // first k with cdf[k] > target
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    const int p = a.kept[lo];
    float z0, z1, z2, z3;
    acmpc::box_muller(acmpc::uniform_open(q[0]), acmpc::uniform_open(q[1]), z0, z1);
    acmpc::box_muller(acmpc::uniform_open(q[2]), acmpc::uniform_open(q[3]), z2, z3);
    (void)z3;
    const int k = n_valid + j;
    a.states_out[3 * k] = static_cast<float>(static_cast<double>(a.states_in[3 * p]) + a.sigma_x * static_cast<double>(z0));
    a.states_out[3 * k + 1] =
        static_cast<float>(static_cast<double>(a.states_in[3 * p + 1]) + a.sigma_y * static_cast<double>(z1));
    a.states_out[3 * k + 2] =
        static_cast<float>(static_cast<double>(a.states_in[3 * p + 2]) + a.sigma_yaw * static_cast<double>(z2));
    a.scores_out[k] = a.scores_in[p];
  }
}

// The estimate of pf_estimate_kernel for many particles: partial sums per workgroup of kEstimateTile particles (float64, a
// fixed order: thread, then the tree of the workgroup, then the workgroups in turn), the spread against the estimate in a
// second launch, its maximum in a third.
__global__ void __launch_bounds__(kBlock) pf_estimate_partial_kernel(const float* states, const float* scores, const int* live,
                                                                     double* partial /*[tiles][8]*/) {
  __shared__ double s[7][kBlock];
  const int tid = threadIdx.x;
  const int P = live[0];
  const int begin = blockIdx.x * kEstimateTile, end = min(begin + kEstimateTile, P);
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};   // sum(state * score) x 3, sum(score), sum(state) x 3
  for (int p = begin + tid; p < end; p += kBlock) {
    const double wgt = scores[p];
    for (int c = 0; c < 3; ++c) {
      const double v = static_cast<double>(states[3 * p + c]);
      acc[c] += v * wgt;
      acc[4 + c] += v;
    }
    acc[3] += wgt;
  }
  for (int c = 0; c < 7; ++c) s[c][tid] = acc[c];
  __syncthreads();
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if (tid < half)
      for (int c = 0; c < 7; ++c) s[c][tid] += s[c][tid + half];
    __syncthreads();
  }
  if (tid < 7) partial[8 * blockIdx.x + tid] = s[tid][0];
}

__device__ __forceinline__ void estimate_from_partials(const double* partial, int tiles, int P, double est[3]) {
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int t = 0; t < tiles; ++t)
    for (int c = 0; c < 7; ++c) acc[c] += partial[8 * t + c];
  for (int c = 0; c < 3; ++c) est[c] = acc[c] / acc[3];
  if (est[0] != est[0] || est[1] != est[1] || est[2] != est[2])   // NaN: uniform weights
    for (int c = 0; c < 3; ++c) est[c] = acc[4 + c] / static_cast<double>(P);
}

__global__ void __launch_bounds__(kBlock) pf_estimate_spread_kernel(const float* states, const int* live, const double* partial,
                                                                    double* spread /*[tiles][2]*/) {
  __shared__ double s[2][kBlock];
  __shared__ double s_est[3];
  const int tid = threadIdx.x;
  const int P = live[0];
  const int tiles = (P + kEstimateTile - 1) / kEstimateTile;
  if (tid == 0) {
    double est[3];
    estimate_from_partials(partial, tiles, P, est);
    for (int c = 0; c < 3; ++c) s_est[c] = est[c];
  }
  __syncthreads();
  const double ex = s_est[0], ey = s_est[1], ez = s_est[2];
  const int begin = blockIdx.x * kEstimateTile, end = min(begin + kEstimateTile, P);
  double md = 0.0, ma = 0.0;
  for (int p = begin + tid; p < end; p += kBlock) {
    const double dx = states[3 * p] - ex, dy = states[3 * p + 1] - ey;
    md = fmax(md, sqrt(dx * dx + dy * dy));
    ma = fmax(ma, fabs(states[3 * p + 2] - ez));
  }
  s[0][tid] = md;
  s[1][tid] = ma;
  __syncthreads();
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if (tid < half) {
      s[0][tid] = fmax(s[0][tid], s[0][tid + half]);
      s[1][tid] = fmax(s[1][tid], s[1][tid + half]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    spread[2 * blockIdx.x] = s[0][0];
    spread[2 * blockIdx.x + 1] = s[1][0];
  }
}

__global__ void __launch_bounds__(kBlock) pf_estimate_final_kernel(const int* live, const double* partial, const double* spread,
                                                                   double* out /*[5]*/, int* counts_out) {
  __shared__ double s[2][kBlock];
  const int tid = threadIdx.x;
  const int P = live[0];
  const int tiles = (P + kEstimateTile - 1) / kEstimateTile;
  double md = 0.0, ma = 0.0;
  for (int t = tid; t < tiles; t += kBlock) {
    md = fmax(md, spread[2 * t]);
    ma = fmax(ma, spread[2 * t + 1]);
  }
  s[0][tid] = md;
  s[1][tid] = ma;
  __syncthreads();
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if (tid < half) {
      s[0][tid] = fmax(s[0][tid], s[0][tid + half]);
      s[1][tid] = fmax(s[1][tid], s[1][tid + half]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    double est[3];
    estimate_from_partials(partial, tiles, P, est);
    if (counts_out != nullptr)
      for (int e = 0; e < 4; ++e) counts_out[e] = live[e];
    out[0] = est[0];
    out[1] = est[1];
    out[2] = est[2];
    out[3] = s[0][0];
    out[4] = s[1][0];
  }
}

// Localiser.step (localiser.py:41-77): delta = tyre_angle + N(0, sigma_yaw), speed = |velocity + N(0, sigma_v)| per
// particle from Philox (counter = particle, step), then the float32 kinematic step of pf_advance_kernel
__global__ void pf_step_kernel(float* states, const int* counts, float tyre_angle, float velocity, float sigma_yaw,
                               float sigma_v, float wheelbase, float dt, uint32_t seed_lo, uint32_t seed_hi,
                               uint32_t counter) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= counts[0]) return;
  const uint32_t ctr[4] = {static_cast<uint32_t>(p), counter, kTagControl, 0u};
  const uint32_t key[2] = {seed_lo, seed_hi};
  uint32_t r[4];
  acmpc::philox4x32_10(ctr, key, r);
  float z0, z1;
  acmpc::box_muller(acmpc::uniform_open(r[0]), acmpc::uniform_open(r[1]), z0, z1);
  const float delta = tyre_angle + sigma_yaw * z0;
  const float v = fabsf(velocity + sigma_v * z1);
  const float phi = states[3 * p + 2];
  states[3 * p] += (v * cosf(phi)) * dt;
  states[3 * p + 1] += (v * sinf(phi)) * dt;
  states[3 * p + 2] += (v * tanf(delta) / wheelbase) * dt;
}

}  // namespace

namespace acmpc::pf {

void launch_advance(float* states, const float* delta, const float* velocity, int P, float wheelbase, float dt, hipStream_t s) {
  hipLaunchKernelGGL(pf_advance_kernel, dim3((P + 255) / 256), dim3(256), 0, s, states, delta, velocity, P, wheelbase, dt);
}

// (a thread per particle of the capacity: those beyond the live count return at once)
void launch_step(const acmpc_pf* h, float tyre_angle, float velocity, float sigma_yaw, float sigma_v, float dt, uint64_t seed,
                 uint32_t counter) {
  const int P = h->prm.max_particles;
  hipLaunchKernelGGL(pf_step_kernel, dim3((P + 255) / 256), dim3(256), 0, h->stream, h->f_states[h->f_cur], h->f_counts,
                     tyre_angle, velocity, sigma_yaw, sigma_v, static_cast<float>(h->prm.wheelbase), dt,
                     static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), counter);
}

// the one-workgroup resampling kernel, which resets where too few particles are valid: all of them, with `f` as
// acmpc_pf_filter_reset fills it (n_live = 0, minimum_particles = 1)
void launch_reset(const FilterArgs& f, hipStream_t s) {
  hipLaunchKernelGGL(pf_resample_kernel, dim3(1), dim3(kScanBlock), 0, s, f);
}

void launch_resample(const acmpc_pf* h, const FilterArgs& f, bool wide, hipStream_t s) {
  if (!wide) return launch_reset(f, s);
  const size_t Pmax = h->prm.max_particles;
  const int tiles = static_cast<int>((Pmax + kScanBlock - 1) / kScanBlock);
  const WideScratch w{h->f_wide, h->f_wide + tiles, h->f_wide + 2 * tiles};
  hipLaunchKernelGGL(pf_resample_tiles_kernel, dim3(tiles), dim3(kScanBlock), 0, s, f, w);
  hipLaunchKernelGGL(pf_resample_plan_kernel, dim3(1), dim3(kScanBlock), 0, s, f, w, tiles);
  hipLaunchKernelGGL(pf_resample_scatter_kernel, dim3(tiles), dim3(kScanBlock), 0, s, f, w);
  hipLaunchKernelGGL(pf_resample_emit_kernel, dim3(static_cast<unsigned>((Pmax + 255) / 256)), dim3(256), 0, s, f, w);
}

void launch_estimate(const acmpc_pf* h, bool wide, const float* states, const float* scores, int P, const int* live,
                     double* out, int* counts_out, hipStream_t s) {
  if (!wide) {
    hipLaunchKernelGGL(pf_estimate_kernel, dim3(1), dim3(kBlock), 0, s, states, scores, P, out, live, counts_out);
    return;
  }
  const size_t Pmax = h->prm.max_particles;
  const int sums = static_cast<int>((Pmax + kEstimateTile - 1) / kEstimateTile);
  double* spread = h->f_partial + static_cast<size_t>(sums) * 8;
  hipLaunchKernelGGL(pf_estimate_partial_kernel, dim3(sums), dim3(kBlock), 0, s, states, scores, live, h->f_partial);
  hipLaunchKernelGGL(pf_estimate_spread_kernel, dim3(sums), dim3(kBlock), 0, s, states, live, h->f_partial, spread);
  hipLaunchKernelGGL(pf_estimate_final_kernel, dim3(1), dim3(kBlock), 0, s, live, h->f_partial, spread, out, counts_out);
}

}  // namespace acmpc::pf
