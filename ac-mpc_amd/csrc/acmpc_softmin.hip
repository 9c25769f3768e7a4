// softmin_*: the score-weighted mean of the control sequences, over a control matrix or over candidates re-drawn from
// their indices.
#include "acmpc_kernels_impl.h"

namespace acmpc {

namespace {

// ---- softmin-weighted mean -------------------------------------------------------------------------------
constexpr int kSoftChunk = 1024;  // candidates per workgroup
constexpr int kSoftBlock = 256;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// the weight of one candidate against the minimum cost of its problem; 0 for a non-finite cost.  ONE function for the
// two partial kernels below: their weights are the same bits.
__device__ __forceinline__ float softmin_weight(float cost, float cmin, float lambda) {
  const bool finite = (__float_as_uint(cost) & 0x7f800000u) != 0x7f800000u;
  return finite ? expf(-(cost - cmin) / lambda) : 0.0f;
}

// partial[p][chunk][0] = sum of weights; [1 .. 2n] = weighted sums; [2n+1 .. 4n] = unweighted sums.
template <int LAYOUT>
__global__ void __launch_bounds__(kSoftBlock) softmin_partial_kernel(const SoftminArgs a) {
  __shared__ float s_w[kSoftChunk];
  __shared__ double s_red[kSoftBlock / kWave];
  __shared__ double s_acc[2][kSoftBlock];
  const int p = blockIdx.y;
  const int chunk = blockIdx.x;
  const int tid = threadIdx.x;
  const int n2 = 2 * a.n;
  const int base = chunk * kSoftChunk;
  const int count = min(kSoftChunk, a.N - base);
  const float cmin = key_cost(a.keys[p]);
  const float* __restrict__ costs = a.costs + static_cast<size_t>(p) * a.N + base;
  double* __restrict__ out = a.partial + (static_cast<size_t>(p) * a.chunks + chunk) * (2 * n2 + 1);

  double wsum = 0.0;
  for (int c = tid; c < count; c += kSoftBlock) {
    const float wt = softmin_weight(costs[c], cmin, a.lambda);
    s_w[c] = wt;
    wsum += static_cast<double>(wt);
  }
  wsum = wave_sum_f64(wsum);
  if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = wsum;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int q = 0; q < kSoftBlock / kWave; ++q) t += s_red[q];
    out[0] = t;
  }

  if constexpr (LAYOUT == 0) {
    // rows of 2n floats: thread group g owns rows c = g (mod G); each thread a fixed entry e of the row
    const int G = kSoftBlock / n2 > 0 ? kSoftBlock / n2 : 1;
    for (int e0 = 0; e0 < n2; e0 += kSoftBlock) {  // n2 > 256 only for n > 128
      const int g = tid / n2;
      const int e = e0 + (tid % n2);
      double acc = 0.0, plain = 0.0;
      if (g < G && e < n2) {
        const float* __restrict__ U = a.U + (static_cast<size_t>(p) * a.N + base) * n2 + e;
        for (int c = g; c < count; c += G) {
          const double u = static_cast<double>(U[static_cast<size_t>(c) * n2]);
          const double wt = static_cast<double>(s_w[c]);
          if (wt != 0.0) acc += wt * u;  // a zero-weight (non-finite cost) candidate is excluded, NaN controls too
          plain += u;
        }
      }
      s_acc[0][tid] = acc;
      s_acc[1][tid] = plain;
      __syncthreads();
      if (tid < n2 && e0 + tid < n2) {
        double t0 = 0.0, t1 = 0.0;
        for (int g2 = 0; g2 < G; ++g2) {
          t0 += s_acc[0][g2 * n2 + tid];
          t1 += s_acc[1][g2 * n2 + tid];
        }
        out[1 + e0 + tid] = t0;
        out[1 + n2 + e0 + tid] = t1;
      }
      __syncthreads();
    }
  } else {
    // U[p][i][comp][N]: each WAVE owns entries e = wave, wave + 4, ... of the 2n, its lanes stride the chunk's
    // candidates (coalesced) and a shuffle reduction finishes the entry - no workgroup barrier per entry (a
    // workgroup-wide reduction per entry made this kernel 98 dependent barriers long: 630 us at N = 16 384)
    const int wave = tid / kWave;
    const int lane = tid & (kWave - 1);
    for (int e = wave; e < n2; e += kSoftBlock / kWave) {
      const float* __restrict__ U = a.U + (static_cast<size_t>(p) * n2 + e) * a.N + base;
      double acc = 0.0, plain = 0.0;
      for (int c = lane; c < count; c += kWave) {
        const double u = static_cast<double>(U[c]);
        const double wt = static_cast<double>(s_w[c]);
        if (wt != 0.0) acc += wt * u;
        plain += u;
      }
      acc = wave_sum_f64(acc);
      plain = wave_sum_f64(plain);
      if (lane == 0) {
        out[1 + e] = acc;
        out[1 + n2 + e] = plain;
      }
    }
  }
}

// softmin_partial_kernel<1> without a control matrix (mode D's sampled rounds have none): the same partial sums, bit for
// bit, over candidates that are RE-DRAWN from their global index - candidate c of the launch is global candidate
// index_offset + c as sample_kernel writes it (draw_normal_block / candidate_amplitude / blend_control on the same
// operands; global candidate 0 = the centre, 1 = u_ref when given).  The bits are fixed by the order of the additions:
//   weights      thread t of 256 adds c = t, t + 256, ... of its chunk of 1 024, wave_sum_f64's xor tree, the four wave
//                sums in order - the matrix kernel's own lines;
//   an entry     lane l adds w_c u_c (a multiply, then an add) over c = l, l + 64, ... in that order, then the xor tree.
// Which wave takes which entry changes no bit, so the work is cut into ITEMS: a run of at most TILE steps that share a
// left knot.  A wave owns an item: lane l walks its (at most 16) candidates of the chunk in order, draws for each only the
// Philox blocks that hold the item's two knots (one block for an even left knot, two for an odd one) and adds the TILE
// steps' controls into 4 TILE double accumulators that stay in registers.  Items go round the 4 gridDim.z waves of a chunk, so
// a solve of a few chunks still spreads over many CUs; every workgroup computes the chunk's weights for itself (1 024
// expf) and the one with blockIdx.z == 0 writes their sum.  The blend weights, the centre and the reference controls are
// staged in LDS; nothing crosses workgroups.
constexpr int kSoftTile = 8;
constexpr int kSoftItemsMax = 160;   // >= max_steps / kSoftTile + kKnots - 1 (max_steps <= 1024)

template <int TILE>
__global__ void __launch_bounds__(kSoftBlock) softmin_sampled_partial_kernel(const SoftminArgs a, const SampleArgs smp) {
  extern __shared__ __attribute__((aligned(16))) float s_draw[];   // [n] weight of the left knot | [n][2] centre | [n][2] reference
  __shared__ float s_w[kSoftChunk];
  __shared__ double s_red[kSoftBlock / kWave];
  __shared__ int s_item[kSoftItemsMax];   // first step | steps << 16 | left knot << 24
  __shared__ int s_items;
  const int p = blockIdx.y;
  const int chunk = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = a.n;
  const int n2 = 2 * n;
  const int base = chunk * kSoftChunk;
  const int count = min(kSoftChunk, a.N - base);
  const float cmin = key_cost(a.keys[p]);
  const float* __restrict__ costs = a.costs + static_cast<size_t>(p) * a.N + base;
  double* __restrict__ out = a.partial + (static_cast<size_t>(p) * a.chunks + chunk) * (2 * n2 + 1);
  float* s_w0 = s_draw;
  float* s_centre = s_draw + n;
  float* s_ref = s_centre + n2;
  {
    const float* __restrict__ centre = smp.centre + static_cast<size_t>(p) * smp.centre_stride;
    const float* __restrict__ ref = smp.u_ref != nullptr ? smp.u_ref + static_cast<size_t>(p) * n2 : centre;
    for (int e = tid; e < n; e += kSoftBlock) s_w0[e] = smp.spec.segments[2 * e + 1];
    for (int e = tid; e < n2; e += kSoftBlock) {
      s_centre[e] = centre[e];
      s_ref[e] = ref[e];
    }
  }
  if (tid == 0) {
    int m = 0;
#pragma unroll
    for (int k = 0; k < kKnots - 1; ++k)
      for (int i = smp.spec.knot_begin[k]; i < smp.spec.knot_begin[k + 1] && m < kSoftItemsMax; i += TILE)
        s_item[m++] = i | (min(TILE, smp.spec.knot_begin[k + 1] - i) << 16) | (k << 24);
    s_items = m;
  }

  double wsum = 0.0;
  for (int c = tid; c < count; c += kSoftBlock) {
    const float wt = softmin_weight(costs[c], cmin, a.lambda);
    s_w[c] = wt;
    wsum += static_cast<double>(wt);
  }
  wsum = wave_sum_f64(wsum);
  if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = wsum;
  __syncthreads();
  if (tid == 0 && blockIdx.z == 0) {
    double t = 0.0;
    for (int q = 0; q < kSoftBlock / kWave; ++q) t += s_red[q];
    out[0] = t;
  }

  SampleSpec sp = smp.spec;   // (the key read once, not per draw)
  if (sp.seed_ptr != nullptr) {
    sp.seed_lo = sp.seed_ptr[0];
    sp.seed_hi = sp.seed_ptr[1];
    sp.seed_ptr = nullptr;
  }
  const bool has_ref = smp.u_ref != nullptr;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int lane = tid & (kWave - 1);
  const int items = s_items;
  constexpr int kWaves = kSoftBlock / kWave;
  for (int it = static_cast<int>(blockIdx.z) * kWaves + wave; it < items; it += static_cast<int>(gridDim.z) * kWaves) {
    const int packed = __builtin_amdgcn_readfirstlane(s_item[it]);
    const int first = packed & 0xffff;
    const int steps = (packed >> 16) & 0xff;
    const int knot = packed >> 24;
    double acc[TILE][2], plain[TILE][2];
#pragma unroll
    for (int t = 0; t < TILE; ++t) acc[t][0] = acc[t][1] = plain[t][0] = plain[t][1] = 0.0;
    for (int c = lane; c < count; c += kWave) {
      const uint32_t gidx = static_cast<uint32_t>(smp.index_offset + base + c);
      // the normals of knots `knot` and `knot` + 1: both in block knot / 2 when the left knot is even
      float zl[4], zr[4];
      draw_normal_block(sp, gidx, static_cast<uint32_t>(p), static_cast<uint32_t>(knot >> 1), zl);
      float z0v = zl[0], z0k = zl[1], z1v = zl[2], z1k = zl[3];
      if (knot & 1) {   // (wave-uniform)
        draw_normal_block(sp, gidx, static_cast<uint32_t>(p), static_cast<uint32_t>((knot + 1) >> 1), zr);
        z0v = zl[2];
        z0k = zl[3];
        z1v = zr[0];
        z1k = zr[1];
      }
      const bool use_ref = has_ref && gidx == 1u;   // candidate 1 = the reference controls: amplitude 0, own centre
      const float amp = use_ref ? 0.0f : candidate_amplitude(gidx);
      const float* cen = use_ref ? s_ref : s_centre;
      const double wt = static_cast<double>(s_w[c]);
#pragma unroll
      for (int t = 0; t < TILE; ++t) {
        if (t < steps) {
          const int i = first + t;
          float v, k;
          blend_control(sp, amp, s_w0[i], cen[2 * i], cen[2 * i + 1], z0v, z0k, z1v, z1k, v, k);
          const double uv = static_cast<double>(v), uk = static_cast<double>(k);
          if (wt != 0.0) {   // a zero-weight (non-finite cost) candidate is excluded
            acc[t][0] += wt * uv;
            acc[t][1] += wt * uk;
          }
          plain[t][0] += uv;
          plain[t][1] += uk;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
      if (t < steps) {
        const double av = wave_sum_f64(acc[t][0]), ak = wave_sum_f64(acc[t][1]);
        const double pv = wave_sum_f64(plain[t][0]), pk = wave_sum_f64(plain[t][1]);
        if (lane == 0) {
          const int e = 2 * (first + t);
          out[1 + e] = av;
          out[1 + e + 1] = ak;
          out[1 + n2 + e] = pv;
          out[1 + n2 + e + 1] = pk;
        }
      }
    }
  }
}

// Sums the chunk partials in chunk order; sum(w u)/sum(w), uniform weights when sum(w) is not positive
// (the NaN fallback of localiser.py:575-578).
__global__ void __launch_bounds__(kSoftBlock) softmin_final_kernel(const SoftminArgs a) {
  const int p = blockIdx.x;
  const int n2 = 2 * a.n;
  const double* __restrict__ part = a.partial + static_cast<size_t>(p) * a.chunks * (2 * n2 + 1);
  double wsum = 0.0;
  for (int q = 0; q < a.chunks; ++q) wsum += part[static_cast<size_t>(q) * (2 * n2 + 1)];
  const bool usable = wsum > 0.0;
  for (int e = threadIdx.x; e < n2; e += kSoftBlock) {
    double acc = 0.0;
    const int col = usable ? 1 + e : 1 + n2 + e;
    for (int q = 0; q < a.chunks; ++q) acc += part[static_cast<size_t>(q) * (2 * n2 + 1) + col];
    a.mean[static_cast<size_t>(p) * n2 + e] =
        static_cast<float>(acc / (usable ? wsum : static_cast<double>(a.N)));
  }
  if (threadIdx.x == 0 && a.weight_sum != nullptr) a.weight_sum[p] = wsum;
}

}  // namespace

int softmin_chunks(int N) { return (N + kSoftChunk - 1) / kSoftChunk; }

// softmin_partial_kernel<0>'s own two numbers: G = 256 / 2n thread groups (1 once a row is wider than the workgroup) and the
// trips of its e0 loop, one per 256 entries of a row
SoftminRows softmin_rows(int n) {
  const int n2 = 2 * n;
  return SoftminRows{kSoftBlock / n2 > 0 ? kSoftBlock / n2 : 1, (n2 + kSoftBlock - 1) / kSoftBlock};
}

int softmin_item_count(const int (&knot_begin)[kKnotsMax + 1]) {
  int m = 0;
  for (int k = 0; k < kKnots - 1; ++k) m += (knot_begin[k + 1] - knot_begin[k] + kSoftTile - 1) / kSoftTile;
  return m;
}

// workgroups per chunk: enough of them that a lone problem of a few chunks still covers the chip, never more than
// there are items for their four waves
SoftminItems softmin_items(int chunks_per_problem, int P, int items) {
  constexpr int kWaves = kSoftBlock / kWave;
  const long long chunks = static_cast<long long>(chunks_per_problem) * P;
  const int by_items = (items + kWaves - 1) / kWaves;
  const int by_chip = static_cast<int>(std::min<long long>((512 + chunks - 1) / chunks, by_items));
  const int z = std::max(by_chip, 1);
  return SoftminItems{z, (items + z * kWaves - 1) / (z * kWaves)};
}

hipError_t launch_softmin(int layout, const SoftminArgs& args, hipStream_t s) {
  clear_stale_error();
  const dim3 grid(args.chunks, args.P);
  if (layout != 0 && layout != 1) return hipErrorInvalidValue;
  const hipError_t e = (layout == 0) ? launch_kernel(softmin_partial_kernel<0>, grid, dim3(kSoftBlock), 0, s, nullptr, nullptr, args)
                                     : launch_kernel(softmin_partial_kernel<1>, grid, dim3(kSoftBlock), 0, s, nullptr, nullptr, args);
  if (e != hipSuccess) return e;
  return launch_kernel(softmin_final_kernel, dim3(args.P), dim3(kSoftBlock), 0, s, nullptr, nullptr, args);
}

hipError_t launch_softmin_sampled(const SoftminArgs& args, const SampleArgs& sample, hipStream_t s) {
  clear_stale_error();
  if (args.P < 1 || args.N < 1 || args.n < 1 || args.n > 1024 || args.chunks != softmin_chunks(args.N)) return hipErrorInvalidValue;
  if (sample.P != args.P || sample.N != args.N || sample.n != args.n) return hipErrorInvalidValue;
  if (sample.centre == nullptr || sample.spec.segments == nullptr || sample.centre_stride < 2 * args.n) return hipErrorInvalidValue;
  if (sample.u_extra != nullptr || sample.prev_keys != nullptr) return hipErrorInvalidValue;
  if (sample.index_offset < 0 || sample.index_offset + args.N > 0xffffffffLL) return hipErrorInvalidValue;
  const int (&kb)[kKnotsMax + 1] = sample.spec.knot_begin;   // the knot table's bounds must be those of this horizon
  if (kb[0] != 0 || kb[kKnots - 1] != args.n) return hipErrorInvalidValue;
  for (int k = 0; k < kKnots - 1; ++k)
    if (kb[k + 1] < kb[k]) return hipErrorInvalidValue;
  const int items = softmin_item_count(kb);
  if (items < 1 || items > kSoftItemsMax) return hipErrorInvalidValue;
  const dim3 grid(args.chunks, args.P, softmin_items(args.chunks, args.P, items).grid_z);
  const size_t lds = static_cast<size_t>(5) * args.n * sizeof(float);
  const hipError_t e = launch_kernel(softmin_sampled_partial_kernel<kSoftTile>, grid, dim3(kSoftBlock), lds, s, nullptr, nullptr, args, sample);
  if (e != hipSuccess) return e;
  return launch_kernel(softmin_final_kernel, dim3(args.P), dim3(kSoftBlock), 0, s, nullptr, nullptr, args);
}

}  // namespace acmpc
