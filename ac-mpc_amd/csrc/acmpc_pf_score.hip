// Particle filter, scoring: the three nearest-point searches per particle and the score of the observation against the
// map (LocalisationProcess._update_particles, src/acmpc/localisation/localiser.py:255-410), with the policy that picks
// the launches.
//
// Precision follows the reference step by step: float32 particle states and observations, placement of the observation
// in float32, a float64 map, float64 distances/error/score.  Nearest-neighbour indices must be the ones a KD-tree query
// returns, so every search compares float64 squared distances (lowest index on ties).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "acmpc_pf.h"

using namespace acmpc::pf;

namespace {

constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ void take_smaller(double& d, int& i, double od, int oi) {
  if (od < d || (od == d && oi < i)) {  // lowest index on ties: the first minimum
    d = od;
    i = oi;
  }
}

// (distance^2, index) minimum over the wavefront, every lane ends with the result
__device__ __forceinline__ void wave_argmin(double& d, int& i) {
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) {
    const double od = __shfl_xor(d, mask, 64);
    const int oi = __shfl_xor(i, mask, 64);
    take_smaller(d, i, od, oi);
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) v += __shfl_xor(v, mask, 64);  // fixed tree: reproducible
  return v;
}

// ---- nearest map point through a uniform grid ------------------------------------------------------------------------
// The reference answers its three nearest-point queries per particle with KD-trees (localiser.py:282-289); scanning the
// whole map per particle, as pf_score_kernel does on its own, is 3 x 34 758 distance evaluations each.  The map's points
// are binned once (host, at create) into square cells of `cell` metres, one index per polyline over a common box:
// `start` [cells + 1] and the points themselves in cell order (x, y, index in the polyline).  A query visits the cell of the particle,
// then ring after ring of cells round it; after ring r every point not yet seen lies outside the block of
// (2r + 1)^2 cells, i.e. at least `margin` = the particle's distance to the nearest side of that block away (sides on
// the box's own border do not count: nothing lies beyond them), so the search stops as soon as the best squared
// distance is below margin^2.  Same float64 distance expression, ties to the lower index: the answer is the
// exhaustive scan's, bit for bit.  A particle whose search is not settled after kMaxRings rings (far from the track,
// or outside the box) is scanned exhaustively by its whole wavefront.
constexpr int kMaxRings = 4;

// (distance^2, index) minimum over the LANES consecutive lanes that share a query (LANES a power of two), every one
// of them ends with the result
template <int LANES>
__device__ __forceinline__ void group_argmin(double& d, int& i) {
#pragma unroll
  for (int mask = LANES / 2; mask >= 1; mask >>= 1) {
    const double od = __shfl_xor(d, mask, 64);
    const int oi = __shfl_xor(i, mask, 64);
    take_smaller(d, i, od, oi);
  }
}

// One run of the cell-ordered arrays - the points of a row of cells - against the query, LANES lanes side by side, two
// points per lane and trip: consecutive lanes read consecutive points, so a trip is a handful of cache lines, where a lane
// walking its own run (rounds 2-4: one lane per query) touched a line per lane and array - the search was bound by the
// number of LINES its gathers asked the vector cache for, not by their bytes (round 5, profiles/r05_pf_sq_counters.json).
template <int LANES>
__device__ __forceinline__ void scan_run(const double* __restrict__ gx, const double* __restrict__ gy,
                                         const int* __restrict__ gi, int j0, int j1, int sub, double px, double py,
                                         double& best, int& best_i) {
  for (int j = j0 + sub; j < j1; j += 2 * LANES) {
    const int k = min(j + LANES, j1 - 1);   // past the run: its last point again (harmless: same distance, same index)
    const double ax = gx[j], ay = gy[j], bx = gx[k], by = gy[k];
    const int ai = gi[j], bi = gi[k];
    const double adx = px - ax, ady = py - ay, bdx = px - bx, bdy = py - by;
    take_smaller(best, best_i, adx * adx + ady * ady, ai);
    take_smaller(best, best_i, bdx * bdx + bdy * bdy, bi);
  }
}

// The nearest point of one polyline to (px, py) through the grid, by the LANES lanes of a group together (`sub` = the
// lane's place in its group; every argument but `sub` is the same for all of them).  The block of 3 x 3 cells round the
// query first - its three rows requested together - then 5 x 5 ... (2 kMaxRings + 1)^2, each block scanned whole; after a
// block every point not yet seen is at least `margin` = the distance to the nearest side of the block that has cells
// beyond it away, so the search stops as soon as the best squared distance is below margin^2.  Returns whether it settled;
// (best, best_i) are the group's result then.  Same float64 distance expression as the exhaustive scan, ties to the lower
// index: its answer, bit for bit.  (The single cell of rounds 2-4 is no longer tried first: the left and right limits
// lie 4.75 m from the centre line, more than half a cell - two queries in three never settled there.)
template <int LANES>
__device__ __forceinline__ bool grid_nearest(double px, double py, const GridGeometry& g, const GridBlocks& blocks,
                                             const GridIndex (&grids)[3], int t, int sub, double& best, int& best_i) {
  // (any cell will do for a correct answer - the margins below are measured from the particle itself - so the particle's
  // cell comes from a product with 1 / cell here, where the host bins the map's points with the division)
  const double inv_cell = 1.0 / g.cell;   // wave-uniform: scalar registers
  const int ix = min(max(static_cast<int>(floor((px - g.x0) * inv_cell)), 0), g.nx - 1);
  const int iy = min(max(static_cast<int>(floor((py - g.y0) * inv_cell)), 0), g.ny - 1);
  for (int r = 1; r <= kMaxRings; ++r) {
    best = INFINITY;
    best_i = 0x7fffffff;
    if (r == 1 && blocks.start != nullptr) {   // the 3 x 3 block: one run
      const int c = t * blocks.cells + iy * g.nx + ix;
      scan_run<LANES>(blocks.x, blocks.y, blocks.index, blocks.start[c], blocks.start[c + 1], sub, px, py, best, best_i);
    } else {
      // (rare from the second ring on: the polyline's own arrays are chosen here, not in front of the search)
      const GridIndex& gr = (t == 0) ? grids[0] : (t == 1) ? grids[1] : grids[2];
      const int x_lo = max(ix - r, 0), x_hi = min(ix + r, g.nx - 1);
      const int y_lo = max(iy - r, 0), y_hi = min(iy + r, g.ny - 1);
      for (int cy = y_lo; cy <= y_hi; ++cy)
        scan_run<LANES>(gr.x, gr.y, gr.index, gr.start[cy * g.nx + x_lo], gr.start[cy * g.nx + x_hi + 1], sub, px, py, best,
                        best_i);
    }
    group_argmin<LANES>(best, best_i);
    // distance to the nearest side of the block that has cells beyond it
    double margin = INFINITY;
    if (ix - r > 0) margin = fmin(margin, px - (g.x0 + (ix - r) * g.cell));
    if (ix + r < g.nx - 1) margin = fmin(margin, (g.x0 + (ix + r + 1) * g.cell) - px);
    if (iy - r > 0) margin = fmin(margin, py - (g.y0 + (iy - r) * g.cell));
    if (iy + r < g.ny - 1) margin = fmin(margin, (g.y0 + (iy + r + 1) * g.cell) - py);
    // (1 - 1e-9: the comparison must hold for the exact values; strictly below, so that a point outside the block at
    // exactly the same distance, which could carry a lower index, is still looked at)
    if (margin > 0.0 && best < margin * margin * (1.0 - 1e-9)) return true;
    if (margin == INFINITY) return true;   // the block covers the whole box
  }
  return false;
}

// The exhaustive scan of one polyline by a whole wavefront (what the grid search falls back to: a query far from the
// track, outside the box, non-finite); every lane ends with the result.
__device__ __forceinline__ void wave_scan(const Track& track, double qx, double qy, int lane, double& d, int& i) {
  d = INFINITY;
  i = 0x7fffffff;
  for (int m = lane; m < track.m; m += 64) {
    const double dx = qx - track.xy[2 * m], dy = qy - track.xy[2 * m + 1];
    const double dd = dx * dx + dy * dy;
    if (dd < d) {   // ascending m per lane: the first minimum stays
      d = dd;
      i = m;
    }
  }
  wave_argmin(d, i);
}

// kGroupLanes lanes per (particle, polyline) query, 64 / kGroupLanes queries per wavefront at a time, kQueriesPerWave per
// wavefront.  (A/B builds: ACMPC_HIPCC_EXTRA=-DACMPC_PF_GROUP_LANES=8)
#ifndef ACMPC_PF_GROUP_LANES
#define ACMPC_PF_GROUP_LANES 16
#endif
constexpr int kGroupLanes = ACMPC_PF_GROUP_LANES;
constexpr int kQueriesPerWave = 16;
static_assert(kGroupLanes == 4 || kGroupLanes == 8 || kGroupLanes == 16 || kGroupLanes == 32, "a power of two, several groups per wave");
static_assert(kQueriesPerWave % (64 / kGroupLanes) == 0, "whole rounds");

__global__ void __launch_bounds__(64) pf_nearest_kernel(const GridArgs a, const int P_arg) {
  const int lane = threadIdx.x;
  const int P = (a.live != nullptr) ? a.live[0] : P_arg;
  const int first = blockIdx.x * kQueriesPerWave;
  if (first >= 3 * P) return;   // wave-uniform
  const int group = lane / kGroupLanes, sub = lane % kGroupLanes;
  const GridGeometry geo{a.x0, a.y0, a.cell, a.nx, a.ny};
#pragma unroll 1
  for (int round = 0; round < kQueriesPerWave / (64 / kGroupLanes); ++round) {
    const int base = first + round * (64 / kGroupLanes);
    if (base >= 3 * P) break;   // wave-uniform
    const int query = base + group;
    const bool active = query < 3 * P;
    const int p = active ? query / 3 : P - 1;
    const int t = active ? query - 3 * p : 0;
    const double px = a.states[3 * p], py = a.states[3 * p + 1];
    double best;
    int best_i;
    const bool settled = grid_nearest<kGroupLanes>(px, py, geo, a.blocks, a.grid, t, sub, best, best_i);
    // the rest: all 64 lanes scan the polyline side by side for each unsettled query of the wave
    unsigned long long pending = __ballot(!settled && sub == 0);
    while (pending != 0ull) {
      const int src = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(pending)) - 1);
      pending &= pending - 1ull;
      const double qx = __shfl(px, src, 64), qy = __shfl(py, src, 64);
      const int qt = __builtin_amdgcn_readlane(t, src);
      double d;
      int i;
      wave_scan(a.track[qt], qx, qy, lane, d, i);
      if (lane == src) {
        best = d;
        best_i = i;
      }
    }
    if (active && sub == 0) {
      a.index_out[3 * p + t] = best_i;
      a.d2_out[3 * p + t] = best;
    }
  }
}

// One workgroup scores PB particles.  Every map point a thread loads is compared against all PB of them, so the
// map (557 kB for the three 11.6 k-point polylines) crosses the L2 once per workgroup instead of once per particle -
// at 100 000 particles that read was the bound (55 GB per scoring call).  Reductions are wave shuffles plus one
// kWaves-entry exchange through LDS per polyline, for all PB particles at once (the first form ran three 256-wide
// LDS trees of eight barriers each per particle).  PB = 1 keeps one particle per workgroup for the reference's
// particle counts (500: configs/monza.yaml:47), where the launch has to fill the chip with workgroups.
template <int PB>
__global__ void __launch_bounds__(kBlock) pf_score_kernel(const ScoreArgs a, const int P_arg) {
  __shared__ double s_d[3][PB][kWaves];
  __shared__ int s_i[3][PB][kWaves];
  __shared__ double s_sum[PB][kWaves];
  __shared__ float s_frame[PB][4];   // cos, sin of the placement angle and the particle's position, per particle
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int p0 = blockIdx.x * PB;
  if (a.live != nullptr) {   // wave-uniform
    if (p0 >= a.live[0]) return;
  }
  const int P = (a.live != nullptr) ? a.live[0] : P_arg;
  double px[PB], py[PB];
#pragma unroll
  for (int q = 0; q < PB; ++q) {
    const int p = min(p0 + q, P - 1);  // the last workgroup repeats its last particle; only p < P is written
    px[q] = a.states[3 * p];
    py[q] = a.states[3 * p + 1];
  }

  // three nearest-neighbour queries (localiser.py:282-289): first minimum of the float64 squared distance - found
  // already by the grid search, or scanned here
  const Track tracks[3] = {a.centre, a.left, a.right};
  const bool own_search = PB == 1 && a.own_grid_search != 0;   // wave-uniform
  if (own_search) {
    // the reference's particle counts (hundreds): a wavefront per polyline, its 64 lanes across the points of the cells
    // round the particle - ~150 points per polyline instead of all 11 600 (rounds 1-4 scanned the whole map here: 35 us
    // for 500 particles, every workgroup reading 556 kB through the L2)
    if (wave < 3) {
      double best;
      int best_i;
      const int which = __builtin_amdgcn_readfirstlane(wave);
      if (!grid_nearest<64>(px[0], py[0], a.geometry, a.blocks, a.grid, which, lane, best, best_i))
        wave_scan(tracks[wave], px[0], py[0], lane, best, best_i);
      if (lane < kWaves) {
        s_d[wave][0][lane] = (lane == 0) ? best : INFINITY;
        s_i[wave][0][lane] = (lane == 0) ? best_i : 0x7fffffff;
      }
    }
  }
  // the placement of the observation in each particle's frame needs cos / sin of ITS angle: once per particle (round 5;
  // every thread used to evaluate both for every particle of the workgroup - a fifth of the kernel's instructions at PB = 8)
  if (tid < PB) {
    const int p = min(p0 + tid, P - 1);
    const float angle = -a.states[3 * p + 2] + 1.57079632679489661923f;
    s_frame[tid][0] = cosf(angle);
    s_frame[tid][1] = sinf(angle);
    s_frame[tid][2] = a.states[3 * p];
    s_frame[tid][3] = a.states[3 * p + 1];
  }
  const bool given = a.given_index != nullptr || own_search;   // wave-uniform
  if (given && !own_search) {
    for (int e = tid; e < 3 * PB * kWaves; e += kBlock) {
      const int w = e % kWaves, q = (e / kWaves) % PB, t = e / (kWaves * PB);
      const int p = min(p0 + q, P - 1);
      s_d[t][q][w] = (w == 0) ? a.given_d2[3 * p + t] : INFINITY;
      s_i[t][q][w] = (w == 0) ? a.given_index[3 * p + t] : 0x7fffffff;
    }
  }
#pragma unroll
  for (int t = 0; t < 3 && !given; ++t) {
    double best[PB];
    int best_i[PB];
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      best[q] = INFINITY;
      best_i[q] = 0x7fffffff;
    }
    const double* __restrict__ xy = tracks[t].xy;
    for (int m = tid; m < tracks[t].m; m += kBlock) {
      const double mx = xy[2 * m], my = xy[2 * m + 1];
#pragma unroll
      for (int q = 0; q < PB; ++q) {
        const double dx = px[q] - mx, dy = py[q] - my;
        const double d = dx * dx + dy * dy;
        if (d < best[q]) {  // ascending m per thread: the first minimum stays
          best[q] = d;
          best_i[q] = m;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      wave_argmin(best[q], best_i[q]);
      if (lane == 0) {
        s_d[t][q][wave] = best[q];
        s_i[t][q][wave] = best_i[q];
      }
    }
  }
  __syncthreads();
  int nearest[3][PB];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      double d = s_d[t][q][0];
      int i = s_i[t][q][0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) take_smaller(d, i, s_d[t][q][w], s_i[t][q][w]);
      nearest[t][q] = (i == 0x7fffffff) ? 0 : i;   // a non-finite position is nearest to nothing: point 0, like np.argmin
    }

  // observation placed in each particle's frame vs the map limits ahead of the nearest points (:330-410)
  // The reference places the observation in float32 (float32 states and observation, :330-353) and only then
  // subtracts the float64 map: do the same, so that the placed points round the way its do.
  const int K = a.k_left + a.k_right;
#pragma unroll
  for (int q = 0; q < PB; ++q) {
    const float ca = s_frame[q][0], sa = s_frame[q][1], px32 = s_frame[q][2], py32 = s_frame[q][3];
    double sum = 0.0;
    for (int k = tid; k < K; k += kBlock) {
      const float ox = a.obs[2 * k], oy = a.obs[2 * k + 1];
      const double wx = (ca * ox + sa * oy) + px32;   // transpose of [[cos, -sin], [sin, cos]] (:355-364)
      const double wy = (-sa * ox + ca * oy) + py32;
      const bool is_left = k < a.k_left;
      const Track t = is_left ? a.left : a.right;
      const int i = is_left ? k : k - a.k_left;
      const int count = is_left ? a.k_left : a.k_right;
      const int closest = is_left ? nearest[1][q] : nearest[2][q];
      // np.linspace(closest, closest + count, count, dtype=uint16): closest + i, except the last entry = closest + count
      const int off = (count > 1 && i == count - 1) ? count : i;
      const int idx = ((closest + off) & 0xffff) % t.m;
      const double dx = wx - t.xy[2 * idx], dy = wy - t.xy[2 * idx + 1];
      sum += sqrt(dx * dx + dy * dy);
    }
    sum = wave_sum(sum);
    if (lane == 0) s_sum[q][wave] = sum;
  }
  __syncthreads();

  if (tid < PB && p0 + tid < P) {
    const int q = tid, p = p0 + tid;
    double total = s_sum[q][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) total += s_sum[q][w];
    const double error = total / static_cast<double>(K);
    const double phi = a.states[3 * p + 2];
    // nearest[...][q] with a run-time q: read them back from LDS (the registers are indexed statically)
    int i_centre = s_i[0][q][0], i_left = s_i[1][q][0], i_right = s_i[2][q][0];
    double dc = s_d[0][q][0], dl = s_d[1][q][0], dr = s_d[2][q][0];
    for (int w = 1; w < kWaves; ++w) {
      take_smaller(dc, i_centre, s_d[0][q][w], s_i[0][q][w]);
      take_smaller(dl, i_left, s_d[1][q][w], s_i[1][q][w]);
      take_smaller(dr, i_right, s_d[2][q][w], s_i[2][q][w]);
    }
    i_centre = (i_centre == 0x7fffffff) ? 0 : i_centre;
    i_left = (i_left == 0x7fffffff) ? 0 : i_left;
    i_right = (i_right == 0x7fffffff) ? 0 : i_right;
    // heading of the centreline at the nearest point, indices mod (len - 1) (:291-318)
    const int m1 = a.centre.m - 1;
    const int here = i_centre % m1, next = (i_centre + 1) % m1;
    const double track_heading = atan2(a.centre.xy[2 * next + 1] - a.centre.xy[2 * here + 1],
                                       a.centre.xy[2 * next] - a.centre.xy[2 * here]);
    const double raw = track_heading - phi + kPi;
    const double heading = fabs(raw - floor(raw / (2 * kPi)) * (2 * kPi) - kPi);
    const double offset = sqrt(dc);
    const double z = (error - a.mean) / a.sigma;
    const double score = exp(-z * z / 2.0) / sqrt(2.0 * kPi) / a.sigma / a.scale;
    a.track_indices[3 * p] = i_centre;
    a.track_indices[3 * p + 1] = i_left;
    a.track_indices[3 * p + 2] = i_right;
    a.minimum_offset[p] = offset;
    a.heading_offset[p] = heading;
    a.error[p] = error;
    a.score[p] = score;
    if (a.publish != nullptr) a.publish[p] = static_cast<float>(score);
    a.valid[p] = (heading < a.thr_rotation && offset < a.thr_offset && error < a.thr_error) ? 1 : 0;
  }
}

// x mod m for 0 <= x < 65 536 and m >= 1 (the reference's uint16 index arithmetic, :388-392) without the integer division
// the compiler emits for `%`: the quotient from a float32 product (inv_m = 1.0f / m), off by one at most, then put right.
__device__ __forceinline__ int mod_u16(int x, int m, float inv_m) {
  const int q = static_cast<int>(static_cast<float>(x) * inv_m);
  int r = x - q * m;
  r = (r < 0) ? r + m : r;
  return (r >= m) ? r - m : r;
}

// v of lane (l ^ MASK): the vector pipe's own lane permutations where it has one for the mask (inside a quad, across the
// halves of a row of 16), the LDS crossbar otherwise
template <int MASK>
__device__ __forceinline__ double from_lane_xor(double v) {
  if constexpr (MASK == 1 || MASK == 2 || MASK == 8) {
    constexpr int ctrl = (MASK == 1) ? 0xB1 : (MASK == 2) ? 0x4E : 0x128;   // quad_perm [1,0,3,2] / [2,3,0,1] / row_ror:8
    const long long bits = __double_as_longlong(v);
    // (every lane has a source under these controls: `old` is never kept, and passing the value itself saves its zeroing)
    const int lo = __builtin_amdgcn_update_dpp(static_cast<int>(bits), static_cast<int>(bits), ctrl, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(static_cast<int>(bits >> 32), static_cast<int>(bits >> 32), ctrl, 0xf, 0xf, false);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
  } else {
    return __shfl_xor(v, MASK, 64);
  }
}

// ((wave_sum(s[0]) + wave_sum(s[1])) + wave_sum(s[2])) + wave_sum(s[3]), bit for bit, in ten exchanges instead of twenty-
// four.  wave_sum's tree adds lane l ^ 32, then l ^ 16, ... l ^ 1; after the first stage both halves of the wave hold the
// same 32 partial sums (a + b = b + a), so two sums share a vector from there - and after the second stage four.  Every
// sum is still reduced by exactly wave_sum's tree.
__device__ __forceinline__ double wave_sum_of_four(const double (&s)[4], int lane) {
  double t[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) t[w] = s[w] + from_lane_xor<32>(s[w]);
  double a = (lane < 32) ? t[0] : t[1], b = (lane < 32) ? t[2] : t[3];
  a += from_lane_xor<16>(a);
  b += from_lane_xor<16>(b);
  double c = (lane & 16) ? b : a;   // lanes 0-15: s[0]'s partial sums, 16-31: s[2]'s, 32-47: s[1]'s, 48-63: s[3]'s
  c += from_lane_xor<8>(c);
  c += from_lane_xor<4>(c);
  c += from_lane_xor<2>(c);
  c += from_lane_xor<1>(c);
  auto of_lane = [&](int l) {
    const long long bits = __double_as_longlong(c);
    const int lo = __builtin_amdgcn_readlane(static_cast<int>(bits), l), hi = __builtin_amdgcn_readlane(static_cast<int>(bits >> 32), l);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
  };
  return ((of_lane(0) + of_lane(32)) + of_lane(16)) + of_lane(48);
}

// The scoring of particles whose nearest points are GIVEN (pf_nearest_kernel ran in front: 4 096 particles and more), one
// WAVEFRONT for PW particles and no workgroup at all: lane l (< PW) holds particle l's frame and nearest points and
// evaluates its score at the end; in between the 64 lanes place the observation in one particle's frame after the other
// (wave-uniform frame: read out of lane l's registers) and sum the distances.  pf_score_kernel<8> spent its time waiting -
// two barriers and four dependent trips to memory per workgroup of 3 us of work, 1 150 instructions per wave (profiles/
// r05_pf_sq_counters.json) - and evaluated the eight tails (atan2, exp, float64 divisions) on eight lanes of one wave.
// Same bits: pf_score_kernel's thread `tid` sums the observation points k = tid, tid + 256, ...; its wave w reduces them
// with wave_sum and the four sums are added in the order of the waves.  Here lane l does the same for each of the four
// slots w (k = 64 w + l, + 256, ...), each slot is reduced by the same tree, and they are added in the same order.
// ONE_TRIP: at most 256 observation points (the reference's downsampled observation: 200), a point per lane and slot.
// NO_WRAP: nearest index + offset stays below 65 536 and below twice the polyline's length on both sides (launch_score
// checks the lengths), so the uint16 wrap never happens and the modulo is one conditional subtraction.
// PW (1 ... 64, wave-uniform): particles per wave - launch_score picks it so that the launch is whole generations of waves.
template <bool ONE_TRIP, bool NO_WRAP>
__global__ void __launch_bounds__(64) pf_score_given_kernel(const ScoreArgs a, const int P_arg, const int PW) {
  static_assert(kWaves == 4, "wave_sum_of_four");
  const int lane = threadIdx.x;
  const int p0 = blockIdx.x * PW;
  const int P = (a.live != nullptr) ? a.live[0] : P_arg;
  if (p0 >= P) return;   // wave-uniform
  // phase 0: lane l's own particle (lanes beyond the count repeat the last one and write nothing)
  const int p_own = min(p0 + min(lane, PW - 1), P - 1);
  const float sx = a.states[3 * p_own], sy = a.states[3 * p_own + 1], sphi = a.states[3 * p_own + 2];
  const float angle = -sphi + 1.57079632679489661923f;
  const float ca_own = cosf(angle), sa_own = sinf(angle);
  int i_centre = a.given_index[3 * p_own], i_left = a.given_index[3 * p_own + 1], i_right = a.given_index[3 * p_own + 2];
  const double dc = a.given_d2[3 * p_own];
  i_centre = (i_centre == 0x7fffffff) ? 0 : i_centre;   // a non-finite position is nearest to nothing: point 0, like np.argmin
  i_left = (i_left == 0x7fffffff) ? 0 : i_left;
  i_right = (i_right == 0x7fffffff) ? 0 : i_right;

  // phase 1: the observation against the map limits ahead of each particle's nearest points (:330-410), float32 placement
  // as the reference's, float64 from the subtraction of the map on
  const int K = a.k_left + a.k_right;
  // what observation point k contributes for every particle alike
  struct Slot {
    float ox, oy;
    int off;        // np.linspace(closest, closest + count, count, dtype=uint16): closest + i, except the last entry = closest + count
    bool is_left, live;
  };
  auto slot_of = [&](int k_raw) {
    Slot t;
    t.live = k_raw < K;
    const int k = min(k_raw, K - 1);   // (a lane past the end evaluates the last point and adds nothing)
    t.ox = a.obs[2 * k];
    t.oy = a.obs[2 * k + 1];
    t.is_left = k < a.k_left;
    const int i = t.is_left ? k : k - a.k_left;
    const int count = t.is_left ? a.k_left : a.k_right;
    t.off = (count > 1 && i == count - 1) ? count : i;
    return t;
  };
  // in two halves, so that a particle's four map points are requested together and not one after the other's arrival
  auto map_point = [&](const Slot& t, int near_left, int near_right) {
    const double* __restrict__ xy = t.is_left ? a.left.xy : a.right.xy;
    const int m = t.is_left ? a.left.m : a.right.m;
    const int ahead = (t.is_left ? near_left : near_right) + t.off;
    int idx;
    if constexpr (NO_WRAP) {
      idx = (ahead >= m) ? ahead - m : ahead;
    } else {
      idx = mod_u16(ahead & 0xffff, m, t.is_left ? a.inv_left_m : a.inv_right_m);
    }
    return *reinterpret_cast<const double2*>(xy + 2 * idx);   // (x, y): 16-byte aligned
  };
  auto distance = [&](const Slot& t, float ca, float sa, float px32, float py32, double2 at) {
    const double wx = (ca * t.ox + sa * t.oy) + px32;   // transpose of [[cos, -sin], [sin, cos]] (:355-364)
    const double wy = (-sa * t.ox + ca * t.oy) + py32;
    const double dx = wx - at.x, dy = wy - at.y;
    return sqrt(dx * dx + dy * dy);
  };
  Slot slots[kWaves];
#pragma unroll
  for (int w = 0; w < kWaves; ++w) slots[w] = slot_of(64 * w + lane);
  double total_own = 0.0;
  const int count_here = min(PW, P - p0);
#pragma unroll 1
  for (int q = 0; q < count_here; ++q) {
    const float ca = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ca_own), q));
    const float sa = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sa_own), q));
    const float px32 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sx), q));
    const float py32 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sy), q));
    const int near_left = __builtin_amdgcn_readlane(i_left, q), near_right = __builtin_amdgcn_readlane(i_right, q);
    double sum[kWaves];
    double2 at[kWaves];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) at[w] = map_point(slots[w], near_left, near_right);
    __builtin_amdgcn_sched_barrier(0);   // (the scheduler otherwise reuses one register quad and serialises the four loads)
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const double d = distance(slots[w], ca, sa, px32, py32, at[w]);
      sum[w] = slots[w].live ? d : 0.0;
    }
    if constexpr (!ONE_TRIP) {
      for (int base = kBlock; base < K; base += kBlock) {
        Slot t[kWaves];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          t[w] = slot_of(base + 64 * w + lane);
          at[w] = map_point(t[w], near_left, near_right);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          const double d = distance(t[w], ca, sa, px32, py32, at[w]);
          sum[w] += t[w].live ? d : 0.0;
        }
      }
    }
    const double total = wave_sum_of_four(sum, lane);
    total_own = (lane == q) ? total : total_own;
  }

  // phase 2: lane l finishes particle l (heading of the centre line at the nearest point, score, validity)
  if (lane < count_here) {
    const int p = p0 + lane;
    const double error = total_own / static_cast<double>(K);
    const double phi = sphi;
    // heading of the centreline at the nearest point, indices mod (len - 1) (:291-318)
    const int m1 = a.centre.m - 1;
    const int here = i_centre % m1, next = (i_centre + 1) % m1;
    const double track_heading = atan2(a.centre.xy[2 * next + 1] - a.centre.xy[2 * here + 1],
                                       a.centre.xy[2 * next] - a.centre.xy[2 * here]);
    const double raw = track_heading - phi + kPi;
    const double heading = fabs(raw - floor(raw / (2 * kPi)) * (2 * kPi) - kPi);
    const double offset = sqrt(dc);
    const double z = (error - a.mean) / a.sigma;
    const double score = exp(-z * z / 2.0) / sqrt(2.0 * kPi) / a.sigma / a.scale;
    a.track_indices[3 * p] = i_centre;
    a.track_indices[3 * p + 1] = i_left;
    a.track_indices[3 * p + 2] = i_right;
    a.minimum_offset[p] = offset;
    a.heading_offset[p] = heading;
    a.error[p] = error;
    a.score[p] = score;
    if (a.publish != nullptr) a.publish[p] = static_cast<float>(score);
    a.valid[p] = (heading < a.thr_rotation && offset < a.thr_offset && error < a.thr_error) ? 1 : 0;
  }
}

// ---- launch policy ---------------------------------------------------------------------------------------------------
// from kGridParticles up the grid search is a launch of its own in front of the scoring (sixteen lanes per query); below,
// the scoring workgroup of a particle searches the grid itself, a wavefront per polyline
constexpr int kGridParticles = 4096;

bool has_grid(const acmpc_pf* h) { return h->grid.geometry.nx > 0 && !h->no_grid; }

GridIndex grid_index(const acmpc_pf* h, int t) {
  return GridIndex{h->d_grid_start[t], h->d_grid_x[t], h->d_grid_y[t], h->d_grid_index[t]};
}

GridBlocks blocks_of(const acmpc_pf* h) {
  if (h->no_blocks) return GridBlocks{nullptr, nullptr, nullptr, nullptr, 0};
  return GridBlocks{h->d_block_start, h->d_block_x, h->d_block_y, h->d_block_index, h->grid.geometry.nx * h->grid.geometry.ny};
}

}  // namespace

namespace acmpc::pf {

hipError_t launch_nearest(const acmpc_pf* h, ScoreArgs& a, int P, hipStream_t s) {
  a.own_grid_search = 0;
  if (!has_grid(h)) return hipSuccess;
  const GridGeometry& geo = h->grid.geometry;
  if (P < kGridParticles) {
    a.own_grid_search = 1;
    for (int t = 0; t < 3; ++t) a.grid[t] = grid_index(h, t);
    a.geometry = geo;
    a.blocks = blocks_of(h);
    return hipSuccess;
  }
  GridArgs g{};
  g.states = a.states;
  g.live = a.live;
  g.track[0] = a.centre;
  g.track[1] = a.left;
  g.track[2] = a.right;
  for (int t = 0; t < 3; ++t) g.grid[t] = grid_index(h, t);
  g.blocks = blocks_of(h);
  g.x0 = geo.x0;
  g.y0 = geo.y0;
  g.cell = geo.cell;
  g.nx = geo.nx;
  g.ny = geo.ny;
  g.index_out = h->d_near_index;
  g.d2_out = h->d_near_d2;
  hipLaunchKernelGGL(pf_nearest_kernel, dim3((3 * P + kQueriesPerWave - 1) / kQueriesPerWave), dim3(64), 0, s, g, P);
  a.given_index = h->d_near_index;
  a.given_d2 = h->d_near_d2;
  return hipGetLastError();
}

// given nearest points -> a wavefront per 16 particles (4 where that would leave the chip short of waves); none given ->
// the workgroup kernels, which find them (PB = 1: through the grid)
void launch_score(const acmpc_pf* h, const ScoreArgs& a, int P, hipStream_t s) {
  if (a.given_index != nullptr && !h->workgroup_score) {
    ScoreArgs b = a;
    b.inv_left_m = 1.0f / static_cast<float>(a.left.m);
    b.inv_right_m = 1.0f / static_cast<float>(a.right.m);
    const int K = a.k_left + a.k_right;
    const bool one_trip = K <= kBlock;
    // the indices ahead of a nearest point: nearest + offset <= (m - 1) + max(k_left, k_right)
    const bool no_wrap = std::max(a.left.m, a.right.m) + K <= 65536 && K <= std::min(a.left.m, a.right.m);
    const int form = one_trip ? (no_wrap ? 0 : 1) : 2;
    // particles per wave: the launch as whole generations of resident waves (a handful of waves left over for a second
    // generation would double the kernel's time), at least 4 per wave, at most 32
    const int slots = std::max(h->given_wave_slots[form], 1);
    const int generations = (P + 32 * slots - 1) / (32 * slots);
    const int pw = std::min(std::max((P + slots * generations - 1) / (slots * generations), 4), 32);
    const dim3 grid((P + pw - 1) / pw);
    if (form == 0) hipLaunchKernelGGL((pf_score_given_kernel<true, true>), grid, dim3(64), 0, s, b, P, pw);
    else if (form == 1) hipLaunchKernelGGL((pf_score_given_kernel<true, false>), grid, dim3(64), 0, s, b, P, pw);
    else hipLaunchKernelGGL((pf_score_given_kernel<false, false>), grid, dim3(64), 0, s, b, P, pw);
  } else if (P >= kGridParticles) {
    constexpr int PB = 8;
    hipLaunchKernelGGL(pf_score_kernel<PB>, dim3((P + PB - 1) / PB), dim3(kBlock), 0, s, a, P);
  } else {
    hipLaunchKernelGGL(pf_score_kernel<1>, dim3(P), dim3(kBlock), 0, s, a, P);
  }
}

// how many waves of the wave-per-particles scoring kernel the device holds at once (launch_score sizes its waves by it)
int query_given_wave_slots(acmpc_pf* h) {
  int device = 0, units = 0, per_unit[3] = {0, 0, 0};
  PF_HIP(h, hipGetDevice(&device));
  PF_HIP(h, hipDeviceGetAttribute(&units, hipDeviceAttributeMultiprocessorCount, device));
  PF_HIP(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_unit[0], pf_score_given_kernel<true, true>, 64, 0));
  PF_HIP(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_unit[1], pf_score_given_kernel<true, false>, 64, 0));
  PF_HIP(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_unit[2], pf_score_given_kernel<false, false>, 64, 0));
  for (int f = 0; f < 3; ++f) h->given_wave_slots[f] = units * per_unit[f];
  return ACMPC_OK;
}

}  // namespace acmpc::pf
