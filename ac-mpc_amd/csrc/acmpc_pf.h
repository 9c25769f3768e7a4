// Private to the particle filter's units (acmpc_pf.hip: the C API; acmpc_pf_score.hip, acmpc_pf_filter.hip: the kernels
// and their launchers): the handle behind include/acmpc.h's acmpc_pf_* entry points, its error plumbing, the kernels'
// argument structs and the launchers that cross the units.  Nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/acmpc.h"
#include "acmpc_alloc.h"
#include "acmpc_pf_grid.h"

namespace acmpc {
namespace pf __attribute__((visibility("hidden"))) {

constexpr int kBlock = 256;
constexpr double kPi = 3.14159265358979323846;

struct Track {
  const double* xy;  // [m][2]
  int m;
};

// the map's points binned into square cells (PfGrid, acmpc_pf_grid.h), on the device
struct GridIndex {
  const int* start;     // [nx * ny + 1]: cell c holds entries [start[c], start[c + 1]) of the three arrays below
  const double* x;      // the points in cell order (row-major cells, ascending point index inside a cell) ...
  const double* y;
  const int* index;     // ... and the index each has in the polyline
};
// ... and, for the first ring of a search, the points of the 3 x 3 block of cells round every cell as ONE run (each point is
// in nine blocks: 6 MB for the 35 k-point map), all three polylines in one set of arrays: a query reads two bounds and one
// run instead of six bounds and three runs, and needs no choice of pointers by polyline
struct GridBlocks {
  const int* start;     // [3 * cells + 1]: block (t, c) holds entries [start[t * cells + c], start[t * cells + c + 1])
  const double* x;      // rows of the block in order, cells of a row in order, ascending point index inside a cell
  const double* y;
  const int* index;
  int cells;            // nx * ny
};

struct ScoreArgs {
  const float* states;     // [P][3]
  const float* obs;        // [K_left + K_right][2], vehicle frame (x right, y forward)
  int k_left, k_right;
  Track centre, left, right;
  double mean, sigma, scale;
  double thr_rotation, thr_offset, thr_error;
  int32_t* track_indices;  // [P][3]
  double* minimum_offset;  // [P]
  double* heading_offset;  // [P]
  double* error;           // [P]
  double* score;           // [P]
  uint8_t* valid;          // [P]
  const int* live;         // when not null: the number of particles is read from the device (resident filter)
  // nearest points found by pf_nearest_kernel (the grid search) - the scoring kernel then skips its own scan
  const int32_t* given_index;   // [P][3] or nullptr
  const double* given_d2;       // [P][3]
  // or found by the scoring workgroup itself through the grid (pf_score_kernel<1>: a wavefront per polyline)
  int own_grid_search;
  GridIndex grid[3];
  GridGeometry geometry;
  GridBlocks blocks;
  float inv_left_m, inv_right_m;   // 1.0f / left.m, 1.0f / right.m (pf_score_given_kernel: mod_u16)
  float* publish;   // device-resident filter: the float32 score the reference publishes (_update_particle_scores), or nullptr
};

struct GridArgs {
  const float* states;   // [P][3]
  const int* live;       // or nullptr
  Track track[3];
  GridIndex grid[3];
  GridBlocks blocks;
  double x0, y0, cell;
  int nx, ny;
  int32_t* index_out;    // [P][3]
  double* d2_out;        // [P][3]
};

struct FilterArgs {
  const float* states_in;   // [n_live][3]
  const float* scores_in;   // [n_live]  (float32 scores of this update)
  const double* score;      // [n_live]  float64 scores of this update
  const uint8_t* valid;     // [n_live]
  float* states_out;        // [capacity][3]
  float* scores_out;        // [capacity]
  unsigned long long* cdf;  // [n_live] workspace: inclusive prefix sums of the kept weights
  int* kept;                // [n_live] workspace: source index of kept particle k
  int* counts;              // [4]: n_live (in/out), n_valid (out), was_reset (out), spare
  const double* centre;     // map centre line [m][2] (reset pattern)
  int m_centre;
  int capacity;             // max_particles
  int n_desired, minimum_particles;
  double sigma_x, sigma_y, sigma_yaw;
  uint32_t seed_lo, seed_hi, counter;
};

struct WideScratch {
  unsigned long long* tile_count;    // [tiles]      valid particles per tile, then (plan) their exclusive prefix sums
  unsigned long long* tile_weight;   // [tiles]      likewise the integer weights
  unsigned long long* meta;          // [6]: n before the update, n_valid, total weight, uniform (0 / 1), reset (0 / 1), n_new
};

// the device-resident filter's tiles (acmpc_pf_filter.hip), which size its scratch: resampling in tiles of kScanBlock
// particles from a capacity of kWideFilter up, the estimate in tiles of kEstimateTile
constexpr int kScanBlock = 1024;
constexpr int kWideFilter = 8192;
constexpr int kEstimateTile = 4096;

}  // namespace pf
}  // namespace acmpc

struct acmpc_pf {
  acmpc_pf_params prm{};
  // A/B switches of the tests, read from the environment once, by acmpc_pf_create
  bool no_grid = false;           // ACMPC_PF_NO_GRID: every nearest point by the exhaustive scan
  bool workgroup_score = false;   // ACMPC_PF_WORKGROUP_SCORE: pf_score_kernel<8> behind the grid search, as in rounds 2-5
  bool narrow_filter = false;     // ACMPC_PF_NARROW_FILTER: the device-resident filter's one-workgroup kernels at any capacity
  bool no_blocks = false;         // ACMPC_PF_NO_BLOCKS: the first ring row by row from the cell-ordered arrays
  int given_wave_slots[3] = {0, 0, 0};   // waves of pf_score_given_kernel's three forms the device holds at once (ensure_device)
  std::vector<double> h_track[3];
  acmpc::pf::PfGrid grid;   // over h_track: built at create, uploaded with the polylines
  double scale = 1.0;
  bool device_chosen = false;   // pf_ensure_device got as far as its device: from here on there may be something to free
  bool device_ready = false;
  double* d_track[3] = {nullptr, nullptr, nullptr};
  int* d_grid_start[3] = {nullptr, nullptr, nullptr};
  int* d_grid_index[3] = {nullptr, nullptr, nullptr};
  double* d_grid_x[3] = {nullptr, nullptr, nullptr};
  double* d_grid_y[3] = {nullptr, nullptr, nullptr};
  int* d_block_start = nullptr;
  int* d_block_index = nullptr;
  double* d_block_x = nullptr;
  double* d_block_y = nullptr;
  int32_t* d_near_index = nullptr;   // [max_particles][3]
  double* d_near_d2 = nullptr;       // [max_particles][3]
  hipStream_t stream = nullptr;
  // staging for the host-pointer entry points: ONE pinned block up (states | observation) and ONE down (all
  // per-particle results) per scoring call - at the reference's 500 particles the call is a handful of microseconds
  // of kernel and otherwise transfer round trips (it used to make nine of them)
  unsigned char* h_up = nullptr;    // pinned
  unsigned char* h_down = nullptr;  // pinned
  unsigned char* d_down = nullptr;  // [4 P doubles | 3 P int32 | P bytes]
  float* d_states = nullptr;        // [P][3] then the observation [K][2] directly behind it
  float* d_aux = nullptr;      // 2 * max_particles floats: delta / velocity, or scores
  double* d_out = nullptr;     // 8 doubles: result of the estimate kernel
  // device-resident filter: ping-pong particle buffers, this update's results, workspace of the resampling
  bool filter_ready = false;
  float* f_states[2] = {nullptr, nullptr};  // [max_particles][3]
  float* f_scores[2] = {nullptr, nullptr};
  int f_cur = 0;
  float* f_obs = nullptr;                   // [K][2]
  unsigned long long* f_cdf = nullptr;
  int* f_kept = nullptr;
  int* f_counts = nullptr;                  // [4] n_live, n_valid, was_reset
  unsigned long long* f_wide = nullptr;     // capacity >= kWideFilter: [2 tiles + 6] scratch of the tiled resampling
  double* f_partial = nullptr;              //   ... and of the tiled estimate: [tiles][8] sums, [tiles][2] spreads
  double* h_result = nullptr;               // pinned [8 doubles + 4 ints]
  mutable std::string err;
};

namespace acmpc {
namespace pf __attribute__((visibility("hidden"))) {

int pf_fail(const acmpc_pf* h, int code, const std::string& msg);   // (h == nullptr: acmpc_pf_create's error)

#define PF_HIP(h, call)                                                                                   \
  do {                                                                                                    \
    const hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess)                                                                                 \
      return ::acmpc::pf::pf_fail((h), (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? ACMPC_ENODEVICE : ACMPC_EHIP, \
                                  std::string(#call) + ": " + hipGetErrorString(e_));                     \
  } while (0)

// ---- acmpc_pf_score.hip ----
// the grid search in front of a scoring launch (fills `a.given_*`) - or, below 4 096 particles, inside it (`a.grid` ...)
hipError_t launch_nearest(const acmpc_pf* h, ScoreArgs& a, int P, hipStream_t s);
// the scoring launch behind launch_nearest
void launch_score(const acmpc_pf* h, const ScoreArgs& a, int P, hipStream_t s);
// h->given_wave_slots from the device and the three forms of the kernel (pf_ensure_device)
int query_given_wave_slots(acmpc_pf* h);

// ---- acmpc_pf_filter.hip: one launcher per sequence; `wide`: the tiled kernels (wide_filter) ----
void launch_advance(float* states, const float* delta, const float* velocity, int P, float wheelbase, float dt, hipStream_t s);
void launch_step(const acmpc_pf* h, float tyre_angle, float velocity, float sigma_yaw, float sigma_v, float dt, uint64_t seed,
                 uint32_t counter);
void launch_reset(const FilterArgs& f, hipStream_t s);
void launch_resample(const acmpc_pf* h, const FilterArgs& f, bool wide, hipStream_t s);
// (live == nullptr: P particles; otherwise the count is live[0], and counts_out receives live[0 .. 3] beside the estimate)
void launch_estimate(const acmpc_pf* h, bool wide, const float* states, const float* scores, int P, const int* live,
                     double* out, int* counts_out, hipStream_t s);

}  // namespace pf
}  // namespace acmpc
