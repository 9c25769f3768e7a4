// Private to the C API units (acmpc_capi*.hip): the handle behind include/acmpc.h, its error plumbing, the cache of
// captured graphs, and the helpers that cross those units.  Nothing here is exported: acmpc::capi has hidden visibility.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/acmpc.h"
#include "acmpc_alloc.h"  // alloc_once, host_alloc_once
#include "acmpc_dynamic.h"
#include "acmpc_kernels.h"
#include "acmpc_lq_box.h"

struct acmpc_ctx;

namespace acmpc {
namespace capi __attribute__((visibility("hidden"))) {

constexpr double kEps = 1e-12;  // dynamics.py:21
constexpr int kTraceBlocks = 1024;  // workgroups per launch the traced fused finalize has room for (64 candidates each)

// a few captured shapes side by side (a controller alternates between its exploring and its refining schedule);
// the least recently used slot is re-captured when a new shape arrives
constexpr int kOptGraphs = 4;

int fail(const acmpc_ctx* ctx, int code, const std::string& msg);   // (ctx == nullptr: acmpc_create's error)
int fail_hip(const acmpc_ctx* ctx, hipError_t e, const char* what);

#define ACMPC_HIP(ctx, call)                                                    \
  do {                                                                          \
    const hipError_t e_ = (call);                                               \
    if (e_ != hipSuccess) return ::acmpc::capi::fail_hip((ctx), e_, #call);     \
  } while (0)

// (a step that has failed has left its message in the handle: pass its code on)
#define ACMPC_TRY(call)                   \
  do {                                    \
    const int rc_ = (call);               \
    if (rc_ != ACMPC_OK) return rc_;      \
  } while (0)

using ::acmpc::alloc_once;
using ::acmpc::host_alloc_once;

int upload_segments(acmpc_ctx* c, int n, hipStream_t s);

// Captured launch sequences by key (a plain struct with operator== and a horizon `n`).  A slot whose executable is null
// is empty; clear() empties all of them - whatever the graphs were captured with (launch forms, a map) has changed.
template <typename Key>
struct GraphCache {
  hipGraphExec_t exec[kOptGraphs] = {};
  Key key[kOptGraphs];
  uint64_t used[kOptGraphs] = {};
  uint64_t clock = 0;

  int find(const Key& k) const {
    int slot = -1;
    for (int g = 0; g < kOptGraphs; ++g)
      if (exec[g] != nullptr && k == key[g]) slot = g;
    return slot;
  }
  void clear() {
    for (hipGraphExec_t& g : exec) {
      if (g != nullptr) (void)hipGraphExecDestroy(g);
      g = nullptr;
    }
  }
  hipGraphExec_t use(int slot) {
    used[slot] = ++clock;
    return exec[slot];
  }
  // `enqueue(s, &rc)` on the capturing stream into the least recently used slot (*slot).  The sampler's knot table goes
  // up BEFORE the capture (upload_segments synchronises).  What comes back, in this order: the rc enqueue left, its HIP
  // error (as `what`), the end of the capture, the instantiation; after any of them the slot is empty.
  template <typename Enqueue>
  int capture(acmpc_ctx* c, hipStream_t s, const Key& k, const char* what, Enqueue&& enqueue, int* slot) {
    int victim = 0;
    for (int g = 1; g < kOptGraphs; ++g)
      if (used[g] < used[victim]) victim = g;
    *slot = victim;
    if (exec[victim] != nullptr) {
      (void)hipGraphExecDestroy(exec[victim]);
      exec[victim] = nullptr;
    }
    ACMPC_TRY(upload_segments(c, k.n, s));
    hipGraph_t graph = nullptr;
    ACMPC_HIP(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc_rounds = ACMPC_OK;
    const hipError_t e = enqueue(s, &rc_rounds);
    const hipError_t e_end = hipStreamEndCapture(s, &graph);
    if (rc_rounds != ACMPC_OK || e != hipSuccess) {
      if (graph != nullptr) (void)hipGraphDestroy(graph);
      return rc_rounds != ACMPC_OK ? rc_rounds : fail_hip(c, e, what);
    }
    ACMPC_HIP(c, e_end);
    const hipError_t e_inst = hipGraphInstantiate(&exec[victim], graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e_inst != hipSuccess) exec[victim] = nullptr;
    ACMPC_HIP(c, e_inst);
    key[victim] = k;
    return ACMPC_OK;
  }
};

// acmpc_optimize as a hipGraph: the whole sample -> rollout -> finalize chain of `rounds` rounds plus the
// transfers either side of it is captured once per shape and replayed; per-call inputs travel through the pinned
// staging block `h_opt` (x0 | centre | u_ref | table | seed) and the records come back into `h_opt_records`.
struct OptKey {
  int P = 0, N = 0, n = 0, rounds = 0, has_uref = 0;
  double sigma_v = 0, sigma_k = 0, shrink = 0;
  bool operator==(const OptKey& o) const {
    return P == o.P && N == o.N && n == o.n && rounds == o.rounds && has_uref == o.has_uref &&
           sigma_v == o.sigma_v && sigma_k == o.sigma_k && shrink == o.shrink;
  }
};

// acmpc_control_tick: prologue + rounds as one captured graph per (N, n, rounds, spread); per-tick inputs travel
// through the pinned block `h_tick` (TickHeader | coords | centre), results come back into `h_tick_out`
// (record | table | QP status) by posted writes
struct TickKey {
  int N = 0, n = 0, rounds = 0, from_map = 0;
  double sigma_v = 0, sigma_k = 0, shrink = 0;
  bool operator==(const TickKey& o) const {
    return N == o.N && n == o.n && rounds == o.rounds && from_map == o.from_map && sigma_v == o.sigma_v &&
           sigma_k == o.sigma_k && shrink == o.shrink;
  }
};

}  // namespace capi
}  // namespace acmpc

struct acmpc_ctx {
  acmpc_params prm{};
  acmpc::Weights w{};
  int coef_stride = 0;

  // host copy of the packed tables
  std::vector<float> h_coef;
  int P_set = 0, n_set = 0;
  bool tables_dirty = false;
  bool frames_dirty = false;  // the verified search's frames of the current paths are not on the device yet

  // device state (created lazily)
  bool device_ready = false;
  bool touched_device = false;  // a HIP call has been made for this handle (acmpc_destroy must not make the first one)
  float* d_coef = nullptr;
  int64_t* d_partial_keys = nullptr;
  int* d_partial_feas = nullptr;
  size_t partial_slots = 0;  // slots of ONE set of partial keys / feasible counts (there are two)
  // acmpc_solve_stream_device: the finalize the last call of the stream left for the next one (or for the flush)
  bool stream_pending = false;
  acmpc::FinalizeArgs stream_fin{};
  int stream_fin_layout = 0;
  int stream_set = 0;        // the half of the partial buffers the pending finalize reads
  double* d_soft_partial = nullptr;
  size_t soft_partial_doubles = 0;

  // sampler: per-step (left knot, weight) table, uploaded when n changes
  float* d_segments = nullptr;
  int segments_n = 0;
  int knot_begin[acmpc::kKnots + 1] = {};
  float* d_centre = nullptr;  // [P][n][2] staging of acmpc_optimize (first round's centre, then u_ref)
  float* d_uref = nullptr;

  // staging for the host-pointer entry point (created on its first use)
  bool staging_ready = false;
  hipStream_t stream = nullptr;
  float* d_U = nullptr;
  float* d_x0 = nullptr;
  float* d_costs = nullptr;
  float* d_records = nullptr;
  int64_t* d_keys = nullptr;
  int* d_tickets = nullptr;  // last-workgroup counters of the in-launch finalizes (ensure_tail_buffers); zero between launches
  unsigned tick_sequence = 0;   // completion flag values of acmpc_control_tick
  float* d_trace = nullptr;  // [2][kTraceBlocks][trace_floats(max_steps)] best-candidate traces of the fused rounds' workgroups
  // mode T with exhaustive search: frames of the verified window search (acmpc_device.h: nearest_verified)
  std::vector<float> h_nn_frames;  // [P][verified_frame_floats(n)], empty when not applicable
  float* d_nn_frames = nullptr;
  int64_t* h_keys = nullptr;  // pinned
  float* h_io = nullptr;      // pinned: x0 [P][3] on the way up, records [P][record_floats] on the way down (acmpc_solve)

  acmpc::capi::GraphCache<acmpc::capi::OptKey> opt_graphs;   // acmpc_optimize's captured shapes (OptKey above)
  bool opt_ready = false;
  unsigned char* h_opt = nullptr;   // pinned
  unsigned char* d_opt = nullptr;   // device mirror of h_opt: ONE H2D copy per solve
  size_t opt_capacity = 0;
  float* h_opt_records = nullptr;   // pinned
  uint32_t* d_seed = nullptr;

  acmpc::capi::GraphCache<acmpc::capi::TickKey> tick_graphs;   // acmpc_control_tick's, under ACMPC_TICK_GRAPH (TickKey above)
  bool tick_ready = false;
  unsigned char* h_tick = nullptr;      // pinned
  unsigned char* d_tick = nullptr;
  unsigned char* h_tick_out = nullptr;  // pinned
  std::vector<double> h_map;            // bound map: centre polyline [M][2]
  double map_spacing = 0.0;
  bool map_dirty = false;
  double* d_map = nullptr;
  double* d_coords = nullptr;           // [H][3] path the window kernel builds for the prologue
  double* d_warm = nullptr;             // speed-profile iterate of the two solvers, kept between ticks
  int warm_stride = 0;
  int tick_last_n = 0;

  // the LQ plan (csrc/acmpc_lq.h; acmpc_params::lq_candidate): candidate 2 of the LAST sampling round
  std::vector<double> h_tables;         // the float64 tables of acmpc_set_paths: [P][7][n]
  float* h_lq = nullptr;                // pinned [max_problems][max_steps][2]: the plans, read by the last round in place
  std::vector<double> tick_prev_table;  // what the previous acmpc_control_tick solved: its 7 x n table ...
  double tick_prev_x0[3] = {0.0, 0.0, 0.0};   // ... and its start state (Frenet)
  std::vector<double> tick_lq_table;    // scratch: this tick's waypoints with the speed profile the host plans with
  std::vector<double> tick_lq_scratch;  // scratch: its ceiling and (unused) multipliers
  std::vector<double> tick_host_coords; // scratch: the H x 3 path of a map window, cut on the host for the plan
  int tick_prev_n = 0;                  // 0: nothing usable (first tick, or a tick that did not end with a finite plan)
  // lq_candidate = 2 (csrc/acmpc_lq_box.h): the splitting's iterate per problem, its factorisation scratch, what the last
  // plan did (acmpc_lq_box_stats) and the iteration cap (ACMPC_LQ_BOX_ITERATIONS)
  // ACMPC_START_CLOCKS: the rollout launches leave every workgroup's start time here (acmpc_rollout_start_clocks)
  bool want_start_clocks = false;
  unsigned long long* d_start_clock = nullptr;
  size_t start_clock_slots = 0;
  int start_clock_count = 0;
  std::vector<acmpc::lqbox::State> lq_box_state;
  acmpc::lqbox::Workspace lq_box_ws;
  acmpc::lqbox::Result lq_box_last;
  int lq_box_iterations = 40;

  // A/B switches of the tests and the tools: read from the environment ONCE, by acmpc_create, or set with acmpc_set_option;
  // nothing on a launch path calls getenv
  acmpc::LaunchOptions opt;
  struct Switches {
    bool no_verified_search = false, no_solo = false, no_fused_finalize = false, no_traced_finalize = false,
         no_chained_rounds = false, no_chained_stream = false, no_graph = false, no_fused_sampling = false, tick_graph = false, tick_no_flag = false, tick_no_inline_path = false, no_zero_copy = false,
         tailed_rollout = false,
         dynamic_matrix_rounds = false;   // mode D's acmpc_optimize through the control matrix: sample -> rollout -> finalize
  } sw;

  // optional timing of the rollout dispatches (acmpc_profile_*): event pairs attached to the launches
  std::vector<hipEvent_t> prof_start, prof_stop;
  size_t prof_used = 0;

  // mode D: the vehicles' float32 constants, one (acmpc_set_dynamics) or an ensemble (acmpc_set_dynamics_ensemble)
  bool has_dynamics = false;
  acmpc::VehicleEnsemble vehicles{};
  // mode D: the integration setting (acmpc_set_dynamics_integration), kept apart from the vehicles: (1, 0, 0) = off
  int substeps = 1;
  double blend_lo = 0.0, blend_hi = 0.0;
  double vehicle_L[acmpc::kMaxVehicles] = {};   // lf + lr of each vehicle in float64: the blend's 1 / L is rounded from it
  // mode D, grip identification (acmpc_score_grips): vehicle 0's float64 block - a hypothesis's peaks are derived from it -
  // and the call's device block (partial keys | best key | errors | peaks | log), per-segment values e and host staging,
  // all made on the call's first use
  double vehicle0[acmpc::kDynamicsCount] = {};
  unsigned char* d_identify = nullptr;
  float* d_identify_e = nullptr;
  size_t identify_e_floats = 0;
  std::vector<unsigned char> h_identify;
  // mode D: the rate and slip terms (acmpc_set_dynamics_terms), kept apart like the integration setting: weights 0 and
  // limits +inf = off; and the previous control (acmpc_set_previous_control), staged here until the next upload_tables
  double rate_weight[2] = {0.0, 0.0}, rate_max[2] = {HUGE_VAL, HUGE_VAL};
  double slip_weight = 0.0, slip_max = HUGE_VAL;
  std::vector<float> h_uprev;   // [uprev_P][2]
  int uprev_P = 0;              // 0: none set
  bool uprev_dirty = false;
  float* d_uprev = nullptr;     // [max_problems][2]
  // mode D: the objective (acmpc_set_dynamics_objective), kept apart like the terms: weight 0 and no ceiling = off; and the
  // progress table q [P_set][n_set], derived from the packed rows whenever they change and uploaded with them
  double progress_weight = 0.0;
  bool has_ceiling = false;
  double speed_ceiling[2] = {0.0, 0.0};   // (scale, offset)
  std::vector<float> h_progress;
  float* d_progress = nullptr;  // [max_problems][max_steps]
  // mode D: the tyre coupling (acmpc_set_dynamics_coupling), kept apart like the others: the two ratios as the float32 the
  // kernels get (+inf: no coupling on that axle).  While it is on every vehicle of the handle has finite, positive peaks.
  bool has_coupling = false;
  float coupling[2] = {HUGE_VALF, HUGE_VALF};
  // mode D: the load transfer (acmpc_set_dynamics_load_transfer), kept apart like the others: the setting (h_cg, w_frac), what
  // each vehicle block gives it in float64 - (F_zf, F_zr, e_f, e_r) - and the six float32 scalars the kernels get per vehicle
  // (c_h, w_max, a1_f, a2_f, a1_r, a2_r), derived whenever the setting or the vehicles change.  While it is on every vehicle
  // of the handle has finite, positive peaks and factors phi > 0 over +-w_max.
  bool has_load = false;
  double load_setting[2] = {0.0, 0.0};
  double vehicle_axle[acmpc::kMaxVehicles][4] = {};
  float load_const[acmpc::kMaxVehicles][6] = {};
  // mode D: the downforce (acmpc_set_dynamics_downforce), kept apart like the others: (k_f, k_r, v_sat) as the kernels get
  // them.  While it is on load_const is derived too (c_h = w_max = 0 while the load transfer is off), and every vehicle of the
  // handle has finite, positive peaks and factors > 0 over -w_max .. w_max + k_a v_sat^2.
  bool has_aero = false;
  float aero[3] = {0.0f, 0.0f, 0.0f};
  // mode D: the moving obstacles (acmpc_set_obstacles), staged here like the previous control until the next upload: positions
  // [obs_P][obs_n][obs_K][2] then radii [obs_P][obs_K] in one block, on the host and on the device (allocated by the upload
  // that first needs it, grown when a larger one arrives); and the clearance setting (acmpc_set_dynamics_clearance)
  std::vector<float> h_obs;
  int obs_P = 0, obs_n = 0, obs_K = 0;   // obs_K = 0: none set
  bool obs_dirty = false;
  float* d_obs = nullptr;
  size_t obs_capacity = 0;               // floats
  double clearance_weight = 0.0, clearance_margin = 0.0;
  // mode D: the surface table (acmpc_set_surface), staged here like the obstacles until the next upload: (mu_f, mu_r)
  // [surf_P][surf_n][2] on the host and on the device (allocated by the upload that first needs it, grown when a larger one
  // arrives)
  std::vector<float> h_surface;
  int surf_P = 0, surf_n = 0;            // surf_P = 0: none set
  bool surf_dirty = false;
  float* d_surface = nullptr;
  size_t surf_capacity = 0;              // floats
  // mode D: the actuator lag (acmpc_set_dynamics_actuator), kept apart like the others: per channel (steering, pedal) the two
  // float32 the kernels get, k = exp(-dt / tau) and m = (tau / dt)(1 - k), derived in float64 and rounded once (tau = 0: both 0,
  // which is ON); and the actuator positions at the start of the plan (acmpc_set_actuator_state), staged here like the previous
  // control until the next upload
  bool has_actuator = false;
  float actuator_k[2] = {0.0f, 0.0f}, actuator_m[2] = {0.0f, 0.0f};
  std::vector<float> h_astate;  // [astate_P][2]
  int astate_P = 0;             // 0: none set
  bool astate_dirty = false;
  float* d_astate = nullptr;    // [max_problems][2]
  // mode D: the road table (acmpc_set_road), staged here like the surface table until the next upload: (a_x, a_y, n_z, 0)
  // [road_P][road_n][4] on the host - padded as the device reads it, one aligned 16-byte row per waypoint - and on the device
  // (allocated by the upload that first needs it, grown when a larger one arrives)
  std::vector<float> h_road;
  int road_P = 0, road_n = 0;            // road_P = 0: none set
  bool road_dirty = false;
  float* d_road = nullptr;
  size_t road_capacity = 0;              // floats
  // mode D: the plan trace's device block (acmpc_trace_plans): x0 | U | states | totals | terms of ONE call, made on the call's
  // first use, kept between calls and regrown when a later call needs more
  unsigned char* d_plan_trace = nullptr;
  size_t plan_trace_bytes = 0;

  mutable std::string err;
};

namespace acmpc {
namespace capi __attribute__((visibility("hidden"))) {

// ---- acmpc_capi.hip: bring-up of the device state and the staging buffers, uploads of the tables, the shape check
int ensure_device(acmpc_ctx* c);
int ensure_staging(acmpc_ctx* c);
int ensure_matrix(acmpc_ctx* c);
int ensure_tail_buffers(acmpc_ctx* c);
int upload_previous_control(acmpc_ctx* c, hipStream_t s);
void derive_progress_table(acmpc_ctx* c);   // mode D: h_progress from h_coef (no-op in the other modes)
int upload_tables(acmpc_ctx* c, hipStream_t s);
int upload_frames(acmpc_ctx* c, hipStream_t s);
int check_shape(acmpc_ctx* c, int P, int N, int n, int layout, bool stream_call = false);
bool paths_tabulate_frames(const acmpc_ctx* c, int n);   // acmpc_set_paths leaves the verified search's frames at this horizon

// ---- acmpc_capi_solve.hip: the kernels' argument blocks from the handle, and one launch each
struct Regenerate {
  const float* d_centre;
  int centre_stride;
  const float* d_uref;
  acmpc::SampleSpec spec;
  const float* d_extra = nullptr;   // candidate 2's controls (the LQ plan), or nullptr
};
acmpc::Integration dynamics_integration(const acmpc_ctx* c);
// (acmpc_capi_dynamic.hip) the six load scalars of vehicle k as the surface step needs them while neither the load transfer nor
// the downforce is on: c_h = w_max = 0 and the vehicle's own a1, a2 (zeros for a block that has none)
void surface_load_const(const acmpc_ctx* c, int k, float* out);
acmpc::WithActuator<acmpc::WithObstacles<acmpc::TermsRoad>> dynamics_terms(const acmpc_ctx* c);   // (after the call's uploads: upload_tables)
acmpc::SampleSpec make_spec(const acmpc_ctx* c, double sigma_v, double sigma_k, uint64_t seed, uint32_t round);
// (`set`: which half of the partial keys / feasible counts - chained rounds and the stream of batches alternate)
acmpc::RolloutArgs rollout_args(const acmpc_ctx* c, const float* d_x0, const float* d_U, float* d_costs, int P, int N, int n,
                                int64_t offset, size_t set = 0);
acmpc::FinalizeArgs finalize_args(const acmpc_ctx* c, const Regenerate* regen, const int64_t* d_keys_in, int64_t* d_keys_out,
                                  const float* d_x0, const float* d_U, int P, int N, int n, int64_t offset, float* d_records,
                                  int blocks_per_problem, size_t set = 0);
void next_event_pair(acmpc_ctx* c, hipEvent_t* e0, hipEvent_t* e1);
int rollout(acmpc_ctx* c, const float* d_x0, const float* d_U, int P, int N, int n, int layout, int64_t offset,
            float* d_costs, hipStream_t s, acmpc::LaunchShape* shape_out);
int finalize(acmpc_ctx* c, const int64_t* d_keys_in, int64_t* d_keys_out, const float* d_x0, const float* d_U, int P,
             int N, int n, int layout, int64_t offset, float* d_records, int blocks_per_problem, hipStream_t s,
             const Regenerate* regen = nullptr, const float* d_coef_override = nullptr);
int rollout_sampled_dynamic(acmpc_ctx* c, const float* d_x0, const float* d_centre, int centre_stride, const float* d_uref,
                            int P, int N, int n, int64_t offset, double sigma_d, double sigma_p, uint64_t seed, uint32_t round,
                            float* d_costs, hipStream_t s);
int softmin_sampled(acmpc_ctx* c, const float* d_costs, const int64_t* d_keys, const float* d_centre, int centre_stride,
                    const float* d_uref, int P, int N, int n, int64_t offset, double sigma_v, double sigma_k, uint64_t seed,
                    uint32_t round, float* d_mean, double* d_weight_sum, hipStream_t s);
// one round through the control matrix on the handle's own buffers: sample -> rollout -> finalize (-> softmin mean)
struct RoundCentre {
  const float* centre;
  int stride;
  const float* ref;   // candidate 1, or nullptr
};
int round_centre(acmpc_ctx* c, int r, bool has_uref, int P, int n, hipStream_t s, RoundCentre* out);
int matrix_round(acmpc_ctx* c, const float* d_x0, const RoundCentre& from, const float* d_extra, const uint32_t* d_seed, int P,
                 int N, int n, int r, int rounds, double sigma_v, double sigma_k, uint64_t seed, hipStream_t s);

// ---- acmpc_capi_optimize.hip: the rounds of one optimisation, enqueued on a stream (directly or under capture)
struct OptInputs {
  const float* x0;
  const float* centre;
  const float* uref;  // or nullptr
  const float* coef;
  const float* frames = nullptr;  // mode T, exhaustive search: the verified search's frames of these paths, or nullptr
  // the LQ plans [P][n][2] (device-visible), candidate 2 of the LAST round, or nullptr; `before_last` - when set - runs on
  // the host right before that round is enqueued and fills them (acmpc_control_tick plans while the earlier launches
  // execute) and returns false when there is no plan after all
  const float* extra = nullptr;
  std::function<bool()> before_last;
};
bool use_fused_finalize(const acmpc_ctx* c, int n);
struct RoundPlan {
  bool fused_finalize;   // the last workgroup of a problem writes its record inside the round's launch
  bool traced;           // ... copied from the winning workgroup's trace
  bool chained;          // ... and only in the last round: the others hand their keys and traces to the next launch
};
RoundPlan plan_rounds(const acmpc_ctx* c, int P, int N, int n);
bool lq_plan_into(acmpc_ctx* c, const double* table, int n, const double start[3], float* out, bool start_is_pose = false,
                  int problem = 0);
int enqueue_rounds(acmpc_ctx* c, const OptInputs& in, int P, int N, int n, int rounds, double sigma_v, double sigma_k,
                   double shrink, uint64_t seed, const uint32_t* d_seed, hipStream_t s, bool fused,
                   float* final_records = nullptr, unsigned* done = nullptr, unsigned done_value = 0);

// ---- acmpc_capi_tick.hip: what a tick of H points asks of the handle (the code acmpc_control_tick fails with, and why),
// and whether its prologue tabulates the verified search's frames
int tick_check(const acmpc_ctx* c, int H, int rounds, int N, const char** why);
bool tick_tabulates_frames(const acmpc_ctx* c, int n);

}  // namespace capi
}  // namespace acmpc
