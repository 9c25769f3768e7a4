// C ABI of the rollout-and-cost engine (include/acmpc.h).  This unit owns the handle's life - create, options, destroy -
// the host-side table preparation (acmpc_set_paths, the verified search's frames), the lazy bring-up of the device state
// and the staging buffers, and the small exports (version, keys, LQ plans, pinned memory).  The launch sequences are in
// acmpc_capi_solve.hip, _optimize.hip and _tick.hip, mode D's setters in _dynamic.hip, RCCL in _rccl.hip.  No CPU fallback
// exists: every compute entry point needs the GPU.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <new>

#include "acmpc_ctx.h"
#include "acmpc_frames.h"
#include "acmpc_lq.h"

using namespace acmpc::capi;

namespace {

thread_local std::string g_create_error;

}  // namespace

namespace acmpc {
namespace capi __attribute__((visibility("hidden"))) {

int fail(const acmpc_ctx* ctx, int code, const std::string& msg) {
  if (ctx != nullptr) {
    ctx->err = msg;
  } else {
    g_create_error = msg;
  }
  return code;
}

int fail_hip(const acmpc_ctx* ctx, hipError_t e, const char* what) {
  (void)hipGetLastError();  // do not leave the error behind for the next launch check (of this or any other library)
  const bool nodev = (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver ||
                      e == hipErrorNotInitialized);
  return fail(ctx, nodev ? ACMPC_ENODEVICE : ACMPC_EHIP,
              std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
}

// Frames of mode T's verified nearest-waypoint search for P paths of n packed waypoint rows (acmpc_frames.h has the
// arithmetic and why it is sound).  O(n^2) per path, hence the cap on n.
static constexpr int kMaxVerifiedSteps = 256;

static void verified_frames(const float* coef, int P, int n, std::vector<float>* out) {
  constexpr int W = acmpc::kVerifiedWindow;
  const int windows = n - W + 1;
  const int floats = acmpc::verified_frame_floats(n);
  out->assign(static_cast<size_t>(P) * floats, 0.0f);
  std::vector<acmpc::frames::Geometry> geometry(static_cast<size_t>(windows));
  for (int p = 0; p < P; ++p) {
    const float* t = coef + static_cast<size_t>(p) * n * acmpc::kCoefT;
    // positions in the path's own frame, as the kernels take them (acmpc_device.h: start_temporal): float32 differences
    const float ox = t[0], oy = t[1];
    auto at = [t, ox, oy](int m, double& x, double& y) {
      x = static_cast<double>(t[m * acmpc::kCoefT] - ox);
      y = static_cast<double>(t[m * acmpc::kCoefT + 1] - oy);
    };
    double wn = 0.0;   // largest norm of a waypoint
    bool finite = true;
    for (int m = 0; m < n; ++m) {
      double x, y;
      at(m, x, y);
      finite = finite && std::isfinite(x) && std::isfinite(y);
      wn = std::max(wn, std::sqrt(x * x + y * y));
    }
    float largest_gap2 = 0.0f;
    for (int m = 0; m + 1 < n; ++m) {
      const float gap2 = acmpc::frames::squared_gap(t[(m + 1) * acmpc::kCoefT] - ox, t[(m + 1) * acmpc::kCoefT + 1] - oy,
                                                    t[m * acmpc::kCoefT] - ox, t[m * acmpc::kCoefT + 1] - oy);
      largest_gap2 = (gap2 > largest_gap2) ? gap2 : largest_gap2;
    }
    const int first = acmpc::frames::near_first(largest_gap2);
    double slab_max = 0.0;
    for (int lo = 0; lo < windows; ++lo) {
      double R = finite ? acmpc::frames::far_distance(at, n, lo, first) : 0.0;
      const int near = finite ? acmpc::frames::choose_near(at, n, lo, first, R) : first;
      geometry[lo] = acmpc::frames::window_geometry<0>(at, n, lo, finite, near, R);
      if (geometry[lo].usable) slab_max = std::max(slab_max, geometry[lo].aA - geometry[lo].aB);
    }
    const acmpc::frames::Scale scale = acmpc::frames::path_scale(wn, slab_max);
    float* table = out->data() + static_cast<size_t>(p) * floats;
    for (int lo = 0; lo < windows; ++lo) acmpc::frames::frame_row(geometry[lo], scale, table + acmpc::kFrameStride * lo);
  }
}

// mode T with the exhaustive search, from the verified window's width up to the cap above
bool paths_tabulate_frames(const acmpc_ctx* c, int n) {
  return c->prm.mode == ACMPC_MODE_TEMPORAL && c->prm.nn_ahead < 0 && n >= acmpc::kVerifiedWindow && n <= kMaxVerifiedSteps;
}

int ensure_device(acmpc_ctx* c) {
  if (c->device_ready) return ACMPC_OK;
  c->touched_device = true;
  int count = 0;
  const hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) {
    return fail(c, ACMPC_ENODEVICE,
                "no HIP device visible: the rollout path has no CPU fallback (hipGetDeviceCount: " +
                    std::string(e == hipSuccess ? "0 devices" : hipGetErrorString(e)) + ")");
  }
  if (c->prm.device >= 0) ACMPC_HIP(c, hipSetDevice(c->prm.device));
  const acmpc_params& p = c->prm;
  const size_t coef_floats = static_cast<size_t>(p.max_problems) * p.max_steps * c->coef_stride;
  const size_t partials = static_cast<size_t>(p.max_problems) * acmpc::max_blocks_per_problem(p.max_candidates);
  c->soft_partial_doubles = static_cast<size_t>(p.max_problems) * acmpc::softmin_chunks(p.max_candidates) *
                            (4 * static_cast<size_t>(p.max_steps) + 1);
  ACMPC_HIP(c, alloc_once(&c->d_coef, coef_floats * sizeof(float)));
  // (two sets: chained optimisation rounds alternate, a round reads the keys its predecessor wrote while it writes its own)
  ACMPC_HIP(c, alloc_once(&c->d_partial_keys, 2 * partials * sizeof(int64_t)));
  ACMPC_HIP(c, alloc_once(&c->d_partial_feas, 2 * partials * sizeof(int)));
  c->partial_slots = partials;
  ACMPC_HIP(c, alloc_once(&c->d_soft_partial, c->soft_partial_doubles * sizeof(double)));
  ACMPC_HIP(c, alloc_once(&c->d_segments, static_cast<size_t>(p.max_steps) * 2 * sizeof(float)));
  if (p.mode == ACMPC_MODE_TEMPORAL && p.nn_ahead < 0)
    ACMPC_HIP(c, alloc_once(&c->d_nn_frames, static_cast<size_t>(p.max_problems) * sizeof(float) *
                                                 acmpc::verified_frame_floats(std::max(std::min(p.max_steps, kMaxVerifiedSteps),
                                                                                       acmpc::kVerifiedWindow))));
  if (p.mode == ACMPC_MODE_DYNAMIC) ACMPC_HIP(c, alloc_once(&c->d_uprev, static_cast<size_t>(p.max_problems) * 2 * sizeof(float)));
  if (p.mode == ACMPC_MODE_DYNAMIC) ACMPC_HIP(c, alloc_once(&c->d_astate, static_cast<size_t>(p.max_problems) * 2 * sizeof(float)));
  if (p.mode == ACMPC_MODE_DYNAMIC)
    ACMPC_HIP(c, alloc_once(&c->d_progress, static_cast<size_t>(p.max_problems) * p.max_steps * sizeof(float)));
  c->device_ready = true;
  return ACMPC_OK;
}

// mode D: the previous control staged by acmpc_set_previous_control goes up on the stream of the call that reads it
// and with it the obstacles staged by acmpc_set_obstacles (one block: positions, then radii)
int upload_previous_control(acmpc_ctx* c, hipStream_t s) {
  if (c->obs_dirty && c->obs_K != 0 && c->device_ready) {
    if (c->obs_capacity < c->h_obs.size()) {   // (hipFree waits for whatever still reads the old block)
      (void)hipFree(c->d_obs);
      c->d_obs = nullptr;
      c->obs_capacity = 0;
      ACMPC_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_obs), c->h_obs.size() * sizeof(float)));
      c->obs_capacity = c->h_obs.size();
    }
    ACMPC_HIP(c, hipMemcpyAsync(c->d_obs, c->h_obs.data(), c->h_obs.size() * sizeof(float), hipMemcpyHostToDevice, s));
    c->obs_dirty = false;
  }
  if (c->surf_dirty && c->surf_P != 0 && c->device_ready) {   // and the surface table staged by acmpc_set_surface
    if (c->surf_capacity < c->h_surface.size()) {
      (void)hipFree(c->d_surface);
      c->d_surface = nullptr;
      c->surf_capacity = 0;
      ACMPC_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_surface), c->h_surface.size() * sizeof(float)));
      c->surf_capacity = c->h_surface.size();
    }
    ACMPC_HIP(c, hipMemcpyAsync(c->d_surface, c->h_surface.data(), c->h_surface.size() * sizeof(float), hipMemcpyHostToDevice, s));
    c->surf_dirty = false;
  }
  if (c->road_dirty && c->road_P != 0 && c->device_ready) {   // and the road table staged by acmpc_set_road
    if (c->road_capacity < c->h_road.size()) {
      (void)hipFree(c->d_road);
      c->d_road = nullptr;
      c->road_capacity = 0;
      ACMPC_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_road), c->h_road.size() * sizeof(float)));
      c->road_capacity = c->h_road.size();
    }
    ACMPC_HIP(c, hipMemcpyAsync(c->d_road, c->h_road.data(), c->h_road.size() * sizeof(float), hipMemcpyHostToDevice, s));
    c->road_dirty = false;
  }
  if (c->astate_dirty && c->astate_P != 0 && c->d_astate != nullptr) {   // and the actuator positions staged by acmpc_set_actuator_state
    ACMPC_HIP(c, hipMemcpyAsync(c->d_astate, c->h_astate.data(), c->h_astate.size() * sizeof(float), hipMemcpyHostToDevice, s));
    c->astate_dirty = false;
  }
  if (!c->uprev_dirty || c->uprev_P == 0 || c->d_uprev == nullptr) return ACMPC_OK;
  ACMPC_HIP(c, hipMemcpyAsync(c->d_uprev, c->h_uprev.data(), c->h_uprev.size() * sizeof(float), hipMemcpyHostToDevice, s));
  c->uprev_dirty = false;
  return ACMPC_OK;
}

int upload_tables(acmpc_ctx* c, hipStream_t s) {
  if (c->P_set == 0) return fail(c, ACMPC_ESTATE, "acmpc_set_paths has not been called");
  ACMPC_TRY(upload_previous_control(c, s));
  // pageable source: hipMemcpyAsync stages it before returning, so the host vectors may change afterwards.  (Round 4 tried
  // a page-locked staging block for small tables - a memcpy and a true asynchronous packet: 0.7 us of a 91 us
  // set_paths + solve, not worth the bookkeeping of when the block is free again.)
  ACMPC_TRY(upload_frames(c, s));
  if (!c->tables_dirty) return ACMPC_OK;
  const size_t bytes = static_cast<size_t>(c->P_set) * c->n_set * c->coef_stride * sizeof(float);
  ACMPC_HIP(c, hipMemcpyAsync(c->d_coef, c->h_coef.data(), bytes, hipMemcpyHostToDevice, s));
  if (c->d_progress != nullptr)   // mode D: the progress table of these rows, [P][n]
    ACMPC_HIP(c, hipMemcpyAsync(c->d_progress, c->h_progress.data(), c->h_progress.size() * sizeof(float), hipMemcpyHostToDevice, s));
  c->tables_dirty = false;
  return ACMPC_OK;
}

// Mode D's progress table ("Progress and ceiling") from the packed float32 rows, whoever put them
// there: in float64, in the order written, no fused multiply-add (the unit is built with -ffp-contract=off)
//   S_0 = 0, S_m = S_{m-1} + sqrt(dx dx + dy dy);  q_m = float32(S_m - (c_m (x_m - x_0) + s_m (y_m - y_0)))
// so that with positions relative to the first waypoint fma(s_j, Y, fma(c_j, X, q_j)) is the arc length of waypoint j plus
// the along-track offset from it.
void derive_progress_table(acmpc_ctx* c) {
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return;
  const int P = c->P_set, n = c->n_set, stride = c->coef_stride;
  c->h_progress.resize(static_cast<size_t>(P) * n);
  for (int p = 0; p < P; ++p) {
    const float* rows = c->h_coef.data() + static_cast<size_t>(p) * n * stride;
    float* q = c->h_progress.data() + static_cast<size_t>(p) * n;
    const double x0 = rows[0], y0 = rows[1];
    double S = 0.0;
    for (int m = 0; m < n; ++m) {
      const float* r = rows + static_cast<size_t>(m) * stride;
      const double x = r[0], y = r[1], cm = r[2], sm = r[3];
      if (m > 0) {
        const double dx = x - static_cast<double>(r[0 - stride]), dy = y - static_cast<double>(r[1 - stride]);
        S = S + std::sqrt(dx * dx + dy * dy);
      }
      q[m] = static_cast<float>(S - (cm * (x - x0) + sm * (y - y0)));
    }
  }
}

// The captured optimisation carries the coefficient table in its staging block but not the frames of mode T's
// verified nearest-waypoint search, which the three-kernel form of a round reads (rollout(): a.nn_frames): bring them
// up to date on the launch stream before the graph runs.
int upload_frames(acmpc_ctx* c, hipStream_t s) {
  if (!c->frames_dirty || c->h_nn_frames.empty() || c->d_nn_frames == nullptr) return ACMPC_OK;
  ACMPC_HIP(c, hipMemcpyAsync(c->d_nn_frames, c->h_nn_frames.data(), c->h_nn_frames.size() * sizeof(float),
                              hipMemcpyHostToDevice, s));
  c->frames_dirty = false;
  return ACMPC_OK;
}

int check_shape(acmpc_ctx* c, int P, int N, int n, int layout, bool stream_call) {
  if (c->stream_pending && !stream_call)
    return fail(c, ACMPC_ESTATE, "a batch of acmpc_solve_stream_device is pending: acmpc_solve_stream_flush first");
  if (c->prm.mode == ACMPC_MODE_DYNAMIC && !c->has_dynamics)
    return fail(c, ACMPC_ESTATE, "mode D: acmpc_set_dynamics has not been called");
  if (P < 1 || N < 1 || n < 1) return fail(c, ACMPC_EINVAL, "P, N and n must be positive");
  if (layout != ACMPC_LAYOUT_CANDIDATE_MAJOR && layout != ACMPC_LAYOUT_STEP_MAJOR)
    return fail(c, ACMPC_EINVAL, "unknown layout");
  if (P > c->prm.max_problems || N > c->prm.max_candidates || n > c->prm.max_steps) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "shape (P=%d, N=%d, n=%d) exceeds the handle's capacity (%d, %d, %d)", P, N, n,
                  c->prm.max_problems, c->prm.max_candidates, c->prm.max_steps);
    return fail(c, ACMPC_ECAPACITY, buf);
  }
  if (c->P_set == 0) return fail(c, ACMPC_ESTATE, "acmpc_set_paths has not been called");
  if (P != c->P_set || n != c->n_set) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "shape (P=%d, n=%d) does not match the tables set (P=%d, n=%d)", P, n, c->P_set,
                  c->n_set);
    return fail(c, ACMPC_EINVAL, buf);
  }
  if (c->prm.mode == ACMPC_MODE_DYNAMIC && c->uprev_P != 0 && P != c->uprev_P) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "P=%d does not match the previous controls set (P=%d): acmpc_set_previous_control", P,
                  c->uprev_P);
    return fail(c, ACMPC_ESTATE, buf);
  }
  if (c->prm.mode == ACMPC_MODE_DYNAMIC && c->astate_P != 0 && P != c->astate_P) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "P=%d does not match the actuator positions set (P=%d): acmpc_set_actuator_state", P, c->astate_P);
    return fail(c, ACMPC_ESTATE, buf);
  }
  if (c->prm.mode == ACMPC_MODE_DYNAMIC && c->obs_K != 0 && (P != c->obs_P || n != c->obs_n)) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "shape (P=%d, n=%d) does not match the obstacles set (P=%d, n=%d): acmpc_set_obstacles", P, n,
                  c->obs_P, c->obs_n);
    return fail(c, ACMPC_ESTATE, buf);
  }
  if (c->prm.mode == ACMPC_MODE_DYNAMIC && c->surf_P != 0 && (P != c->surf_P || n != c->surf_n)) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "shape (P=%d, n=%d) does not match the surface table set (P=%d, n=%d): acmpc_set_surface", P, n,
                  c->surf_P, c->surf_n);
    return fail(c, ACMPC_ESTATE, buf);
  }
  if (c->prm.mode == ACMPC_MODE_DYNAMIC && c->road_P != 0 && (P != c->road_P || n != c->road_n)) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "shape (P=%d, n=%d) does not match the road table set (P=%d, n=%d): acmpc_set_road", P, n,
                  c->road_P, c->road_n);
    return fail(c, ACMPC_ESTATE, buf);
  }
  return ACMPC_OK;
}

// what the in-launch finalize of the fused rounds and of the one-launch solve needs: ticket counters (zero between
// launches) and the workgroups' traces
int ensure_tail_buffers(acmpc_ctx* c) {
  if (c->d_tickets != nullptr && c->d_trace != nullptr) return ACMPC_OK;
  c->touched_device = true;
  const acmpc_params& p = c->prm;
  // [P][kTicketGroups + 1] for the fused rounds, [P][up to kTicketGroupsMax + 1] for the one-launch solve (which takes at
  // most kSoloBlocks workgroups, so at most that many problems), every counter on a line of its own
  const size_t ticket_ints =
      std::max(static_cast<size_t>(p.max_problems) * (acmpc::kTicketGroups + 1),
               static_cast<size_t>(std::min(p.max_problems, acmpc::kSoloBlocks)) * (acmpc::kTicketGroupsMax + 1)) *
      acmpc::kTicketStride;
  if (c->d_tickets == nullptr) {
    ACMPC_HIP(c, alloc_once(&c->d_tickets, ticket_ints * sizeof(int)));
    ACMPC_HIP(c, hipMemset(c->d_tickets, 0, ticket_ints * sizeof(int)));
    ACMPC_HIP(c, hipStreamSynchronize(nullptr));  // the callers' streams do not order against the null stream
  }
  ACMPC_HIP(c, alloc_once(&c->d_trace, 2 * static_cast<size_t>(kTraceBlocks) * acmpc::trace_floats(p.max_steps) * sizeof(float)));
  return ACMPC_OK;
}

// the control matrix of the host-pointer entry points.  Mode D allocates it on first use: its acmpc_optimize draws the
// candidates inside the rollout and needs none (acmpc_solve and ACMPC_DYNAMIC_MATRIX_ROUNDS do)
int ensure_matrix(acmpc_ctx* c) {
  const acmpc_params& p = c->prm;
  ACMPC_HIP(c, alloc_once(&c->d_U, static_cast<size_t>(p.max_problems) * p.max_candidates * p.max_steps * 2 * sizeof(float)));
  return ACMPC_OK;
}

int ensure_staging(acmpc_ctx* c) {
  if (c->staging_ready) return ACMPC_OK;
  c->touched_device = true;
  const acmpc_params& p = c->prm;
  const size_t cand = static_cast<size_t>(p.max_problems) * p.max_candidates;
  ACMPC_HIP(c, alloc_once(&c->d_centre, static_cast<size_t>(p.max_problems) * p.max_steps * 2 * sizeof(float)));
  ACMPC_HIP(c, alloc_once(&c->d_uref, static_cast<size_t>(p.max_problems) * p.max_steps * 2 * sizeof(float)));
  if (c->stream == nullptr) ACMPC_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if (p.mode != ACMPC_MODE_DYNAMIC) {
    ACMPC_TRY(ensure_matrix(c));
  }
  const size_t state_floats = p.mode == ACMPC_MODE_DYNAMIC ? acmpc::kDynamicStateFloats : 3;
  ACMPC_HIP(c, alloc_once(&c->d_x0, static_cast<size_t>(p.max_problems) * state_floats * sizeof(float)));
  ACMPC_HIP(c, alloc_once(&c->d_costs, cand * sizeof(float)));
  ACMPC_HIP(c, alloc_once(&c->d_records,
                          static_cast<size_t>(p.max_problems) * acmpc_record_floats(p.max_steps) * sizeof(float)));
  ACMPC_HIP(c, alloc_once(&c->d_keys, static_cast<size_t>(p.max_problems) * sizeof(int64_t)));
  ACMPC_TRY(ensure_tail_buffers(c));
  ACMPC_HIP(c, host_alloc_once(&c->h_keys, static_cast<size_t>(p.max_problems) * sizeof(int64_t)));
  ACMPC_HIP(c, host_alloc_once(&c->h_io, (static_cast<size_t>(p.max_problems) * (state_floats + acmpc_record_floats(p.max_steps)) + 4) * sizeof(float)));
  if (p.lq_candidate != 0 && c->h_lq == nullptr) {
    const size_t lq_bytes = static_cast<size_t>(p.max_problems) * p.max_steps * 2 * sizeof(float);
    ACMPC_HIP(c, host_alloc_once(&c->h_lq, lq_bytes));
    std::memset(c->h_lq, 0, lq_bytes);
  }
  c->staging_ready = true;
  return ACMPC_OK;
}

// ---- A/B switches: names as the environment spells them; a null or empty value, or "0" for the boolean ones, is the default
static const char* const kOptionNames[] = {
    "ACMPC_SHAPE", "ACMPC_T_PACK", "ACMPC_NO_TILE", "ACMPC_TILE_ROWS", "ACMPC_TILE_TABLE", "ACMPC_NO_TRIO_ROUNDS",
    "ACMPC_NO_QUAD_ROUNDS", "ACMPC_NO_PAIR_ROUNDS", "ACMPC_SOLO_REGISTERS", "ACMPC_SOLO_SPLIT", "ACMPC_NO_VERIFIED_SEARCH",
    "ACMPC_NO_SOLO", "ACMPC_NO_FUSED_FINALIZE", "ACMPC_NO_TRACED_FINALIZE", "ACMPC_NO_CHAINED_ROUNDS", "ACMPC_NO_GRAPH",
    "ACMPC_NO_FUSED_SAMPLING", "ACMPC_TICK_GRAPH", "ACMPC_TICK_NO_FLAG", "ACMPC_TICK_NO_INLINE_PATH", "ACMPC_NO_ZERO_COPY", "ACMPC_TAILED_ROLLOUT", "ACMPC_NO_GROUP_FINALIZE", "ACMPC_FINALIZE_WAVES",
    "ACMPC_NO_CHAINED_STREAM", "ACMPC_LQ_BOX_ITERATIONS", "ACMPC_START_CLOCKS", "ACMPC_DYNAMIC_MATRIX_ROUNDS",
    "ACMPC_CONFORMANT_SYNC"};   // (last: it sets several of the switches above, and wins over them when both are in the environment)

static bool apply_option(acmpc_ctx* c, const char* name, const char* value) {
  const std::string key(name);
  const bool present = value != nullptr && value[0] != '\0';
  const bool on = present && !(value[0] == '0' && value[1] == '\0');
  auto tri = [&](int* field) { *field = present ? (value[0] == '1' ? 1 : 0) : -1; return true; };
  acmpc::LaunchOptions& o = c->opt;
  if (key == "ACMPC_SHAPE") {
    o.shape_block = o.shape_cpt = 0;
    if (present && std::sscanf(value, "%d,%d", &o.shape_block, &o.shape_cpt) != 2) o.shape_block = o.shape_cpt = 0;
    return true;
  }
  if (key == "ACMPC_T_PACK") { o.temporal_pack = present ? (value[0] == '1' ? 1 : 2) : 0; return true; }
  if (key == "ACMPC_NO_TILE") { o.no_tile = on; return true; }
  if (key == "ACMPC_TILE_ROWS") { o.tile_rows = present ? std::atoi(value) : -1; return true; }
  if (key == "ACMPC_TILE_TABLE") { o.tile_table = present ? (value[0] == 'l' ? 1 : 2) : 0; return true; }
  if (key == "ACMPC_NO_TRIO_ROUNDS") { o.no_trio_rounds = on; return true; }
  if (key == "ACMPC_NO_QUAD_ROUNDS") { o.no_quad_rounds = on; return true; }
  if (key == "ACMPC_NO_PAIR_ROUNDS") { o.no_pair_rounds = on; return true; }
  if (key == "ACMPC_SOLO_REGISTERS") return tri(&o.solo_registers);
  if (key == "ACMPC_SOLO_SPLIT") return tri(&o.solo_split);
  if (key == "ACMPC_NO_GROUP_FINALIZE") { o.no_group_finalize = on; return true; }
  if (key == "ACMPC_FINALIZE_WAVES") { o.finalize_waves = on; return true; }
  acmpc_ctx::Switches& w = c->sw;
  if (key == "ACMPC_NO_VERIFIED_SEARCH") { w.no_verified_search = on; return true; }
  if (key == "ACMPC_NO_SOLO") { w.no_solo = on; return true; }
  if (key == "ACMPC_NO_FUSED_FINALIZE") { w.no_fused_finalize = on; return true; }
  if (key == "ACMPC_NO_TRACED_FINALIZE") { w.no_traced_finalize = on; return true; }
  if (key == "ACMPC_NO_CHAINED_ROUNDS") { w.no_chained_rounds = on; return true; }
  if (key == "ACMPC_NO_CHAINED_STREAM") { w.no_chained_stream = on; return true; }
  if (key == "ACMPC_NO_GRAPH") { w.no_graph = on; return true; }
  if (key == "ACMPC_NO_FUSED_SAMPLING") { w.no_fused_sampling = on; return true; }
  if (key == "ACMPC_TICK_GRAPH") { w.tick_graph = on; return true; }
  if (key == "ACMPC_TICK_NO_FLAG") { w.tick_no_flag = on; return true; }
  if (key == "ACMPC_TICK_NO_INLINE_PATH") { w.tick_no_inline_path = on; return true; }
  if (key == "ACMPC_NO_ZERO_COPY") { w.no_zero_copy = on; return true; }
  if (key == "ACMPC_TAILED_ROLLOUT") { w.tailed_rollout = on; return true; }
  if (key == "ACMPC_START_CLOCKS") { c->want_start_clocks = on; return true; }
  if (key == "ACMPC_DYNAMIC_MATRIX_ROUNDS") { w.dynamic_matrix_rounds = on; return true; }
  if (key == "ACMPC_CONFORMANT_SYNC") {
    // ONE switch for the forms that stay inside the HSA memory model and HIP's barrier rule (include/acmpc.h): every solve,
    // round and batch as separate launches, nothing published between workgroups of one launch, no wave of a workgroup
    // ending while the others still meet at a barrier, completion by hipStreamSynchronize.  Sets (or, off, clears) the
    // switches that select them - the one-launch solve, the in-launch finalize (with it the traced finalize, the chained
    // rounds and the multi-wave rounds, which need it), the chained stream, the tick's completion flag - and the tailed
    // rollout off.  The same bits either way (tests/test_gpu_conformant.py); INTEGRATION.md section 6 has what it costs.
    w.no_solo = w.no_fused_finalize = w.no_chained_stream = w.tick_no_flag = on;
    if (on) w.tailed_rollout = false;
    return true;
  }
  if (key == "ACMPC_LQ_BOX_ITERATIONS") { c->lq_box_iterations = present ? std::max(0, std::atoi(value)) : 40; return true; }
  return false;
}

}  // namespace capi
}  // namespace acmpc

extern "C" {

const char* acmpc_version(void) { return "acmpc-hip 0.1 gfx950"; }

int32_t acmpc_record_floats(int32_t n) { return ACMPC_REC_HEADER + 2 * n + 3 * (n + 1); }

int acmpc_lq_plan(const double* table, int32_t n, const double x0[3], const double step_cost[3], const double r_term[2],
                  const double final_cost[3], const float u_min[2], const float u_max[2], float* plan) {
  if (table == nullptr || x0 == nullptr || step_cost == nullptr || r_term == nullptr || final_cost == nullptr ||
      u_min == nullptr || u_max == nullptr || plan == nullptr || n < 1)
    return ACMPC_EINVAL;
  return acmpc::lq::plan(table, n, x0, step_cost, r_term, final_cost, u_min, u_max, plan) ? ACMPC_OK : ACMPC_ESTATE;
}

int acmpc_lq_box_plan(const double* table, int32_t n, const double x0[3], const double step_cost[3], const double r_term[2],
                      const double final_cost[3], const float u_min[2], const float u_max[2], double margin, double w_bound,
                      int32_t iterations, double* state, float* plan, double* info) {
  if (table == nullptr || x0 == nullptr || step_cost == nullptr || r_term == nullptr || final_cost == nullptr ||
      u_min == nullptr || u_max == nullptr || plan == nullptr || state == nullptr || info == nullptr || n < 1)
    return ACMPC_EINVAL;
  if (!acmpc::lq::plan(table, n, x0, step_cost, r_term, final_cost, u_min, u_max, plan)) return ACMPC_ESTATE;
  acmpc::lqbox::State st;
  const size_t m = static_cast<size_t>(n) * 2;
  if (state[0] == static_cast<double>(n)) {   // a warm iterate: wx, wu, lx, lu behind the horizon it belongs to
    st.n = n;
    st.wx.assign(state + 1, state + 1 + m);
    st.wu.assign(state + 1 + m, state + 1 + 2 * m);
    st.lx.assign(state + 1 + 2 * m, state + 1 + 3 * m);
    st.lu.assign(state + 1 + 3 * m, state + 1 + 4 * m);
  }
  acmpc::lqbox::Workspace ws;
  const acmpc::lqbox::Result r = acmpc::lqbox::refine(table, n, x0, step_cost, r_term, final_cost, u_min, u_max, margin,
                                                      w_bound, iterations, st, ws, plan);
  state[0] = static_cast<double>(st.n);
  if (st.n == n) {
    std::copy(st.wx.begin(), st.wx.end(), state + 1);
    std::copy(st.wu.begin(), st.wu.end(), state + 1 + m);
    std::copy(st.lx.begin(), st.lx.end(), state + 1 + 2 * m);
    std::copy(st.lu.begin(), st.lu.end(), state + 1 + 3 * m);
  }
  info[0] = r.iterations, info[1] = r.chosen, info[2] = r.triggered ? 1.0 : 0.0, info[3] = r.cost.J, info[4] = r.cost.V;
  return ACMPC_OK;
}

int acmpc_lq_box_stats(const acmpc_ctx* c, double info[5]) {
  if (c == nullptr || info == nullptr) return ACMPC_EINVAL;
  const acmpc::lqbox::Result& r = c->lq_box_last;
  info[0] = r.iterations, info[1] = r.chosen, info[2] = r.triggered ? 1.0 : 0.0, info[3] = r.cost.J, info[4] = r.cost.V;
  return ACMPC_OK;
}

int64_t acmpc_pack_key(float cost, uint32_t index) { return acmpc::pack_key(cost, index); }

float acmpc_key_cost(int64_t key) {
  const int32_t hi = static_cast<int32_t>(key >> 32);
  const int32_t bits = (hi >= 0) ? hi : (hi ^ 0x7fffffff);
  float f;
  std::memcpy(&f, &bits, sizeof f);
  return f;
}

uint32_t acmpc_key_index(int64_t key) { return static_cast<uint32_t>(key & 0xffffffffLL); }

const char* acmpc_last_error(const acmpc_ctx* ctx) { return ctx != nullptr ? ctx->err.c_str() : g_create_error.c_str(); }

int acmpc_create(const acmpc_params* params, acmpc_ctx** out) {
  if (params == nullptr || out == nullptr) return fail(nullptr, ACMPC_EINVAL, "null argument");
  *out = nullptr;
  if (params->struct_size != sizeof(acmpc_params)) return fail(nullptr, ACMPC_EINVAL, "acmpc_params size mismatch");
  if (params->mode != ACMPC_MODE_SPATIAL && params->mode != ACMPC_MODE_TEMPORAL && params->mode != ACMPC_MODE_DYNAMIC)
    return fail(nullptr, ACMPC_EINVAL, "unknown mode");
  if (params->mode == ACMPC_MODE_DYNAMIC && params->lq_candidate != 0)
    return fail(nullptr, ACMPC_EINVAL, "mode D: lq_candidate must be 0 (the LQ plan is for the spatial model)");
  if (params->mode == ACMPC_MODE_DYNAMIC && params->max_steps > acmpc::kDynamicMaxSteps)
    return fail(nullptr, ACMPC_EINVAL, "mode D: max_steps <= 512");
  if (params->max_problems < 1 || params->max_candidates < 1 || params->max_steps < 1)
    return fail(nullptr, ACMPC_EINVAL, "capacities must be positive");
  if (params->nn_ahead >= 0 && (params->nn_back < 0 || params->nn_back + params->nn_ahead + 1 > 64))
    return fail(nullptr, ACMPC_EINVAL, "nearest-waypoint window: need nn_back >= 0 and at most 64 waypoints");
  if (params->centre_update != 0 && params->centre_update != 1)
    return fail(nullptr, ACMPC_EINVAL, "centre_update must be 0 (argmin) or 1 (softmin mean)");
  if (params->lq_candidate < 0 || params->lq_candidate > 2)
    return fail(nullptr, ACMPC_EINVAL, "lq_candidate must be 0, 1 (LQ plan) or 2 (LQ plan + box-constrained refinement)");
  if (params->max_steps > 1024)
    return fail(nullptr, ACMPC_EINVAL, "the waypoint table and the winner record are staged in LDS: max_steps <= 1024");
  if (params->max_problems > 65535)
    return fail(nullptr, ACMPC_EINVAL, "problems map to the grid's y dimension: max_problems <= 65535");
  acmpc_ctx* c = new (std::nothrow) acmpc_ctx();
  if (c == nullptr) return fail(nullptr, ACMPC_EINVAL, "out of host memory");
  c->prm = *params;
  c->coef_stride = params->mode == ACMPC_MODE_SPATIAL ? ACMPC_COEF_STRIDE_SPATIAL : ACMPC_COEF_STRIDE_TEMPORAL;
  acmpc::Weights& w = c->w;
  w.q0 = static_cast<float>(params->step_cost[0]);
  w.q1 = static_cast<float>(params->step_cost[1]);
  w.q2 = static_cast<float>(params->step_cost[2]);
  w.r0 = static_cast<float>(params->r_term[0]);
  w.r1 = static_cast<float>(params->r_term[1]);
  w.qn0 = static_cast<float>(params->final_cost[0]);
  w.qn1 = static_cast<float>(params->final_cost[1]);
  w.qn2 = static_cast<float>(params->final_cost[2]);
  w.hq0 = 0.5f * w.q0;
  w.hq1 = 0.5f * w.q1;
  w.hr0 = 0.5f * w.r0;
  w.hr1 = 0.5f * w.r1;
  w.hqn0 = 0.5f * w.qn0;
  w.hqn1 = 0.5f * w.qn1;
  w.hqn2 = 0.5f * w.qn2;
  w.ulo0 = static_cast<float>(params->u_min[0]);
  w.ulo1 = static_cast<float>(params->u_min[1]);
  w.uhi0 = static_cast<float>(params->u_max[0]);
  w.uhi1 = static_cast<float>(params->u_max[1]);
  w.tmin = static_cast<float>(params->t_min);
  w.wbound = static_cast<float>(params->w_bound);
  w.dt = static_cast<float>(params->dt);
  w.nn_back = params->nn_back;
  w.nn_ahead = params->nn_ahead;
  // the A/B switches of the tests and the tools (tools/README.md): the environment is read HERE, once per handle
  for (const char* name : kOptionNames) {
    const char* value = std::getenv(name);
    if (value != nullptr) (void)apply_option(c, name, value);
  }
  *out = c;
  return ACMPC_OK;
}

int acmpc_set_option(acmpc_ctx* c, const char* name, const char* value) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (name == nullptr) return fail(c, ACMPC_EINVAL, "null option name");
  if (!apply_option(c, name, value)) return fail(c, ACMPC_EINVAL, std::string("unknown option or bad value: ") + name);
  // captured graphs hold the launch forms they were captured with
  c->opt_graphs.clear();
  c->tick_graphs.clear();
  return ACMPC_OK;
}

void acmpc_destroy(acmpc_ctx* c) {
  if (c == nullptr) return;
  if (c->touched_device) {  // also after a failed bring-up: whatever was allocated before the failure is freed
    if (c->prm.device >= 0) (void)hipSetDevice(c->prm.device);
    (void)hipFree(c->d_coef);
    (void)hipFree(c->d_start_clock);
    (void)hipFree(c->d_partial_keys);
    (void)hipFree(c->d_partial_feas);
    (void)hipFree(c->d_soft_partial);
    (void)hipFree(c->d_segments);
    (void)hipFree(c->d_uprev);
    (void)hipFree(c->d_astate);
    (void)hipFree(c->d_obs);
    (void)hipFree(c->d_surface);
    (void)hipFree(c->d_road);
    (void)hipFree(c->d_progress);
    (void)hipFree(c->d_identify);
    (void)hipFree(c->d_identify_e);
    (void)hipFree(c->d_plan_trace);
    (void)hipFree(c->d_centre);
    (void)hipFree(c->d_uref);
    (void)hipFree(c->d_U);
    (void)hipFree(c->d_x0);
    (void)hipFree(c->d_costs);
    (void)hipFree(c->d_records);
    (void)hipFree(c->d_keys);
    (void)hipFree(c->d_tickets);
    (void)hipFree(c->d_trace);
    (void)hipFree(c->d_nn_frames);
    if (c->h_keys != nullptr) (void)hipHostFree(c->h_keys);
    if (c->h_io != nullptr) (void)hipHostFree(c->h_io);
    if (c->h_lq != nullptr) (void)hipHostFree(c->h_lq);
    c->opt_graphs.clear();
    c->tick_graphs.clear();
    if (c->h_tick != nullptr) (void)hipHostFree(c->h_tick);
    if (c->h_tick_out != nullptr) (void)hipHostFree(c->h_tick_out);
    (void)hipFree(c->d_tick);
    (void)hipFree(c->d_warm);
    (void)hipFree(c->d_map);
    (void)hipFree(c->d_coords);
    if (c->h_opt != nullptr) (void)hipHostFree(c->h_opt);
    if (c->h_opt_records != nullptr) (void)hipHostFree(c->h_opt_records);
    (void)hipFree(c->d_seed);
    (void)hipFree(c->d_opt);
    if (c->stream != nullptr) (void)hipStreamDestroy(c->stream);
    for (hipEvent_t e : c->prof_start) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->prof_stop) (void)hipEventDestroy(e);
  }
  delete c;
}

int acmpc_set_paths(acmpc_ctx* c, const double* tables, int32_t P, int32_t n) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (tables == nullptr) return fail(c, ACMPC_EINVAL, "null tables");
  if (P < 1 || n < 2) return fail(c, ACMPC_EINVAL, "need P >= 1 and n >= 2");
  if (P > c->prm.max_problems || n > c->prm.max_steps) return fail(c, ACMPC_ECAPACITY, "P or n exceeds capacity");
  const int stride = c->coef_stride;
  c->h_coef.assign(static_cast<size_t>(P) * n * stride, 0.0f);
  const double margin = c->prm.margin;
  for (int p = 0; p < P; ++p) {
    const double* t = tables + static_cast<size_t>(p) * 7 * n;
    const double *x = t, *y = t + n, *psi = t + 2 * n, *kappa = t + 3 * n, *ds = t + 4 * n, *width = t + 5 * n,
                 *v = t + 6 * n;
    float* out = c->h_coef.data() + static_cast<size_t>(p) * n * stride;
    for (int i = 0; i < n; ++i, out += stride) {
      if (c->prm.mode == ACMPC_MODE_SPATIAL) {
        // non-trivial entries of A_i, B_i, f_i (dynamics.py:65-103) and the corridor of x_{i+1} (control.py:57-60)
        const double vds = v[i] * ds[i] + kEps;
        out[0] = static_cast<float>(ds[i]);
        out[1] = static_cast<float>(-(kappa[i] * kappa[i]) * ds[i]);
        out[2] = static_cast<float>(-kappa[i] / vds);
        out[3] = static_cast<float>(-1.0 / (v[i] * v[i] * ds[i] + kEps));
        out[4] = static_cast<float>(1.0 / vds);
        out[5] = static_cast<float>(v[i]);
        out[6] = static_cast<float>(kappa[i]);
        out[7] = static_cast<float>(-width[i] / 2.0 + margin);
        out[8] = static_cast<float>(width[i] / 2.0 - margin);
      } else {
        out[0] = static_cast<float>(x[i]);
        out[1] = static_cast<float>(y[i]);
        out[2] = static_cast<float>(std::cos(psi[i]));
        out[3] = static_cast<float>(std::sin(psi[i]));
        out[4] = static_cast<float>(psi[i]);
        out[5] = static_cast<float>(kappa[i]);
        out[6] = static_cast<float>(v[i]);
        out[7] = static_cast<float>(width[i] / 2.0 - margin);
      }
    }
  }
  if (c->prm.lq_candidate != 0) c->h_tables.assign(tables, tables + static_cast<size_t>(P) * 7 * n);
  c->h_nn_frames.clear();
  if (paths_tabulate_frames(c, n))
    verified_frames(c->h_coef.data(), P, n, &c->h_nn_frames);
  c->P_set = P;
  c->n_set = n;
  derive_progress_table(c);
  c->tables_dirty = true;
  c->frames_dirty = !c->h_nn_frames.empty();
  return ACMPC_OK;
}

int acmpc_set_coefficients(acmpc_ctx* c, const float* coef, int32_t P, int32_t n) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (coef == nullptr) return fail(c, ACMPC_EINVAL, "null coefficients");
  if (P < 1 || n < 2) return fail(c, ACMPC_EINVAL, "need P >= 1 and n >= 2");
  if (P > c->prm.max_problems || n > c->prm.max_steps) return fail(c, ACMPC_ECAPACITY, "P or n exceeds capacity");
  c->h_coef.assign(coef, coef + static_cast<size_t>(P) * n * c->coef_stride);
  if (c->h_tables.size() != static_cast<size_t>(P) * 7 * n) c->h_tables.clear();   // (no float64 tables for these paths)
  c->h_nn_frames.clear();
  if (paths_tabulate_frames(c, n))
    verified_frames(c->h_coef.data(), P, n, &c->h_nn_frames);
  c->P_set = P;
  c->n_set = n;
  derive_progress_table(c);
  c->tables_dirty = true;
  c->frames_dirty = !c->h_nn_frames.empty();
  return ACMPC_OK;
}

int32_t acmpc_search_window(int32_t* back) {
  if (back != nullptr) *back = acmpc::kVerifiedBack;
  return acmpc::kVerifiedWindow;
}

int32_t acmpc_search_frame_floats(int32_t n) {
  return n >= acmpc::kVerifiedWindow ? acmpc::verified_frame_floats(n) : 0;
}

int acmpc_search_frames(const float* coef, int32_t P, int32_t n, float* out, int64_t capacity_floats) {
  if (coef == nullptr || out == nullptr || P < 1 || n < acmpc::kVerifiedWindow) return ACMPC_EINVAL;
  std::vector<float> frames;
  verified_frames(coef, P, n, &frames);
  if (capacity_floats < static_cast<int64_t>(frames.size())) return ACMPC_ECAPACITY;
  std::memcpy(out, frames.data(), frames.size() * sizeof(float));
  return ACMPC_OK;
}

int acmpc_get_coefficients(const acmpc_ctx* c, int32_t problem, float* out, int32_t capacity_floats) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  if (c->P_set == 0) return fail(c, ACMPC_ESTATE, "acmpc_set_paths has not been called");
  if (problem < 0 || problem >= c->P_set) return fail(c, ACMPC_EINVAL, "problem index out of range");
  const size_t count = static_cast<size_t>(c->n_set) * c->coef_stride;
  if (capacity_floats < static_cast<int64_t>(count)) return fail(c, ACMPC_ECAPACITY, "output buffer too small");
  std::memcpy(out, c->h_coef.data() + static_cast<size_t>(problem) * count, count * sizeof(float));
  return ACMPC_OK;
}

int acmpc_get_progress_table(const acmpc_ctx* c, int32_t problem, float* out, int32_t capacity_floats) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_get_progress_table needs a mode D handle");
  if (c->P_set == 0) return fail(c, ACMPC_ESTATE, "acmpc_set_paths has not been called");
  if (problem < 0 || problem >= c->P_set) return fail(c, ACMPC_EINVAL, "problem index out of range");
  const size_t count = static_cast<size_t>(c->n_set);
  if (capacity_floats < static_cast<int64_t>(count)) return fail(c, ACMPC_ECAPACITY, "output buffer too small");
  std::memcpy(out, c->h_progress.data() + static_cast<size_t>(problem) * count, count * sizeof(float));
  return ACMPC_OK;
}

int acmpc_sync_tables(acmpc_ctx* c, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->stream_pending && (c->tables_dirty || c->frames_dirty))   // (the pending finalize reads the tables on the device)
    return fail(c, ACMPC_ESTATE, "a batch of acmpc_solve_stream_device is pending: acmpc_solve_stream_flush first");
  ACMPC_TRY(ensure_device(c));
  hipStream_t s = static_cast<hipStream_t>(stream);
  ACMPC_TRY(upload_tables(c, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  return ACMPC_OK;
}

int acmpc_host_alloc(void** out, uint64_t bytes) {
  if (out == nullptr || bytes == 0) return fail(nullptr, ACMPC_EINVAL, "acmpc_host_alloc: null output or zero size");
  *out = nullptr;
  const hipError_t e = hipHostMalloc(out, static_cast<size_t>(bytes), hipHostMallocDefault);
  if (e != hipSuccess) return fail_hip(nullptr, e, "hipHostMalloc");
  return ACMPC_OK;
}

int acmpc_host_free(void* memory) {
  if (memory == nullptr) return ACMPC_OK;
  const hipError_t e = hipHostFree(memory);
  if (e != hipSuccess) return fail_hip(nullptr, e, "hipHostFree");
  return ACMPC_OK;
}

void acmpc_philox4x32(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  acmpc::philox4x32_10(counter, key, out);
}

}  // extern "C"
