// C ABI, the control tick (include/acmpc.h).  This unit owns the layouts of the tick's pinned and device blocks, the bound
// map and the window cut out of it, acmpc_control_tick as a sequence of steps (validate, argument set-up, header, host plan,
// enqueue, completion, unpacking), and the calls that read back what a tick left on the device.
#include <algorithm>
#include <atomic>
#include <chrono>

#include "acmpc_ctx.h"
#include "acmpc_prologue.h"

using namespace acmpc::capi;

namespace {

size_t align16(size_t v) { return (v + 15) & ~static_cast<size_t>(15); }

// layout of the tick blocks for a horizon of n steps: the pinned host input block (header | coords | centre) and the
// device block the prologue fills for the rollout kernels (seed | x0 | centre | u_ref | table)
struct TickLayout {
  size_t coords, centre_in, host_total;            // pinned host block
  size_t seed, x0, centre, uref, coef, frames, total;   // device block
  explicit TickLayout(int n, int coef_stride = ACMPC_COEF_STRIDE_SPATIAL) {
    coords = align16(sizeof(acmpc::TickHeader));
    centre_in = align16(coords + static_cast<size_t>(n + 1) * 3 * sizeof(double));
    host_total = align16(centre_in + static_cast<size_t>(n) * 2 * sizeof(float));
    seed = 0;
    x0 = 16;
    centre = 32;
    uref = align16(centre + static_cast<size_t>(n) * 2 * sizeof(float));
    coef = align16(uref + static_cast<size_t>(n) * 2 * sizeof(float));
    frames = align16(coef + static_cast<size_t>(n) * coef_stride * sizeof(float));   // (mode T, exhaustive search)
    total = align16(frames + static_cast<size_t>(acmpc::verified_frame_floats(std::max(n, acmpc::kVerifiedWindow))) * sizeof(float));
  }
};

// layout of the pinned result block
struct TickOutLayout {
  size_t record, table, status, coords, done, total;
  explicit TickOutLayout(int n) {
    record = 0;
    table = align16(static_cast<size_t>(acmpc_record_floats(n)) * sizeof(float));
    status = align16(table + static_cast<size_t>(7) * n * sizeof(double));   // QP status, iterations, map index
    coords = status + 16;
    done = align16(coords + static_cast<size_t>(n + 1) * 3 * sizeof(double));   // completion flag of the last round
    total = done + 16;
  }
};

// the bound map -> device (when bound or re-bound since the last upload)
int upload_map(acmpc_ctx* c, hipStream_t s) {
  if (!c->map_dirty) return ACMPC_OK;
  // a captured tick graph has the map's address, length and window size in its kernel arguments: none survives a re-bind
  c->tick_graphs.clear();
  ACMPC_HIP(c, hipStreamSynchronize(s));   // nothing of an earlier tick still reads the old map
  (void)hipFree(c->d_map);
  c->d_map = nullptr;
  ACMPC_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_map), c->h_map.size() * sizeof(double)));
  ACMPC_HIP(c, hipMemcpyAsync(c->d_map, c->h_map.data(), c->h_map.size() * sizeof(double), hipMemcpyHostToDevice, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  c->map_dirty = false;
  return ACMPC_OK;
}

int map_window_args(acmpc_ctx* c, int H, int points, const TickOutLayout& out, acmpc::MapWindowArgs* a) {
  if (c->h_map.empty()) return fail(c, ACMPC_ESTATE, "no map bound (acmpc_bind_map)");
  if (points < H || points % H != 0) return fail(c, ACMPC_EINVAL, "centreline_points must be a multiple of the horizon");
  a->header = reinterpret_cast<const acmpc::TickHeader*>(c->h_tick);
  a->centre = c->d_map;
  a->M = static_cast<int>(c->h_map.size() / 2);
  a->count = static_cast<int>(std::lround(150.0 / c->map_spacing)) + 1;   // BEV look-ahead, perception/tracks.py:14
  if (a->count < 2 || a->count > a->M) return fail(c, ACMPC_EINVAL, "the map is shorter than the 150 m look-ahead window");
  a->points = points;
  a->H = H;
  a->coords = c->d_coords;
  a->coords_out = reinterpret_cast<double*>(c->h_tick_out + out.coords);
  a->first_out = reinterpret_cast<int*>(c->h_tick_out + out.status) + 2;
  return ACMPC_OK;
}

int ensure_tick(acmpc_ctx* c) {
  if (c->tick_ready) return ACMPC_OK;
  c->touched_device = true;
  const int n_cap = std::min(c->prm.max_steps, acmpc::kPrologueMaxSteps);
  ACMPC_HIP(c, host_alloc_once(&c->h_tick, TickLayout(n_cap).host_total));
  ACMPC_HIP(c, alloc_once(&c->d_tick, TickLayout(n_cap).total));
  ACMPC_HIP(c, host_alloc_once(&c->h_tick_out, TickOutLayout(n_cap).total));
  std::memset(c->h_tick_out, 0, TickOutLayout(n_cap).total);   // completion flags start below every sequence number
  ACMPC_HIP(c, alloc_once(&c->d_coords, static_cast<size_t>(n_cap + 1) * 3 * sizeof(double)));
  c->warm_stride = 2 + 3 * n_cap;
  const size_t warm_bytes = static_cast<size_t>(2) * c->warm_stride * sizeof(double);
  ACMPC_HIP(c, alloc_once(&c->d_warm, warm_bytes));
  ACMPC_HIP(c, hipMemset(c->d_warm, 0, warm_bytes));  // valid flags 0: the first tick of each solver starts cold
  ACMPC_HIP(c, hipStreamSynchronize(nullptr));
  c->tick_ready = true;
  return ACMPC_OK;
}

// One acmpc_control_tick on its way through the steps below: the call's inputs, what follows from them and from the
// handle's switches, the two blocks' layouts and the kernels' argument blocks.
struct Tick {
  acmpc_ctx* c;
  const acmpc_tick* t;
  const double* coords;   // the caller's path [H][3], or nullptr: the path is cut out of the bound map on the device
  const float* centre;
  const int H, n, N;
  const bool temporal, from_map, lq_on, use_graph, direct, flagged;
  const TickLayout in;
  const TickOutLayout out;
  acmpc::MapWindowArgs ma{};
  acmpc::PrologueArgs pa{};
  unsigned done_value = 0;   // the completion flag's value for this tick
  // Completion: with direct launches the last round's tail stores a sequence number behind the record, both in pinned
  // host memory, and wait_for_flag polls it - the record is here a microsecond after it was written, where the launch's
  // completion signal (hipStreamSynchronize) takes the driver's path.  The stream is only synchronised when the flag
  // does not come (a fault), and before a host buffer the kernels read is rewritten by a DIFFERENT kind of call.
  Tick(acmpc_ctx* ctx, const acmpc_tick* tick, const double* path, const float* centre_in)
      : c(ctx), t(tick), coords(path), centre(centre_in), H(tick->horizon), n(H - 1), N(tick->n_candidates),
        temporal(ctx->prm.mode == ACMPC_MODE_TEMPORAL), from_map(path == nullptr), lq_on(ctx->prm.lq_candidate != 0),
        use_graph(ctx->sw.tick_graph), direct(use_fused_finalize(ctx, n)),
        flagged(direct && !use_graph && !ctx->sw.tick_no_flag),
        in(n, ctx->coef_stride),   // (spatial rows are the wider: ensure_tick sized the blocks for them)
        out(n) {}
  unsigned* done_flag() const { return reinterpret_cast<unsigned*>(c->h_tick_out + out.done); }
};

int tick_validate(acmpc_ctx* c, const acmpc_tick* t, const double* coords, const float* centre) {
  if (t->struct_size != sizeof(acmpc_tick)) return fail(c, ACMPC_EINVAL, "acmpc_tick size mismatch");
  if (c->stream_pending)
    return fail(c, ACMPC_ESTATE, "a batch of acmpc_solve_stream_device is pending: acmpc_solve_stream_flush first");
  const char* why = nullptr;
  const int rc = tick_check(c, t->horizon, t->rounds, t->n_candidates, &why);
  if (rc != ACMPC_OK) return fail(c, rc, why);
  if (centre == nullptr && t->centre_is_reference == 0) return fail(c, ACMPC_EINVAL, "null centre");
  if (coords == nullptr && c->h_map.empty()) return fail(c, ACMPC_EINVAL, "null coords and no map bound");
  return ACMPC_OK;
}

// the arguments of the window search (a path from the map: the map goes up first) and of the prologue
int tick_arguments(Tick& k, hipStream_t s) {
  acmpc_ctx* c = k.c;
  acmpc::MapWindowArgs& ma = k.ma;
  acmpc::PrologueArgs& pa = k.pa;
  if (k.from_map) {
    ACMPC_TRY(map_window_args(c, k.H, k.t->centreline_points, k.out, &ma));
    ACMPC_TRY(upload_map(c, s));
    ma.centre = c->d_map;
  }
  pa.header = reinterpret_cast<const acmpc::TickHeader*>(c->h_tick);   // read in place over the host link
  pa.coords = reinterpret_cast<const double*>(c->h_tick + k.in.coords);
  if (k.from_map) {
    pa.map_centre = c->d_map;
    pa.map_M = ma.M;
    pa.map_count = ma.count;
    pa.map_points = ma.points;
    pa.map_first = reinterpret_cast<const int*>(c->d_coords);   // (the search kernel leaves the index here)
    pa.coords_out = ma.coords_out;
    pa.index_out = ma.first_out;
    ma.coords = nullptr;                                         // the search launch only needs to leave `first`
    ma.coords_out = nullptr;
    ma.first_out = reinterpret_cast<int*>(c->d_coords);
  }
  pa.temporal = k.temporal ? 1 : 0;
  pa.centre_in = reinterpret_cast<const float*>(c->h_tick + k.in.centre_in);
  pa.x0 = reinterpret_cast<float*>(c->d_tick + k.in.x0);
  pa.u_ref = reinterpret_cast<float*>(c->d_tick + k.in.uref);
  pa.coef = reinterpret_cast<float*>(c->d_tick + k.in.coef);
  pa.frames = tick_tabulates_frames(c, k.n) ? reinterpret_cast<float*>(c->d_tick + k.in.frames) : nullptr;
  pa.centre = reinterpret_cast<float*>(c->d_tick + k.in.centre);
  pa.seed = reinterpret_cast<uint32_t*>(c->d_tick + k.in.seed);
  pa.table_out = reinterpret_cast<double*>(c->h_tick_out + k.out.table);
  pa.status = reinterpret_cast<int*>(c->h_tick_out + k.out.status);
  pa.warm_state = c->d_warm;
  pa.warm_stride = c->warm_stride;
  pa.warm_capacity = (c->warm_stride - 2) / 3;
  pa.margin = c->prm.margin;
  pa.u_lo0 = c->prm.u_min[0];
  pa.u_lo1 = c->prm.u_min[1];
  pa.u_hi0 = c->prm.u_max[0];
  pa.u_hi1 = c->prm.u_max[1];
  return ACMPC_OK;
}

// this tick's header, path and centre into the pinned input block
void fill_header(const Tick& k) {
  const acmpc_tick* t = k.t;
  acmpc::TickHeader* h = reinterpret_cast<acmpc::TickHeader*>(k.c->h_tick);
  h->offset = t->offset;
  h->v_min = t->v_min;
  h->v_max = t->v_max;
  h->a_min = t->a_min;
  h->a_max = t->a_max;
  h->ay_max = t->ay_max;
  h->ki_min = t->ki_min;
  h->end_velocity = t->end_velocity;
  h->qp_eps_abs = t->qp_eps_abs;
  h->qp_eps_rel = t->qp_eps_rel;
  h->eps = kEps;
  h->horizon = k.H;
  h->localised = t->localised;
  h->has_end_velocity = t->has_end_velocity;
  h->centre_is_reference = t->centre_is_reference;
  h->qp_max_iter = t->qp_max_iter;
  h->qp_check_every = t->qp_check_every;
  h->qp_method = t->qp_method;
  h->seed_lo = static_cast<uint32_t>(t->seed);
  h->seed_hi = static_cast<uint32_t>(t->seed >> 32);
  h->use_map = k.from_map ? 1 : 0;
  h->map_index = t->map_index;
  h->pose_x = t->pose_x;
  h->pose_y = t->pose_y;
  h->lateral_offset = t->lateral_offset;
  if (!k.from_map) std::memcpy(k.c->h_tick + k.in.coords, k.coords, static_cast<size_t>(k.H) * 3 * sizeof(double));
  if (k.centre != nullptr) std::memcpy(k.c->h_tick + k.in.centre_in, k.centre, static_cast<size_t>(k.n) * 2 * sizeof(float));
}

// The LQ plan (acmpc_params::lq_candidate), computed on the host while this tick's prologue and earlier rounds run and
// read by the last round in place from pinned memory.  The tick's own table is being built on the device right now; what
// the host has is this tick's PATH - so the plan is for the waypoints of `coords` (acmpc_waypoint_table, the host
// statement of the prologue's first step) with the speed profile the previous tick solved (the QP is warm-started from
// it and moves little from tick to tick) and the start state of this tick's pose (offset, 0, pi / 2).  With the path cut
// out of the map on the device (coords = NULL) the host does not have it: the plan is then the previous tick's problem's.
// There the host cuts the same window itself (round 5) when it knows where it starts - `map_index` given, the window's
// `M`, `count` and `points` as the device takes them; for a pose, whose nearest map point the device searches, the plan
// stays the previous tick's problem's: a scan of the map on the host would outlast the rounds it has to hide behind.
bool plan_previous(acmpc_ctx* c, const acmpc_tick* t, const double* coords, int H, const acmpc::MapWindowArgs& window) {
  const int n = H - 1;
  if (coords == nullptr && t->map_index >= 0) {   // (here, not in front of the launches: this runs while the prologue and the first round do)
    c->tick_host_coords.resize(static_cast<size_t>(H) * 3);
    const int first = ((t->map_index % window.M) + window.M) % window.M;
    const acmpc::MapFrame frame = acmpc::map_frame(c->h_map.data(), window.M, first);
    for (int r = 0; r < H; ++r) {
      double row[3];
      acmpc::map_path_row(c->h_map.data(), window.M, first, window.count, window.points, H, r, t->lateral_offset, frame, row);
      for (int e = 0; e < 3; ++e) c->tick_host_coords[static_cast<size_t>(3) * r + e] = row[e];
    }
    coords = c->tick_host_coords.data();
  }
  // The speed profile the plan is made with.  With the path on the host and the exact profile (qp_method 0) it is THIS
  // tick's - the host statement of the prologue's own two passes (acmpc_velocity_ceiling + acmpc_speed_profile_exact, a
  // microsecond) - on the host's waypoint table; where that does not apply (an infeasible profile; qp_method 1: the
  // splitting is not run twice per tick) the previous tick's, and with no previous tick either (a handle's first, another
  // horizon, a tick without a finite plan) the splitting, cold, once.
  const bool have_previous = c->tick_prev_n == n;
  if (!have_previous && coords == nullptr) return false;   // (no path on the host: nothing to plan for)
  if (coords == nullptr) return lq_plan_into(c, c->tick_prev_table.data(), n, c->tick_prev_x0, c->h_lq);
  c->tick_lq_table.resize(static_cast<size_t>(7) * n);
  if (acmpc_waypoint_table(coords, H, kEps, c->tick_lq_table.data()) != ACMPC_OK) return false;
  {
    c->tick_lq_scratch.resize(static_cast<size_t>(3) * n);
    double* ceiling = c->tick_lq_scratch.data();
    double* dual = ceiling + n;
    double* profile = c->tick_lq_table.data() + static_cast<size_t>(6) * n;
    const double* spacing = c->tick_lq_table.data() + static_cast<size_t>(4) * n;
    int32_t iterations = 0;
    if (acmpc_velocity_ceiling(c->tick_lq_table.data() + static_cast<size_t>(3) * n, n, t->ay_max, t->ki_min, t->v_min,
                               t->v_max, t->localised, t->has_end_velocity, t->end_velocity, ceiling) != ACMPC_OK)
      return false;
    const bool swept = t->qp_method == 0 &&
                       acmpc_speed_profile_exact(ceiling, spacing, n, t->a_min, t->a_max, t->v_min, profile, dual) == 0;
    if (!swept) {
      if (have_previous) {
        std::memcpy(profile, c->tick_prev_table.data() + static_cast<size_t>(6) * n, static_cast<size_t>(n) * sizeof(double));
      } else if (acmpc_speed_profile_qp(ceiling, spacing, n, t->a_min, t->a_max, t->v_min, t->qp_max_iter, t->qp_check_every,
                                        t->qp_eps_abs, t->qp_eps_rel, profile, dual, 0, &iterations) != 0) {
        return false;
      }
    }
  }
  const double pose[3] = {t->offset, 0.0, M_PI / 2.0};
  return lq_plan_into(c, c->tick_lq_table.data(), n, pose, c->h_lq, true);
}

// prologue -> rounds (-> copy of the record when the fused finalize cannot write it to the host itself), on `q` directly
// or while it is being captured.  Launched directly the host plans inside, right before the last round is enqueued; a
// captured graph is planned for before every replay (plan_for_replay).
hipError_t tick_enqueue(const Tick& k, hipStream_t q, int* rc_rounds) {
  acmpc_ctx* c = k.c;
  const acmpc_tick* t = k.t;
  // (a pose instead of a map index: the nearest-point search runs in front, as its own 256-thread launch)
  hipError_t e = (k.from_map && t->map_index < 0) ? acmpc::launch_map_window(k.ma, q) : hipSuccess;
  if (e == hipSuccess) e = acmpc::launch_prologue(k.pa, k.n, q);
  if (e != hipSuccess) return e;
  OptInputs oi{k.pa.x0, k.pa.centre, k.pa.u_ref, k.pa.coef, k.pa.frames};
  if (k.lq_on) {
    oi.extra = c->h_lq;
    if (!k.use_graph) oi.before_last = [&k] { return plan_previous(k.c, k.t, k.coords, k.H, k.ma); };
  }
  // (launched directly the rounds take the seed by value: read from the device block, as a replayed graph must, it is
  // a dependent load in front of every round's first Philox draw)
  *rc_rounds = enqueue_rounds(c, oi, 1, k.N, k.n, t->rounds, t->sigma[0], t->sigma[1], t->shrink,
                              k.use_graph ? 0 : t->seed, k.use_graph ? k.pa.seed : nullptr, q, true,
                              k.direct ? reinterpret_cast<float*>(c->h_tick_out + k.out.record) : nullptr,
                              k.flagged ? k.done_flag() : nullptr, k.done_value);
  if (*rc_rounds == ACMPC_OK && !k.direct)
    e = hipMemcpyAsync(c->h_tick_out + k.out.record, c->d_records,
                       static_cast<size_t>(acmpc_record_floats(k.n)) * sizeof(float), hipMemcpyDeviceToHost, q);
  return e;
}

// ACMPC_TICK_GRAPH=1: the captured graph of this tick's key, captured now when the cache does not hold it
int tick_graph(const Tick& k, hipStream_t s, hipGraphExec_t* graph) {
  const acmpc_tick* t = k.t;
  TickKey key;
  key.N = k.N;
  key.n = k.n;
  key.rounds = t->rounds;
  key.sigma_v = t->sigma[0];
  key.sigma_k = t->sigma[1];
  key.shrink = t->shrink;
  key.from_map = k.from_map ? (t->map_index < 0 ? -t->centreline_points : t->centreline_points) : 0;
  int slot = k.c->tick_graphs.find(key);
  if (slot < 0)
    ACMPC_TRY(k.c->tick_graphs.capture(k.c, s, key, "capturing the tick graph",
                                       [&k](hipStream_t q, int* rc_rounds) { return tick_enqueue(k, q, rc_rounds); }, &slot));
  *graph = k.c->tick_graphs.use(slot);
  return ACMPC_OK;
}

// the host plan in front of a replay.  Without one the replayed graph's candidate 2, which always reads h_lq, gets the
// centre sequence instead (candidate 0 again) or, without one, zeros - the sampler clips them into the input box like
// every candidate, so the slot holds a DEFINED sequence (never the stale plan of another path) that the argmin will not keep
void plan_for_replay(const Tick& k) {
  if (!k.lq_on || plan_previous(k.c, k.t, k.coords, k.H, k.ma)) return;
  if (k.centre != nullptr && k.t->centre_is_reference == 0)
    std::memcpy(k.c->h_lq, k.centre, static_cast<size_t>(k.n) * 2 * sizeof(float));
  else
    std::memset(k.c->h_lq, 0, static_cast<size_t>(k.n) * 2 * sizeof(float));
}

// Three short kernels behind one another: launched directly they start sooner than a graph replay does (the
// replay's fixed cost is ~10 us on this runtime, a launch on an idle stream ~4 us, and the later launches overlap
// the prologue's execution).  The header, and a short path with its centre, travel in the prologue's arguments.
int tick_launch(Tick& k, hipStream_t s) {
  acmpc_ctx* c = k.c;
  k.pa.header_by_value = 1;
  k.pa.header_value = *reinterpret_cast<const acmpc::TickHeader*>(c->h_tick);
  if (!k.from_map && k.H <= acmpc::kInlinePathPoints && !c->sw.tick_no_inline_path) {
    k.pa.path_by_value = 1;
    std::memcpy(k.pa.coords_value, k.coords, static_cast<size_t>(k.H) * 3 * sizeof(double));
    if (k.centre != nullptr) std::memcpy(k.pa.centre_value, k.centre, static_cast<size_t>(k.n) * 2 * sizeof(float));
  }
  int rc_rounds = ACMPC_OK;
  const hipError_t e = tick_enqueue(k, s, &rc_rounds);
  if (rc_rounds != ACMPC_OK || e != hipSuccess) {
    // part of the sequence may be running: it reads the pinned input block and writes the result block, which the
    // caller's next tick would overwrite - wait for it (result ignored in favour of the error that brought us here)
    (void)hipStreamSynchronize(s);
    if (rc_rounds != ACMPC_OK) return rc_rounds;
    ACMPC_HIP(c, e);
  }
  return ACMPC_OK;
}

// the completion flag of the last round's tail, polled in pinned memory
int wait_for_flag(const Tick& k, hipStream_t s) {
  volatile unsigned* flag = k.done_flag();
  const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(200);
  unsigned spins = 0;
  while (*flag != k.done_value) {
    __builtin_ia32_pause();
    if ((++spins & 0x3fffu) == 0 && std::chrono::steady_clock::now() > give_up) break;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  if (*flag != k.done_value) {   // no flag: wait the ordinary way, which also reports what went wrong
    ACMPC_HIP(k.c, hipStreamSynchronize(s));
    if (*flag != k.done_value) return fail(k.c, ACMPC_EHIP, "the tick finished without its completion flag");
  }
  return ACMPC_OK;
}

// the result block into the caller's arrays, and what the next tick's host plan starts from
int unpack_result(const Tick& k, double* table, float* record, double* decision, double* projected_control, double* prediction,
                  double* cum_time, double* times, double* accelerations, double* steer_rates, double* info, double* coords_out) {
  acmpc_ctx* c = k.c;
  const int n = k.n;
  const float* rec = reinterpret_cast<const float*>(c->h_tick_out + k.out.record);
  std::memcpy(record, rec, static_cast<size_t>(acmpc_record_floats(n)) * sizeof(float));
  std::memcpy(table, c->h_tick_out + k.out.table, static_cast<size_t>(7) * n * sizeof(double));
  const int* status = reinterpret_cast<const int*>(c->h_tick_out + k.out.status);
  // dec.x = [x_0 .. x_n ; u_0 .. u_{n-1}] (control.py:121-158) from the record's [u ; x] blocks
  const float* ru = rec + ACMPC_REC_HEADER;
  const float* rx = ru + 2 * n;
  double biggest = 0.0;
  bool finite = std::isfinite(rec[ACMPC_REC_COST]) && std::isfinite(rec[ACMPC_REC_VIOLATION]);
  for (int i = 0; i < 3 * (n + 1); ++i) {
    decision[i] = static_cast<double>(rx[i]);
    biggest = std::max(biggest, std::fabs(decision[i]));
    finite = finite && std::isfinite(rx[i]);
  }
  for (int i = 0; i < 2 * n; ++i) {
    decision[3 * (n + 1) + i] = static_cast<double>(ru[i]);
    biggest = std::max(biggest, std::fabs(static_cast<double>(ru[i])));
    finite = finite && std::isfinite(ru[i]);
  }
  const int rc = k.temporal ? acmpc_unpack_decision_temporal(decision, n, c->prm.dt, c->prm.wheelbase, projected_control,
                                                             prediction, cum_time, times, accelerations, steer_rates)
                            : acmpc_unpack_decision(decision, n, table, c->prm.wheelbase, projected_control, prediction, cum_time,
                                                    times, accelerations, steer_rates);
  if (rc != ACMPC_OK) return fail(c, rc, "acmpc_unpack_decision");
  info[0] = rec[ACMPC_REC_COST];
  info[1] = rec[ACMPC_REC_VIOLATION];
  info[2] = rec[ACMPC_REC_NFEASIBLE];
  info[3] = biggest;
  info[4] = status[0];
  info[5] = status[1];
  info[6] = k.from_map ? static_cast<double>(status[2]) : -1.0;   // first map index of the window
  info[7] = finite ? 0.0 : 1.0;   // a non-finite cost, violation or plan entry (max |dec.x| above skips NaNs)
  if (k.lq_on) {   // what the next tick plans for: this tick's table and start state (the record's x_0: Frenet state or pose)
    c->tick_prev_n = (finite && status[0] == 0) ? n : 0;
    if (c->tick_prev_n != 0) {
      c->tick_prev_table.assign(table, table + static_cast<size_t>(7) * n);
      for (int q = 0; q < 3; ++q) c->tick_prev_x0[q] = static_cast<double>(rx[q]);
    }
  }
  if (coords_out != nullptr)
    std::memcpy(coords_out, k.from_map ? reinterpret_cast<const void*>(c->h_tick_out + k.out.coords)
                                       : reinterpret_cast<const void*>(k.coords),
                static_cast<size_t>(k.H) * 3 * sizeof(double));
  return ACMPC_OK;
}

}  // namespace

namespace acmpc {
namespace capi __attribute__((visibility("hidden"))) {

int tick_check(const acmpc_ctx* c, int H, int rounds, int N, const char** why) {
  auto no = [why](int code, const char* text) { *why = text; return code; };
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) return no(ACMPC_ESTATE, "mode D has no control tick: use acmpc_set_paths + acmpc_optimize");
  if (c->prm.centre_update != 0) return no(ACMPC_ESTATE, "acmpc_control_tick needs a handle with centre_update = 0");
  if (c->prm.mode == ACMPC_MODE_TEMPORAL && !(c->prm.dt > 0.0)) return no(ACMPC_ESTATE, "mode T needs a positive dt");
  const int n = H - 1;
  if (H < 3 || rounds < 1 || N < 1) return no(ACMPC_EINVAL, "need horizon >= 3, rounds >= 1, n_candidates >= 1");
  if (n > c->prm.max_steps || N > c->prm.max_candidates) return no(ACMPC_ECAPACITY, "horizon or candidates exceed capacity");
  if (n > acmpc::kPrologueMaxSteps) return no(ACMPC_ESTATE, "the device prologue holds at most 128 steps");
  if (!acmpc::fused_finalize_fits(c->prm.mode, n)) return no(ACMPC_ESTATE, "fused finalize does not fit");
  return ACMPC_OK;
}

// the frames of the verified search: tabulated (by the prologue's second workgroup) only when the rounds can take them -
// beyond 106 steps they no longer fit the three-wave round's LDS and the search wave scans every waypoint
bool tick_tabulates_frames(const acmpc_ctx* c, int n) {
  return c->prm.mode == ACMPC_MODE_TEMPORAL && c->prm.nn_ahead < 0 && n >= acmpc::kVerifiedWindow && acmpc::trio_frames_fit(n) &&
         !c->opt.no_trio_rounds && !c->sw.no_verified_search;
}

}  // namespace capi
}  // namespace acmpc

extern "C" {

int acmpc_control_tick(acmpc_ctx* c, const acmpc_tick* t, const double* coords, const float* centre, double* table,
                       float* record, double* decision, double* projected_control, double* prediction,
                       double* cum_time, double* times, double* accelerations, double* steer_rates, double* info,
                       double* coords_out) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (t == nullptr || table == nullptr || record == nullptr || decision == nullptr ||
      projected_control == nullptr || prediction == nullptr || cum_time == nullptr || times == nullptr ||
      accelerations == nullptr || steer_rates == nullptr || info == nullptr)
    return fail(c, ACMPC_EINVAL, "null argument");
  ACMPC_TRY(tick_validate(c, t, coords, centre));
  ACMPC_TRY(ensure_device(c));
  ACMPC_TRY(ensure_staging(c));
  ACMPC_TRY(ensure_tick(c));
  hipStream_t s = c->stream;
  Tick k(c, t, coords, centre);
  ACMPC_TRY(tick_arguments(k, s));
  k.done_value = ++c->tick_sequence;   // (before any capture: a tick that fails there has still used its value)
  hipGraphExec_t graph = nullptr;
  // ACMPC_TICK_GRAPH=1 replays a captured graph instead of launching directly (tick_launch has why that is not the default)
  ACMPC_TRY(k.use_graph ? tick_graph(k, s, &graph) : upload_segments(c, k.n, s));  // (a no-op once the table for this n is resident)
  fill_header(k);
  if (k.use_graph) {
    plan_for_replay(k);
    ACMPC_HIP(c, hipGraphLaunch(graph, s));
  } else {
    ACMPC_TRY(tick_launch(k, s));
  }
  if (k.flagged) {
    ACMPC_TRY(wait_for_flag(k, s));
  } else {
    ACMPC_HIP(c, hipStreamSynchronize(s));
  }
  c->tick_last_n = k.n;
  return unpack_result(k, table, record, decision, projected_control, prediction, cum_time, times, accelerations, steer_rates,
                       info, coords_out);
}

int acmpc_bind_map(acmpc_ctx* c, const double* centre, int32_t M, double spacing) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (centre == nullptr || M < 3 || !(spacing > 0.0)) return fail(c, ACMPC_EINVAL, "need a centre line of >= 3 points and a positive spacing");
  c->h_map.assign(centre, centre + 2 * static_cast<size_t>(M));
  c->map_spacing = spacing;
  c->map_dirty = true;
  return ACMPC_OK;
}

int acmpc_map_reference_path(acmpc_ctx* c, int32_t map_index, double pose_x, double pose_y, double lateral_offset,
                             int32_t horizon, int32_t centreline_points, double* coords, int32_t* first_index) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (coords == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  const int n = horizon - 1;
  if (horizon < 3 || n > std::min(c->prm.max_steps, acmpc::kPrologueMaxSteps))
    return fail(c, ACMPC_ECAPACITY, "horizon out of range for this handle");
  ACMPC_TRY(ensure_device(c));
  ACMPC_TRY(ensure_staging(c));
  ACMPC_TRY(ensure_tick(c));
  hipStream_t s = c->stream;
  const TickOutLayout out(n);
  acmpc::MapWindowArgs ma{};
  ACMPC_TRY(map_window_args(c, horizon, centreline_points, out, &ma));
  ACMPC_TRY(upload_map(c, s));
  ma.centre = c->d_map;
  acmpc::TickHeader* h = reinterpret_cast<acmpc::TickHeader*>(c->h_tick);
  h->use_map = 1;
  h->map_index = map_index;
  h->pose_x = pose_x;
  h->pose_y = pose_y;
  h->lateral_offset = lateral_offset;
  ACMPC_HIP(c, acmpc::launch_map_window(ma, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  std::memcpy(coords, c->h_tick_out + out.coords, static_cast<size_t>(horizon) * 3 * sizeof(double));
  if (first_index != nullptr) *first_index = reinterpret_cast<const int*>(c->h_tick_out + out.status)[2];
  return ACMPC_OK;
}

int acmpc_tick_read_device_tables(acmpc_ctx* c, float* x0, float* u_ref, float* coef) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (x0 == nullptr || u_ref == nullptr || coef == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  if (!c->tick_ready || c->tick_last_n == 0) return fail(c, ACMPC_ESTATE, "acmpc_control_tick has not run");
  const int n = c->tick_last_n;
  const TickLayout in(n, c->coef_stride);
  ACMPC_HIP(c, hipMemcpy(x0, c->d_tick + in.x0, 3 * sizeof(float), hipMemcpyDeviceToHost));
  ACMPC_HIP(c, hipMemcpy(u_ref, c->d_tick + in.uref, static_cast<size_t>(n) * 2 * sizeof(float), hipMemcpyDeviceToHost));
  ACMPC_HIP(c, hipMemcpy(coef, c->d_tick + in.coef, static_cast<size_t>(n) * c->coef_stride * sizeof(float),
                         hipMemcpyDeviceToHost));
  return ACMPC_OK;
}

int acmpc_tick_read_device_frames(acmpc_ctx* c, float* out, int64_t capacity_floats) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  if (!c->tick_ready || c->tick_last_n == 0) return fail(c, ACMPC_ESTATE, "acmpc_control_tick has not run");
  const int n = c->tick_last_n;
  if (!tick_tabulates_frames(c, n))
    return fail(c, ACMPC_ESTATE, "the last tick tabulated no frames (mode T with the exhaustive search, window <= n <= 106 steps)");
  const int floats = acmpc::verified_frame_floats(n);
  if (capacity_floats < floats) return fail(c, ACMPC_ECAPACITY, "output buffer too small");
  const TickLayout in(n, c->coef_stride);
  ACMPC_HIP(c, hipMemcpy(out, c->d_tick + in.frames, static_cast<size_t>(floats) * sizeof(float), hipMemcpyDeviceToHost));
  return ACMPC_OK;
}

int acmpc_speed_profile_qp_device(acmpc_ctx* c, const double* v_hi, const double* ds, int32_t n, double a_min,
                                  double a_max, double v_min, int32_t max_iter, int32_t check_every, double eps_abs,
                                  double eps_rel, double* v, double* y, int32_t warm_start, int32_t* iterations) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (v_hi == nullptr || ds == nullptr || v == nullptr || y == nullptr || n < 2) return fail(c, ACMPC_EINVAL, "bad argument");
  if (n > acmpc::kPrologueMaxSteps) return fail(c, ACMPC_ECAPACITY, "the device solver holds at most 128 points");
  ACMPC_TRY(ensure_device(c));
  double* d = nullptr;  // v_hi | ds | v | y | status
  const size_t doubles = static_cast<size_t>(5) * n + 2;
  ACMPC_HIP(c, hipMalloc(reinterpret_cast<void**>(&d), doubles * sizeof(double)));
  double *d_vhi = d, *d_ds = d + n, *d_v = d + 2 * n, *d_y = d + 3 * n;
  int* d_out = reinterpret_cast<int*>(d + 5 * n);
  hipError_t e = hipMemcpy(d_vhi, v_hi, static_cast<size_t>(n) * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_ds, ds, static_cast<size_t>(n) * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_v, v, static_cast<size_t>(n) * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_y, y, static_cast<size_t>(2 * n - 1) * sizeof(double), hipMemcpyHostToDevice);
  const acmpc::admm::Settings st{a_min, a_max, v_min, max_iter, check_every > 0 ? check_every : 10, eps_abs, eps_rel};
  if (e == hipSuccess) e = acmpc::launch_admm(d_vhi, d_ds, n, st, d_v, d_y, warm_start, d_out, nullptr);
  int out[2] = {1, 0};
  if (e == hipSuccess) e = hipMemcpy(v, d_v, static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(y, d_y, static_cast<size_t>(2 * n - 1) * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail_hip(c, e, "acmpc_speed_profile_qp_device");
  if (iterations != nullptr) *iterations = out[1];
  return out[0];
}

}  // extern "C"
