// C ABI, acmpc_optimize (include/acmpc.h).  This unit owns the launch sequence of one sampling optimisation
// (enqueue_rounds, which acmpc_control_tick shares), the LQ plan that competes in its last round, the entry point with its
// eager and its captured-graph path, and mode D's form of it.
#include <algorithm>

#include "acmpc_ctx.h"
#include "acmpc_lq.h"

using namespace acmpc::capi;

namespace acmpc {
namespace capi __attribute__((visibility("hidden"))) {

// the handle's own frames (acmpc_set_paths), for the rounds that read the handle's own table
static const float* own_frames(const acmpc_ctx* c) { return c->h_nn_frames.empty() ? nullptr : c->d_nn_frames; }

bool use_fused_finalize(const acmpc_ctx* c, int n) {
  return !c->sw.no_fused_finalize && acmpc::fused_finalize_fits(c->prm.mode, n);
}

// How the fused rounds of a (P, N, n) optimisation run: THE place where that is decided - enqueue_rounds takes it from
// here, and so does acmpc_describe_rounds.
// Traced: the fused finalize copies the record out of the winning workgroup's trace when the launch is small enough for
// the trace buffer (closed-loop rounds are: 256 workgroups) and the trace fits the LDS; else it re-draws and re-rolls.
// Chained: a traced round that is not the last ends without a finalize and the next launch finds its winner itself,
// while a problem has no more workgroups than a wave's lanes hold keys for.
RoundPlan plan_rounds(const acmpc_ctx* c, int P, int N, int n) {
  const int blocks = (N + 63) / 64;
  RoundPlan plan{};
  plan.fused_finalize = use_fused_finalize(c, n);
  plan.traced = plan.fused_finalize && !c->sw.no_traced_finalize && acmpc::traced_finalize_fits(c->prm.mode, n) &&
                static_cast<long long>(P) * blocks <= kTraceBlocks;
  plan.chained = plan.traced && blocks <= acmpc::kChainBlocks && !c->sw.no_chained_rounds;
  return plan;
}

// One LQ plan (csrc/acmpc_lq.h) into `out` [n][2]: the path's 7 x n float64 table, the start state as the rollouts take it
// (mode S: the Frenet state; mode T: the pose, moved into the Frenet frame of the first waypoint here).  Without a finite
// plan (a singular step, a speed profile that was never solved) `out` gets the reference controls clipped into the box -
// candidate 1 again, harmless - and false comes back.
// With lq_candidate = 2 the plan is then refined against the QP's box rows (csrc/acmpc_lq_box.h; the iterate of problem
// `problem` is kept in the handle between calls).
bool lq_plan_into(acmpc_ctx* c, const double* table, int n, const double start[3], float* out, bool start_is_pose, int problem) {
  double x0[3] = {start[0], start[1], start[2]};
  if (start_is_pose || c->prm.mode == ACMPC_MODE_TEMPORAL) acmpc::lq::frenet_start(table, n, start, x0);
  const float lo[2] = {c->w.ulo0, c->w.ulo1}, hi[2] = {c->w.uhi0, c->w.uhi1};
  const bool finite_start = std::isfinite(x0[0]) && std::isfinite(x0[1]) && std::isfinite(x0[2]);
  if (finite_start && acmpc::lq::plan(table, n, x0, c->prm.step_cost, c->prm.r_term, c->prm.final_cost, lo, hi, out)) {
    if (c->prm.lq_candidate == 2) {
      if (c->lq_box_state.size() <= static_cast<size_t>(problem)) c->lq_box_state.resize(static_cast<size_t>(problem) + 1);
      c->lq_box_last = acmpc::lqbox::refine(table, n, x0, c->prm.step_cost, c->prm.r_term, c->prm.final_cost, lo, hi,
                                            c->prm.margin, c->prm.w_bound, c->lq_box_iterations,
                                            c->lq_box_state[static_cast<size_t>(problem)], c->lq_box_ws, out);
    }
    return true;
  }
  if (c->prm.lq_candidate == 2 && c->lq_box_state.size() > static_cast<size_t>(problem))
    c->lq_box_state[static_cast<size_t>(problem)].reset();
  const double *kappa = table + 3 * static_cast<size_t>(n), *vel = table + 6 * static_cast<size_t>(n);
  for (int i = 0; i < n; ++i) {
    out[2 * i] = std::fmin(std::fmax(static_cast<float>(vel[i]), lo[0]), hi[0]);
    out[2 * i + 1] = std::fmin(std::fmax(static_cast<float>(kappa[i]), lo[1]), hi[1]);
  }
  return false;
}

// `final_records`: where the LAST round's records go when the fused finalize writes them (device memory, or pinned
// host memory - then the winner lands in the caller's staging buffer without a copy node); nullptr = c->d_records
int enqueue_rounds(acmpc_ctx* c, const OptInputs& in, int P, int N, int n, int rounds, double sigma_v, double sigma_k,
                   double shrink, uint64_t seed, const uint32_t* d_seed, hipStream_t s, bool fused, float* final_records,
                   unsigned* done, unsigned done_value) {
  const bool has_uref = in.uref != nullptr;
  const RoundPlan plan = plan_rounds(c, P, N, n);
  const bool fused_finalize = plan.fused_finalize;
  const int layout = ACMPC_LAYOUT_STEP_MAJOR;
  const int rec_floats = acmpc_record_floats(n);
  double scale = 1.0;
  for (int r = 0; r < rounds; ++r, scale *= shrink) {
    // round 0 samples round the caller's centre, later rounds round the incumbent = the u block of the records
    const float* d_c = (r == 0) ? in.centre : c->d_records + ACMPC_REC_HEADER;
    const int stride = (r == 0) ? 2 * n : rec_floats;
    const float* d_ref = has_uref ? in.uref : nullptr;
    const float* d_extra = nullptr;   // the LQ plan competes in the last round only
    if (r + 1 == rounds && in.extra != nullptr && (!in.before_last || in.before_last())) d_extra = in.extra;
    if (!fused) {  // (only with the handle's own buffers: in.centre == c->d_centre, in.uref == c->d_uref, in.coef == c->d_coef)
      RoundCentre from;
      ACMPC_TRY(round_centre(c, r, has_uref, P, n, s, &from));
      ACMPC_TRY(matrix_round(c, in.x0, from, d_extra, d_seed, P, N, n, r, rounds, sigma_v * scale, sigma_k * scale, seed, s));
      continue;
    }
    ACMPC_TRY(upload_segments(c, n, s));
    // Traced rounds are chained: a round that is not the last ends without a finalize - its workgroups leave their
    // partial keys and the trace of their best candidate - and the NEXT launch finds the winner itself (argmin over
    // those keys while its Philox draws run) and samples round that workgroup's trace.  Only the last round pays the
    // last-workgroup tail (six dependent device-scope round trips, ~10 us).  Keys, counts and traces alternate between
    // two sets, since a round reads its predecessor's while it writes its own.
    const int blocks = (N + 63) / 64;
    const bool traced = plan.traced, chain = plan.chained;
    const size_t set = (chain && (r & 1)) ? 1 : 0;
    const size_t trace_set_floats = static_cast<size_t>(kTraceBlocks) * acmpc::trace_floats(c->prm.max_steps);
    float* d_trace = c->d_trace + set * trace_set_floats;
    acmpc::RolloutArgs ra = rollout_args(c, in.x0, nullptr, nullptr, P, N, n, 0, set);
    ra.coef = in.coef;
    ra.nn_frames = !c->sw.no_verified_search ? in.frames : nullptr;
    acmpc::SampleArgs sa{};
    sa.centre = d_c;
    sa.centre_stride = stride;
    sa.u_ref = d_ref;
    sa.u_extra = d_extra;
    sa.P = P;
    sa.N = N;
    sa.n = n;
    sa.spec = make_spec(c, sigma_v * scale, sigma_k * scale, seed, static_cast<uint32_t>(r));
    sa.spec.seed_ptr = d_seed;
    if (chain && r > 0) {
      sa.prev_keys = c->d_partial_keys + (set ^ 1) * c->partial_slots;
      sa.prev_trace = c->d_trace + (set ^ 1) * trace_set_floats;
      sa.prev_blocks = blocks;
      sa.prev_pitch = acmpc::trace_floats(n);
    }
    // NB: the finalize of round r reads its centre from the records it is about to overwrite; it copies the
    // controls it needs into registers/LDS before lane 0..63 write the new record, and one wave owns one record
    // (timing armed - acmpc_profile_enable, eager path only: every round's launch carries an event pair)
    hipEvent_t e0, e1;
    next_event_pair(c, &e0, &e1);
    if (fused_finalize) {
      // one launch per round: the last workgroup of each problem also reduces the partial keys and writes the
      // record; rounds before the last only need the winner's controls (the next centre), not its re-roll
      const bool last = r + 1 == rounds;
      const bool tail = last || !chain;
      const acmpc::FusedFinalize ff{tail ? c->d_tickets : nullptr,
                                    (last && final_records != nullptr) ? final_records : c->d_records, !last,
                                    traced ? d_trace : nullptr, acmpc::trace_floats(n),
                                    last ? done : nullptr, done_value};
      ACMPC_HIP(c, acmpc::launch_rollout_sampled(c->prm.mode, ra, sa, ff, s, e0, e1, c->opt));
    } else {
      ACMPC_HIP(c, acmpc::launch_rollout_sampled(c->prm.mode, ra, sa, acmpc::FusedFinalize{nullptr, nullptr, false, nullptr, 0, nullptr, 0}, s, e0, e1, c->opt));
      Regenerate regen{d_c, stride, d_ref, sa.spec, d_extra};
      ACMPC_TRY(finalize(c, nullptr, nullptr, in.x0, nullptr, P, N, n, layout, 0, c->d_records, (N + 63) / 64, s, &regen,
                         in.coef));
    }
  }
  return ACMPC_OK;
}

// acmpc_optimize in mode D: per round the rollout that draws its own candidates and the finalize that re-draws the winner
// from its index - two launches, no control matrix; round r samples round the u block of round r - 1's record, with the
// spread sigma shrink^r (acmpc_optimize's own schedule).  ACMPC_DYNAMIC_MATRIX_ROUNDS keeps sample -> rollout -> finalize
// through the matrix (three launches): the same records bit for bit.
// centre_update = 1 (softmin): the round protocol of modes S and T (enqueue_rounds) - after every round but the last the
// softmin mean of its candidates goes into d_centre and is the next round's centre (candidate 0), the winner's u block is
// staged into d_uref as the next round's candidate 1.  The rollout then leaves its costs, the finalize its keys, and the
// sampled softmin (launch_softmin_sampled) re-draws the candidates a third time: still no matrix.  With the matrix rounds the
// mean is launch_softmin's over the matrix - the same bits.
static int optimize_dynamic(acmpc_ctx* c, const float* x0, const float* centre, const float* u_ref, int P, int N, int n,
                            int rounds, const double sigma[2], double shrink, uint64_t seed, float* records) {
  hipStream_t s = c->stream;
  const size_t path_bytes = static_cast<size_t>(P) * n * 2 * sizeof(float);
  const int layout = ACMPC_LAYOUT_STEP_MAJOR;
  const int rec_floats = acmpc_record_floats(n);
  const bool softmin = c->prm.centre_update == 1;
  ACMPC_TRY(upload_tables(c, s));
  if (c->sw.dynamic_matrix_rounds) {
    ACMPC_TRY(ensure_matrix(c));
  }
  ACMPC_HIP(c, hipMemcpyAsync(c->d_x0, x0, static_cast<size_t>(P) * acmpc::kDynamicStateFloats * sizeof(float),
                              hipMemcpyHostToDevice, s));
  ACMPC_HIP(c, hipMemcpyAsync(c->d_centre, centre, path_bytes, hipMemcpyHostToDevice, s));
  if (u_ref != nullptr) ACMPC_HIP(c, hipMemcpyAsync(c->d_uref, u_ref, path_bytes, hipMemcpyHostToDevice, s));
  double scale = 1.0;
  for (int r = 0; r < rounds; ++r, scale *= shrink) {
    RoundCentre from;
    ACMPC_TRY(round_centre(c, r, u_ref != nullptr, P, n, s, &from));
    if (c->sw.dynamic_matrix_rounds) {
      ACMPC_TRY(matrix_round(c, c->d_x0, from, nullptr, nullptr, P, N, n, r, rounds, sigma[0] * scale, sigma[1] * scale, seed, s));
      continue;
    }
    ACMPC_TRY(rollout_sampled_dynamic(c, c->d_x0, from.centre, from.stride, from.ref, P, N, n, 0, sigma[0] * scale, sigma[1] * scale,
                                      seed, static_cast<uint32_t>(r), softmin ? c->d_costs : nullptr, s));
    // (the centre may be the u block of c->d_records itself: the finalize reads it before it rewrites the record)
    const Regenerate regen{from.centre, from.stride, from.ref,
                           make_spec(c, sigma[0] * scale, sigma[1] * scale, seed, static_cast<uint32_t>(r))};
    ACMPC_TRY(finalize(c, nullptr, softmin ? c->d_keys : nullptr, c->d_x0, nullptr, P, N, n, layout, 0, c->d_records,
                       acmpc::dynamic_blocks_per_problem(P, N, c->vehicles.K), s, &regen));
    if (softmin && r + 1 < rounds) {   // (reads d_centre in its first launch, writes the mean there in its second)
      ACMPC_TRY(softmin_sampled(c, c->d_costs, c->d_keys, from.centre, from.stride, from.ref, P, N, n, 0, sigma[0] * scale,
                                sigma[1] * scale, seed, static_cast<uint32_t>(r), c->d_centre, nullptr, s));
    }
  }
  ACMPC_HIP(c, hipMemcpyAsync(records, c->d_records, static_cast<size_t>(P) * rec_floats * sizeof(float),
                              hipMemcpyDeviceToHost, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  return ACMPC_OK;
}

}  // namespace capi
}  // namespace acmpc

extern "C" {

static_assert(acmpc::kSampledSingle == ACMPC_ROUND_SINGLE && acmpc::kSampledPair == ACMPC_ROUND_PAIR &&
              acmpc::kSampledQuad == ACMPC_ROUND_QUAD && acmpc::kSampledTrio == ACMPC_ROUND_TRIO, "include/acmpc.h");

int acmpc_describe_rounds(const acmpc_ctx* c, int32_t P, int32_t N, int32_t n, int32_t out[8]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "mode D has no sampled rounds of these forms");
  if (P < 1 || N < 1 || n < 1) return fail(c, ACMPC_EINVAL, "P, N and n must be positive");
  if (P > c->prm.max_problems || N > c->prm.max_candidates || n > c->prm.max_steps)
    return fail(c, ACMPC_ECAPACITY, "shape exceeds the handle's capacity");
  const bool tabulated = paths_tabulate_frames(c, n);
  const bool fused = !c->sw.no_fused_sampling && c->prm.centre_update == 0;   // (else: rounds through the control matrix)
  const RoundPlan plan = fused ? plan_rounds(c, P, N, n) : RoundPlan{};
  const acmpc::SampledForm form = acmpc::choose_sampled_form(c->prm.mode, n, plan.traced, plan.fused_finalize,
                                                             tabulated && !c->sw.no_verified_search, c->opt);
  const char* why = nullptr;
  out[0] = fused ? form.kernel : -1;
  out[1] = plan.fused_finalize ? 1 : 0;
  out[2] = plan.traced ? 1 : 0;
  out[3] = plan.chained ? 1 : 0;
  out[4] = (fused && form.frames) ? 1 : 0;
  out[5] = tabulated ? 1 : 0;
  out[6] = tick_check(c, n + 1, 1, N, &why) == ACMPC_OK ? 1 : 0;
  out[7] = (out[6] != 0 && tick_tabulates_frames(c, n)) ? 1 : 0;
  return ACMPC_OK;
}

int acmpc_optimize(acmpc_ctx* c, const float* x0, const float* centre, const float* u_ref, int32_t P, int32_t N,
                   int32_t n, int32_t rounds, const double sigma[2], double shrink, uint64_t seed, float* records) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (x0 == nullptr || centre == nullptr || sigma == nullptr || records == nullptr)
    return fail(c, ACMPC_EINVAL, "null argument");
  if (rounds < 1) return fail(c, ACMPC_EINVAL, "rounds must be positive");
  const int layout = ACMPC_LAYOUT_STEP_MAJOR;
  ACMPC_TRY(check_shape(c, P, N, n, layout));
  if (c->prm.mode == ACMPC_MODE_DYNAMIC && c->prm.centre_update == 1 && !(c->prm.softmin_lambda > 0.0))
    return fail(c, ACMPC_EINVAL, "softmin_lambda must be positive");
  ACMPC_TRY(ensure_device(c));
  ACMPC_TRY(ensure_staging(c));
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) {
    return optimize_dynamic(c, x0, centre, u_ref, P, N, n, rounds, sigma, shrink, seed, records);
  }
  hipStream_t s = c->stream;
  const size_t x0_bytes = static_cast<size_t>(P) * 3 * sizeof(float);
  const size_t path_bytes = static_cast<size_t>(P) * n * 2 * sizeof(float);
  const size_t table_bytes = static_cast<size_t>(P) * n * c->coef_stride * sizeof(float);
  const size_t rec_bytes = static_cast<size_t>(P) * acmpc_record_floats(n) * sizeof(float);
  const bool has_uref = u_ref != nullptr;
  // the LQ plans of these paths from these start states: candidate 2 of the last round (acmpc_params::lq_candidate)
  const bool has_extra = c->prm.lq_candidate != 0 && c->h_tables.size() == static_cast<size_t>(P) * 7 * n;
  if (has_extra) {
    for (int p = 0; p < P; ++p) {
      const double start[3] = {x0[3 * p], x0[3 * p + 1], x0[3 * p + 2]};
      (void)lq_plan_into(c, c->h_tables.data() + static_cast<size_t>(p) * 7 * n, n, start, c->h_lq + static_cast<size_t>(p) * n * 2,
                         false, p);
    }
  }

  // Eager path: when rollout launches are being timed (event pairs cannot be captured) or on request.
  if (c->prof_used < c->prof_start.size() || c->sw.no_graph) {
    ACMPC_TRY(upload_tables(c, s));
    ACMPC_HIP(c, hipMemcpyAsync(c->d_x0, x0, x0_bytes, hipMemcpyHostToDevice, s));
    ACMPC_HIP(c, hipMemcpyAsync(c->d_centre, centre, path_bytes, hipMemcpyHostToDevice, s));
    if (has_uref) ACMPC_HIP(c, hipMemcpyAsync(c->d_uref, u_ref, path_bytes, hipMemcpyHostToDevice, s));
    OptInputs in{c->d_x0, c->d_centre, has_uref ? c->d_uref : nullptr, c->d_coef, own_frames(c)};
    in.extra = has_extra ? c->h_lq : nullptr;   // (pinned: the last round reads the plans in place)
    ACMPC_TRY(enqueue_rounds(c, in, P, N, n, rounds, sigma[0], sigma[1], shrink, seed, nullptr, s,
                             !c->sw.no_fused_sampling && c->prm.centre_update == 0));
    ACMPC_HIP(c, hipMemcpyAsync(records, c->d_records, rec_bytes, hipMemcpyDeviceToHost, s));
    ACMPC_HIP(c, hipStreamSynchronize(s));
    return ACMPC_OK;
  }

  // Graph path.  Pinned staging block layout: x0 | centre | u_ref | table | seed (each 16-byte aligned).
  auto align16 = [](size_t v) { return (v + 15) & ~static_cast<size_t>(15); };
  const size_t off_x0 = 0, off_centre = align16(off_x0 + x0_bytes), off_uref = align16(off_centre + path_bytes),
               off_table = align16(off_uref + path_bytes), off_seed = align16(off_table + table_bytes);
  if (!c->opt_ready) {
    const acmpc_params& p = c->prm;
    const size_t cap = 64 + 16 * 5 + static_cast<size_t>(p.max_problems) *
                                         (3 + 4 * static_cast<size_t>(p.max_steps) +
                                          static_cast<size_t>(p.max_steps) * c->coef_stride) * sizeof(float);
    ACMPC_HIP(c, host_alloc_once(&c->h_opt, cap));
    ACMPC_HIP(c, alloc_once(&c->d_opt, cap));
    c->opt_capacity = cap;
    ACMPC_HIP(c, host_alloc_once(&c->h_opt_records,
                                 static_cast<size_t>(p.max_problems) * acmpc_record_floats(p.max_steps) * sizeof(float)));
    ACMPC_HIP(c, alloc_once(&c->d_seed, 2 * sizeof(uint32_t)));
    c->opt_ready = true;
  }
  OptKey key;
  key.P = P;
  key.N = N;
  key.n = n;
  key.rounds = rounds;
  key.has_uref = (has_uref ? 1 : 0) | (has_extra ? 2 : 0);
  key.sigma_v = sigma[0];
  key.sigma_k = sigma[1];
  key.shrink = shrink;
  int slot = c->opt_graphs.find(key);
  if (slot < 0) {
    auto enqueue = [&](hipStream_t q, int* rc_rounds) -> hipError_t {
      // ONE host-to-device copy brings x0, centre, u_ref, the table and the seed; the kernels read them in place
      const size_t in_bytes = off_seed + 2 * sizeof(uint32_t);
      hipError_t e = hipMemcpyAsync(c->d_opt, c->h_opt, in_bytes, hipMemcpyHostToDevice, q);
      const bool fused = !c->sw.no_fused_sampling && c->prm.centre_update == 0;
      OptInputs in{reinterpret_cast<const float*>(c->d_opt + off_x0), reinterpret_cast<const float*>(c->d_opt + off_centre),
                   has_uref ? reinterpret_cast<const float*>(c->d_opt + off_uref) : nullptr,
                   reinterpret_cast<const float*>(c->d_opt + off_table), own_frames(c)};
      in.extra = has_extra ? c->h_lq : nullptr;
      if (!fused) {  // the three-kernel form runs on the handle's own buffers: copy the block's parts there
        auto spread = [&](void* dst, size_t off, size_t bytes) {
          if (e == hipSuccess) e = hipMemcpyAsync(dst, c->d_opt + off, bytes, hipMemcpyDeviceToDevice, q);
        };
        spread(c->d_x0, off_x0, x0_bytes);
        spread(c->d_centre, off_centre, path_bytes);
        if (has_uref) spread(c->d_uref, off_uref, path_bytes);
        spread(c->d_coef, off_table, table_bytes);
        in = OptInputs{c->d_x0, c->d_centre, has_uref ? c->d_uref : nullptr, c->d_coef, own_frames(c)};
        in.extra = has_extra ? c->h_lq : nullptr;
      }
      // with the fused finalize the last round writes the winners straight into the pinned host buffer (posted
      // writes over the host link, visible once the stream has drained): no device-to-host copy node
      const bool direct = fused && use_fused_finalize(c, n);
      if (e == hipSuccess)
        *rc_rounds = enqueue_rounds(c, in, P, N, n, rounds, sigma[0], sigma[1], shrink, 0,
                                    reinterpret_cast<const uint32_t*>(c->d_opt + off_seed), q, fused,
                                    direct ? c->h_opt_records : nullptr);
      if (e == hipSuccess && *rc_rounds == ACMPC_OK && !direct)
        e = hipMemcpyAsync(c->h_opt_records, c->d_records, rec_bytes, hipMemcpyDeviceToHost, q);
      return e;
    };
    ACMPC_TRY(c->opt_graphs.capture(c, s, key, "capturing the optimisation graph", enqueue, &slot));
  }
  const hipGraphExec_t graph = c->opt_graphs.use(slot);
  std::memcpy(c->h_opt + off_x0, x0, x0_bytes);
  std::memcpy(c->h_opt + off_centre, centre, path_bytes);
  if (has_uref) std::memcpy(c->h_opt + off_uref, u_ref, path_bytes);
  std::memcpy(c->h_opt + off_table, c->h_coef.data(), table_bytes);
  const uint32_t seed_words[2] = {static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)};
  std::memcpy(c->h_opt + off_seed, seed_words, sizeof seed_words);
  ACMPC_TRY(upload_frames(c, s));
  ACMPC_HIP(c, hipGraphLaunch(graph, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  std::memcpy(records, c->h_opt_records, rec_bytes);
  return ACMPC_OK;
}

}  // extern "C"
