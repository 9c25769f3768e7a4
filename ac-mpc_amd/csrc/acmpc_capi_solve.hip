// C ABI, the solves (include/acmpc.h).  This unit owns the kernels' argument blocks as the handle fills them (rollout_args,
// finalize_args, softmin_args), one launch each of rollout / finalize / sample, the one-launch and the batched solve, the
// round through the control matrix, and the entry points built from them: acmpc_solve, the *_device calls, the stream of
// batches, the sampled and softmin calls, and the timing of the rollout launches (acmpc_profile_*, start clocks).
#include <algorithm>

#include "acmpc_ctx.h"

using namespace acmpc::capi;

namespace acmpc {
namespace capi __attribute__((visibility("hidden"))) {

// mode D: the kernels' view of the handle's rate and slip terms - every float derived in float64 and rounded once
// ("Rate and slip terms").  A part whose weights are 0 and whose limits are +inf is off.  And of its
// objective ("Progress and ceiling"): the progress part is on with a weight that is not 0, the ceiling part when one is set.
// And of its tyre coupling ("Tyre coupling"): the two ratios.
// And of its load transfer ("Load transfer"): the six scalars of each vehicle, and the ratios +inf while the coupling is off.
// And of its obstacles ("Obstacles"): the device block (positions, then radii), what it was set for, and the clearance
// setting; K = 0 while none are set, the soft part on with a weight that is not 0.
// And of its surface table ("Surface"): the device table and what it was set for.
// And of its actuator lag ("Actuator"): the four floats, and the positions' device block while positions are set.
// And of its road table ("Road"): the device table and what it was set for.
acmpc::WithActuator<acmpc::WithObstacles<acmpc::TermsRoad>> dynamics_terms(const acmpc_ctx* c) {
  acmpc::WithActuator<acmpc::WithObstacles<acmpc::TermsRoad>> t{};
  t.rate = (c->rate_weight[0] != 0.0 || c->rate_weight[1] != 0.0 || std::isfinite(c->rate_max[0]) ||
            std::isfinite(c->rate_max[1])) ? 1 : 0;
  t.slip = (c->slip_weight != 0.0 || std::isfinite(c->slip_max)) ? 1 : 0;
  t.inv_dt = static_cast<float>(1.0 / c->prm.dt);
  t.hwd = 0.5f * static_cast<float>(c->rate_weight[0]);
  t.hwp = 0.5f * static_cast<float>(c->rate_weight[1]);
  t.hws = 0.5f * static_cast<float>(c->slip_weight);
  t.rd_max = static_cast<float>(c->rate_max[0]);
  t.rp_max = static_cast<float>(c->rate_max[1]);
  t.b_max = static_cast<float>(c->slip_max);
  t.u_prev = (t.rate != 0 && c->uprev_P != 0) ? c->d_uprev : nullptr;
  t.progress = (c->progress_weight != 0.0) ? 1 : 0;
  t.ceiling = c->has_ceiling ? 1 : 0;
  t.nwp = -static_cast<float>(c->progress_weight);
  t.cs = static_cast<float>(c->speed_ceiling[0]);
  t.co = static_cast<float>(c->speed_ceiling[1]);
  t.q = c->d_progress;
  t.coupled = c->has_coupling ? 1 : 0;
  t.rho_f = c->coupling[0];
  t.rho_r = c->coupling[1];
  t.loaded = c->has_load ? 1 : 0;
  t.aero = c->has_aero ? 1 : 0;   // ("Downforce": c_h = w_max = 0 while the load transfer is off)
  t.k_f = c->aero[0];
  t.k_r = c->aero[1];
  t.v_sat = c->aero[2];
  for (int k = 0; k < c->vehicles.K && (t.loaded != 0 || t.aero != 0); ++k) {
    const float* lc = c->load_const[k];
    t.c_h[k] = lc[0];
    t.w_max[k] = lc[1];
    t.a1_f[k] = lc[2];
    t.a2_f[k] = lc[3];
    t.a1_r[k] = lc[4];
    t.a2_r[k] = lc[5];
  }
  // ("Surface": the top-tier step whatever is on - the downforce's neutral values while it is off, and the load scalars of the
  // vehicles derived all the same)
  // ("Actuator": the same top-tier step, over the vehicle's own peaks while no table is set)
  if (c->has_actuator) {
    t.lag.actuator = 1;
    t.lag.k_d = c->actuator_k[0];
    t.lag.m_d = c->actuator_m[0];
    t.lag.k_p = c->actuator_k[1];
    t.lag.m_p = c->actuator_m[1];
    t.lag.a0 = (c->astate_P != 0) ? c->d_astate : nullptr;   // (as u_prev: every mode D call uploads first)
    t.lag.a0_P = c->astate_P;
  }
  if (c->surf_P != 0) {
    t.surface = 1;
    if (!c->surf_dirty && c->d_surface != nullptr) {   // (every mode D call uploads first; a launch without the table is refused)
      t.mu = c->d_surface;
      t.mu_P = c->surf_P;
      t.mu_n = c->surf_n;
    }
  }
  // ("Road": the same top-tier step again, with or without the surface's scales)
  if (c->road_P != 0) {
    t.road = 1;
    if (!c->road_dirty && c->d_road != nullptr) {   // (every mode D call uploads first; a launch without the table is refused)
      t.road_rows = c->d_road;
      t.road_P = c->road_P;
      t.road_n = c->road_n;
    }
  }
  if (c->surf_P != 0 || c->has_actuator || c->road_P != 0) {
    if (t.aero == 0) {
      t.k_f = t.k_r = 0.0f;
      t.v_sat = 100.0f;
    }
    for (int k = 0; k < c->vehicles.K && t.loaded == 0 && t.aero == 0; ++k) {
      float lc[6];
      surface_load_const(c, k, lc);
      t.c_h[k] = lc[0];
      t.w_max[k] = lc[1];
      t.a1_f[k] = lc[2];
      t.a2_f[k] = lc[3];
      t.a1_r[k] = lc[4];
      t.a2_r[k] = lc[5];
    }
    if (t.coupled == 0) t.rho_f = t.rho_r = HUGE_VALF;
  }
  t.K = c->obs_K;
  if (t.K != 0 && !c->obs_dirty && c->d_obs != nullptr) {   // (every mode D call uploads first; a launch without the data is refused)
    t.obs = c->d_obs;
    t.radii = c->d_obs + static_cast<size_t>(c->obs_P) * c->obs_n * c->obs_K * 2;
    t.P = c->obs_P;
    t.n = c->obs_n;
    t.soft = (static_cast<float>(c->clearance_weight) != 0.0f) ? 1 : 0;
    t.hwo = 0.5f * static_cast<float>(c->clearance_weight);
    t.mg = static_cast<float>(c->clearance_margin);
  }
  return t;
}

// mode D: the kernels' view of the handle's integration setting, for the vehicles it has now - every float derived in
// float64 and rounded once ("Sub-steps and the low-speed blend")
acmpc::Integration dynamics_integration(const acmpc_ctx* c) {
  acmpc::Integration g{};
  g.substeps = c->substeps;
  g.h = static_cast<float>(c->prm.dt / c->substeps);
  g.blend = (c->blend_hi > 0.0) ? 1 : 0;
  if (g.blend != 0) {
    g.v_lo = static_cast<float>(c->blend_lo);
    g.inv_span = static_cast<float>(1.0 / (c->blend_hi - c->blend_lo));
  }
  for (int k = 0; k < c->vehicles.K; ++k) g.inv_L[k] = static_cast<float>(1.0 / c->vehicle_L[k]);
  return g;
}

// (timing armed - acmpc_profile_enable: the launch takes the next event pair; else both stay null)
void next_event_pair(acmpc_ctx* c, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (c->prof_used < c->prof_start.size()) {
    *e0 = c->prof_start[c->prof_used];
    *e1 = c->prof_stop[c->prof_used];
    ++c->prof_used;
  }
}

// the handle's own table and - mode T, exhaustive search - the frames of its paths (empty in the other modes)
acmpc::RolloutArgs rollout_args(const acmpc_ctx* c, const float* d_x0, const float* d_U, float* d_costs, int P, int N, int n,
                                int64_t offset, size_t set) {
  acmpc::RolloutArgs a{};
  a.U = d_U;
  a.x0 = d_x0;
  a.coef = c->d_coef;
  a.nn_frames = (!c->h_nn_frames.empty() && !c->sw.no_verified_search) ? c->d_nn_frames : nullptr;
  a.costs = d_costs;
  a.partial_keys = c->d_partial_keys + set * c->partial_slots;
  a.partial_feas = c->d_partial_feas + set * c->partial_slots;
  a.P = P;
  a.N = N;
  a.n = n;
  a.index_offset = offset;
  a.w = c->w;
  return a;
}

// `regen`: the winner re-drawn from its index (counter-based candidates) instead of read from U
acmpc::FinalizeArgs finalize_args(const acmpc_ctx* c, const Regenerate* regen, const int64_t* d_keys_in, int64_t* d_keys_out,
                                  const float* d_x0, const float* d_U, int P, int N, int n, int64_t offset, float* d_records,
                                  int blocks_per_problem, size_t set) {
  acmpc::FinalizeArgs a{};
  if (regen != nullptr) {
    a.regenerate = true;
    a.centre = regen->d_centre;
    a.centre_stride = regen->centre_stride;
    a.u_ref = regen->d_uref;
    a.u_extra = regen->d_extra;
    a.spec = regen->spec;
  }
  a.U = d_U;
  a.x0 = d_x0;
  a.coef = c->d_coef;
  a.partial_keys = c->d_partial_keys + set * c->partial_slots;
  a.partial_feas = c->d_partial_feas + set * c->partial_slots;
  a.keys_in = d_keys_in;
  a.keys_out = d_keys_out;
  a.records = d_records;
  a.blocks_per_problem = blocks_per_problem;
  a.P = P;
  a.N = N;
  a.n = n;
  a.index_offset = offset;
  a.w = c->w;
  return a;
}

// `d_U`: the control matrix, or nullptr when a sampled launch re-draws the candidates (launch_softmin_sampled)
static acmpc::SoftminArgs softmin_args(const acmpc_ctx* c, const float* d_costs, const int64_t* d_keys, const float* d_U, int P,
                                       int N, int n, float* d_mean, double* d_weight_sum) {
  acmpc::SoftminArgs a{};
  a.costs = d_costs;
  a.keys = d_keys;
  a.U = d_U;
  a.partial = c->d_soft_partial;
  a.mean = d_mean;
  a.weight_sum = d_weight_sum;
  a.chunks = acmpc::softmin_chunks(N);
  a.P = P;
  a.N = N;
  a.n = n;
  a.lambda = static_cast<float>(c->prm.softmin_lambda);
  return a;
}

int rollout(acmpc_ctx* c, const float* d_x0, const float* d_U, int P, int N, int n, int layout, int64_t offset,
            float* d_costs, hipStream_t s, acmpc::LaunchShape* shape_out) {
  acmpc::RolloutArgs a = rollout_args(c, d_x0, d_U, d_costs, P, N, n, offset);
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) {   // mode D: its own kernel (acmpc_dynamic.hip)
    ACMPC_HIP(c, acmpc::launch_rollout_dynamic(layout, a, c->vehicles, dynamics_integration(c), dynamics_terms(c), s));
    *shape_out = acmpc::LaunchShape{};
    shape_out->blocks_per_problem = acmpc::dynamic_blocks_per_problem(P, N, c->vehicles.K);
    return ACMPC_OK;
  }
  const acmpc::LaunchShape shape = acmpc::choose_shape(P, N, layout, c->prm.mode, n, c->opt);
  hipEvent_t e0, e1;
  next_event_pair(c, &e0, &e1);
  c->start_clock_count = 0;
  if (c->want_start_clocks && !shape.tile) {
    const size_t slots = static_cast<size_t>(P) * shape.blocks_per_problem;
    if (slots > c->start_clock_slots) {
      if (c->d_start_clock != nullptr) (void)hipFree(c->d_start_clock);
      c->d_start_clock = nullptr;
      c->start_clock_slots = 0;
      ACMPC_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_start_clock), slots * sizeof(unsigned long long)));
      c->start_clock_slots = slots;
    }
    a.start_clock = c->d_start_clock;
    c->start_clock_count = static_cast<int>(slots);
  }
  ACMPC_HIP(c, acmpc::launch_rollout(c->prm.mode, layout, shape, a, s, e0, e1));
  *shape_out = shape;
  return ACMPC_OK;
}

int finalize(acmpc_ctx* c, const int64_t* d_keys_in, int64_t* d_keys_out, const float* d_x0, const float* d_U, int P,
             int N, int n, int layout, int64_t offset, float* d_records, int blocks_per_problem, hipStream_t s,
             const Regenerate* regen, const float* d_coef_override) {
  acmpc::FinalizeArgs a = finalize_args(c, regen, d_keys_in, d_keys_out, d_x0, d_U, P, N, n, offset, d_records, blocks_per_problem);
  if (d_coef_override != nullptr) a.coef = d_coef_override;
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) {
    ACMPC_TRY(upload_previous_control(c, s));   // (a finalize follows a rollout that has brought it up already)
    ACMPC_HIP(c, acmpc::launch_finalize_dynamic(layout, a, c->vehicles, dynamics_integration(c), dynamics_terms(c), s));
    return ACMPC_OK;
  }
  ACMPC_HIP(c, acmpc::launch_finalize(c->prm.mode, layout, a, s, c->opt));
  return ACMPC_OK;
}

// raised-cosine blend between kSampleKnots knots spread evenly over the n steps: seg [n][2] = (left knot, its weight) and
// the first step of every knot's segment.  upload_segments and acmpc_describe_softmin both take the table from here.
static void knot_table(int n, std::vector<float>& seg, int (&knot_begin)[acmpc::kKnots + 1]) {
  seg.assign(static_cast<size_t>(n) * 2, 0.0f);
  const double width = static_cast<double>(n - 1) / (acmpc::kSampleKnots - 1);
  for (int i = 0; i < n; ++i) {
    const double pos = (n > 1) ? i / width : 0.0;
    int k0 = static_cast<int>(std::floor(pos));
    if (k0 > acmpc::kSampleKnots - 2) k0 = acmpc::kSampleKnots - 2;
    const double frac = pos - k0;
    seg[2 * i] = static_cast<float>(k0);
    seg[2 * i + 1] = static_cast<float>(0.5 * (1.0 + std::cos(3.14159265358979323846 * frac)));
  }
  // first step of every knot's segment (left knots are non-decreasing in the step index)
  for (int k = 0; k <= acmpc::kSampleKnots; ++k) knot_begin[k] = n;
  for (int i = n - 1; i >= 0; --i) knot_begin[static_cast<int>(seg[2 * i])] = i;
  for (int k = acmpc::kSampleKnots - 1; k >= 0; --k)
    if (knot_begin[k] > knot_begin[k + 1]) knot_begin[k] = knot_begin[k + 1];
  knot_begin[0] = 0;
}

int upload_segments(acmpc_ctx* c, int n, hipStream_t s) {
  if (c->segments_n == n) return ACMPC_OK;
  // a pending batch of acmpc_solve_stream_device re-draws its winners with the knot table of ITS horizon, in place in
  // d_segments: it must have run before the table is rewritten for another (acmpc_solve_stream_device flushes it itself)
  if (c->stream_pending)
    return fail(c, ACMPC_ESTATE, "a batch of acmpc_solve_stream_device with another horizon is pending: acmpc_solve_stream_flush first");
  std::vector<float> seg;
  knot_table(n, seg, c->knot_begin);
  ACMPC_HIP(c, hipMemcpyAsync(c->d_segments, seg.data(), seg.size() * sizeof(float), hipMemcpyHostToDevice, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));  // `seg` is a local
  c->segments_n = n;
  return ACMPC_OK;
}

acmpc::SampleSpec make_spec(const acmpc_ctx* c, double sigma_v, double sigma_k, uint64_t seed, uint32_t round) {
  acmpc::SampleSpec sp{};
  sp.segments = c->d_segments;
  sp.seed_lo = static_cast<uint32_t>(seed);
  sp.seed_hi = static_cast<uint32_t>(seed >> 32);
  sp.seed_ptr = nullptr;
  for (int k = 0; k <= acmpc::kKnots; ++k) sp.knot_begin[k] = c->knot_begin[k];
  sp.round = round;
  sp.sigma_v = static_cast<float>(sigma_v);
  sp.sigma_k = static_cast<float>(sigma_k);
  sp.ulo0 = c->w.ulo0;
  sp.ulo1 = c->w.ulo1;
  sp.uhi0 = c->w.uhi0;
  sp.uhi1 = c->w.uhi1;
  return sp;
}

// what a sampler draws for: the centre, candidate 1 and the spread of one round (the launches add what else they take)
static acmpc::SampleArgs sample_args(const acmpc_ctx* c, const float* d_centre, int centre_stride, const float* d_uref, int P,
                                     int N, int n, int64_t offset, double sigma_v, double sigma_k, uint64_t seed, uint32_t round) {
  acmpc::SampleArgs a{};
  a.centre = d_centre;
  a.u_ref = d_uref;
  a.centre_stride = centre_stride;
  a.P = P;
  a.N = N;
  a.n = n;
  a.index_offset = offset;
  a.spec = make_spec(c, sigma_v, sigma_k, seed, round);
  return a;
}

static int sample(acmpc_ctx* c, const float* d_centre, int centre_stride, const float* d_uref, int P, int N, int n,
                  int layout, int64_t offset, double sigma_v, double sigma_k, uint64_t seed, uint32_t round, float* d_U,
                  hipStream_t s, const uint32_t* d_seed = nullptr, const float* d_extra = nullptr) {
  ACMPC_TRY(upload_segments(c, n, s));  // no-op once the table for this n is resident
  acmpc::SampleArgs a = sample_args(c, d_centre, centre_stride, d_uref, P, N, n, offset, sigma_v, sigma_k, seed, round);
  a.u_extra = d_extra;
  a.U = d_U;
  a.spec.seed_ptr = d_seed;
  ACMPC_HIP(c, acmpc::launch_sample(layout, a, s));
  return ACMPC_OK;
}

// mode D: the rollout that draws its own candidates (acmpc_dynamic.hip: launch_rollout_dynamic_sampled) - what sample() into
// a matrix and rollout() of it compute, without the matrix
int rollout_sampled_dynamic(acmpc_ctx* c, const float* d_x0, const float* d_centre, int centre_stride, const float* d_uref,
                            int P, int N, int n, int64_t offset, double sigma_d, double sigma_p, uint64_t seed, uint32_t round,
                            float* d_costs, hipStream_t s) {
  ACMPC_TRY(upload_segments(c, n, s));
  ACMPC_HIP(c, acmpc::launch_rollout_dynamic_sampled(
                   rollout_args(c, d_x0, nullptr, d_costs, P, N, n, offset),
                   sample_args(c, d_centre, centre_stride, d_uref, P, N, n, offset, sigma_d, sigma_p, seed, round), c->vehicles,
                   dynamics_integration(c), dynamics_terms(c), s));
  return ACMPC_OK;
}

// the softmin mean of the candidates sample() would write for these arguments, without the matrix
// (acmpc_softmin.hip: launch_softmin_sampled) - what sample() into a matrix and launch_softmin of it compute
int softmin_sampled(acmpc_ctx* c, const float* d_costs, const int64_t* d_keys, const float* d_centre, int centre_stride,
                    const float* d_uref, int P, int N, int n, int64_t offset, double sigma_v, double sigma_k, uint64_t seed,
                    uint32_t round, float* d_mean, double* d_weight_sum, hipStream_t s) {
  ACMPC_TRY(upload_segments(c, n, s));
  ACMPC_HIP(c, acmpc::launch_softmin_sampled(
                   softmin_args(c, d_costs, d_keys, nullptr, P, N, n, d_mean, d_weight_sum),
                   sample_args(c, d_centre, centre_stride, d_uref, P, N, n, offset, sigma_v, sigma_k, seed, round), s));
  return ACMPC_OK;
}

// Step-major launches with two or four candidates per lane read their controls and write their costs as ONE 8- or 16-byte
// vector per lane (load_controls, rollout_block: a vector type's natural alignment is what the compiler may assume of the
// address), so the matrix and the cost buffer must start on that boundary; every row then does (N is a multiple of the
// lane's candidates).  Checked from the shape the launch will take, before any device work (include/acmpc.h).
static int check_vector_alignment(const acmpc_ctx* c, int P, int N, int n, int layout, const float* d_U, const float* d_costs) {
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) return ACMPC_OK;
  const acmpc::LaunchShape shape = acmpc::choose_shape(P, N, layout, c->prm.mode, n, c->opt);
  if (shape.tile || shape.cpt < 2) return ACMPC_OK;
  const uintptr_t mask = static_cast<uintptr_t>(shape.cpt) * sizeof(float) - 1;
  if ((reinterpret_cast<uintptr_t>(d_U) & mask) != 0 || (reinterpret_cast<uintptr_t>(d_costs) & mask) != 0) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "a step-major launch with %d candidates per lane needs d_U and d_costs on a %d-byte boundary",
                  shape.cpt, static_cast<int>(mask + 1));
    return fail(c, ACMPC_EINVAL, buf);
  }
  return ACMPC_OK;
}

// acmpc_solve_device / acmpc_solve in ONE launch (rollout_solo_kernel) when the problem is small enough for it: rollout,
// argmin and the winner's record without rolling the winner a second time.  ACMPC_NO_SOLO keeps the two launches.
static bool use_solo(const acmpc_ctx* c, int P, int N, int n, int layout) {
  static_assert(kTraceBlocks >= acmpc::kSoloBlocks, "the trace buffer holds one trace per workgroup");
  return c->prm.mode == ACMPC_MODE_SPATIAL && !c->sw.no_solo && acmpc::solo_fits(P, N, n, layout, c->opt);
}

static int solve_solo(acmpc_ctx* c, const float* d_x0, const float* d_U, int P, int N, int n, int layout, float* d_costs,
                      int64_t* d_keys, float* d_records, hipStream_t s) {
  ACMPC_TRY(ensure_tail_buffers(c));
  acmpc::FusedFinalize ff{};
  ff.tickets = c->d_tickets;
  ff.records = d_records;
  ff.trace = c->d_trace;
  ff.trace_pitch = acmpc::solo_trace_floats(n);
  ff.keys_out = d_keys;
  hipEvent_t e0, e1;
  next_event_pair(c, &e0, &e1);
  ACMPC_HIP(c, acmpc::launch_rollout_solo(layout, rollout_args(c, d_x0, d_U, d_costs, P, N, n, 0), ff, s, e0, e1, c->opt));
  return ACMPC_OK;
}

// The batched solve: rollout_kernel + finalize_kernel, or - ACMPC_TAILED_ROLLOUT=1, where the shape allows it (mode S,
// step-major, the 256-thread launch shapes) - both in ONE launch (rollout_tailed_kernel: the last workgroup of a problem
// finalizes it).  The same bits either way (tests/test_gpu_tailed_rollout.py).  The one launch is NOT the default: measured
// on the headline's batch (4 096 x 4 096 x 49, same box) it ends the step's launch gap - ms_per_step 1.145 against a
// kernel of 1.138 - but the kernel grows by 47 us (every workgroup's first wave waits for its ticket's round trip before
// it retires, 16 384 times, and 4 096 lone-wave re-rolls take issue slots from the streaming waves), more than the 29 us
// finalize_kernel + gap it replaces: 1.125 ms per step in two launches.  `regen`: the winner re-drawn from its index
// (counter-based candidates) instead of read from U.
static int solve_batched(acmpc_ctx* c, const float* d_x0, const float* d_U, int P, int N, int n, int layout, float* d_costs,
                         int64_t* d_keys, float* d_records, hipStream_t s, const Regenerate* regen) {
  const acmpc::LaunchShape shape = acmpc::choose_shape(P, N, layout, c->prm.mode, n, c->opt);
  if (!c->sw.tailed_rollout || d_records == nullptr || !acmpc::tailed_rollout_fits(c->prm.mode, layout, shape, n)) {
    acmpc::LaunchShape used;
    ACMPC_TRY(rollout(c, d_x0, d_U, P, N, n, layout, 0, d_costs, s, &used));
    return finalize(c, nullptr, d_keys, d_x0, regen != nullptr ? nullptr : d_U, P, N, n, layout, 0, d_records,
                    used.blocks_per_problem, s, regen);
  }
  ACMPC_TRY(ensure_tail_buffers(c));
  hipEvent_t e0, e1;
  next_event_pair(c, &e0, &e1);
  ACMPC_HIP(c, acmpc::launch_rollout_tailed(
                   layout, shape, rollout_args(c, d_x0, d_U, d_costs, P, N, n, 0),
                   finalize_args(c, regen, nullptr, d_keys, d_x0, d_U, P, N, n, 0, d_records, shape.blocks_per_problem),
                   c->d_tickets, s, e0, e1));
  return ACMPC_OK;
}

// Round r on the handle's own buffers samples round d_centre first, later round the incumbent = the u block of the records,
// with the caller's u_ref as candidate 1.  Softmin rounds (centre_update = 1) after the first: candidate 0 = the weighted
// mean the previous round wrote into d_centre, candidate 1 = the previous round's winner - the best plan found so far is
// never lost - which reads its controls at a stride of 2n: the winner's u block is staged contiguously here.
int round_centre(acmpc_ctx* c, int r, bool has_uref, int P, int n, hipStream_t s, RoundCentre* out) {
  const int rec_floats = acmpc_record_floats(n);
  const bool mean_round = c->prm.centre_update == 1 && r > 0;
  const bool own = r == 0 || mean_round;
  *out = RoundCentre{own ? c->d_centre : c->d_records + ACMPC_REC_HEADER, own ? 2 * n : rec_floats,
                     (has_uref || mean_round) ? c->d_uref : nullptr};
  if (mean_round)
    ACMPC_HIP(c, hipMemcpy2DAsync(c->d_uref, static_cast<size_t>(2 * n) * sizeof(float), c->d_records + ACMPC_REC_HEADER,
                                  static_cast<size_t>(rec_floats) * sizeof(float),
                                  static_cast<size_t>(2 * n) * sizeof(float), P, hipMemcpyDeviceToDevice, s));
  return ACMPC_OK;
}

// With softmin every round but the last leaves the weighted mean of its candidates in d_centre, the next round's centre.
int matrix_round(acmpc_ctx* c, const float* d_x0, const RoundCentre& from, const float* d_extra, const uint32_t* d_seed, int P,
                 int N, int n, int r, int rounds, double sigma_v, double sigma_k, uint64_t seed, hipStream_t s) {
  const int layout = ACMPC_LAYOUT_STEP_MAJOR;
  const bool softmin = c->prm.centre_update == 1;
  ACMPC_TRY(sample(c, from.centre, from.stride, from.ref, P, N, n, layout, 0, sigma_v, sigma_k, seed, static_cast<uint32_t>(r),
                   c->d_U, s, d_seed, d_extra));
  acmpc::LaunchShape shape;
  ACMPC_TRY(rollout(c, d_x0, c->d_U, P, N, n, layout, 0, softmin ? c->d_costs : nullptr, s, &shape));
  ACMPC_TRY(finalize(c, nullptr, softmin ? c->d_keys : nullptr, d_x0, c->d_U, P, N, n, layout, 0, c->d_records,
                     shape.blocks_per_problem, s));
  if (softmin && r + 1 < rounds)
    ACMPC_HIP(c, acmpc::launch_softmin(layout, softmin_args(c, c->d_costs, c->d_keys, c->d_U, P, N, n, c->d_centre, nullptr), s));
  return ACMPC_OK;
}

// acmpc_solve in mode D: copies up, rollout + finalize (acmpc_dynamic.hip), copies down
static int solve_dynamic_host(acmpc_ctx* c, const float* x0, const float* U, int P, int N, int n, int layout, float* costs,
                       int32_t* best_idx, float* records) {
  hipStream_t s = c->stream;
  const size_t cand = static_cast<size_t>(P) * N;
  ACMPC_TRY(ensure_matrix(c));
  ACMPC_HIP(c, hipMemcpyAsync(c->d_x0, x0, static_cast<size_t>(P) * acmpc::kDynamicStateFloats * sizeof(float),
                              hipMemcpyHostToDevice, s));
  ACMPC_HIP(c, hipMemcpyAsync(c->d_U, U, cand * n * 2 * sizeof(float), hipMemcpyHostToDevice, s));
  acmpc::LaunchShape shape;
  ACMPC_TRY(rollout(c, c->d_x0, c->d_U, P, N, n, layout, 0, costs != nullptr ? c->d_costs : nullptr, s, &shape));
  ACMPC_TRY(finalize(c, nullptr, c->d_keys, c->d_x0, c->d_U, P, N, n, layout, 0, records != nullptr ? c->d_records : nullptr,
                     shape.blocks_per_problem, s));
  ACMPC_HIP(c, hipMemcpyAsync(c->h_keys, c->d_keys, static_cast<size_t>(P) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  if (records != nullptr)
    ACMPC_HIP(c, hipMemcpyAsync(records, c->d_records, static_cast<size_t>(P) * acmpc_record_floats(n) * sizeof(float),
                                hipMemcpyDeviceToHost, s));
  if (costs != nullptr) ACMPC_HIP(c, hipMemcpyAsync(costs, c->d_costs, cand * sizeof(float), hipMemcpyDeviceToHost, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  if (best_idx != nullptr)
    for (int p = 0; p < P; ++p) best_idx[p] = static_cast<int32_t>(acmpc_key_index(c->h_keys[p]));
  return ACMPC_OK;
}

}  // namespace capi
}  // namespace acmpc

extern "C" {

int acmpc_rollout_device(acmpc_ctx* c, const float* d_x0, const float* d_U, int32_t P, int32_t N, int32_t n,
                         int32_t layout, int64_t index_offset, float* d_costs, int64_t* d_keys, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_x0 == nullptr || d_U == nullptr) return fail(c, ACMPC_EINVAL, "null device pointer");
  if (index_offset < 0 || index_offset + N > 0xffffffffLL) return fail(c, ACMPC_EINVAL, "global index exceeds 32 bits");
  ACMPC_TRY(check_shape(c, P, N, n, layout));
  ACMPC_TRY(check_vector_alignment(c, P, N, n, layout, d_U, d_costs));
  ACMPC_TRY(ensure_device(c));
  hipStream_t s = static_cast<hipStream_t>(stream);
  ACMPC_TRY(upload_tables(c, s));
  acmpc::LaunchShape shape;
  const int rc = rollout(c, d_x0, d_U, P, N, n, layout, index_offset, d_costs, s, &shape);
  if (rc != ACMPC_OK || d_keys == nullptr) return rc;
  return finalize(c, nullptr, d_keys, d_x0, d_U, P, N, n, layout, index_offset, nullptr, shape.blocks_per_problem, s);
}

int acmpc_finalize_device(acmpc_ctx* c, const int64_t* d_keys, const float* d_x0, const float* d_U, int32_t P,
                          int32_t N, int32_t n, int32_t layout, int64_t index_offset, float* d_records,
                          void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_x0 == nullptr || d_U == nullptr || d_records == nullptr) return fail(c, ACMPC_EINVAL, "null device pointer");
  if (index_offset < 0 || index_offset + N > 0xffffffffLL) return fail(c, ACMPC_EINVAL, "global index exceeds 32 bits");
  ACMPC_TRY(check_shape(c, P, N, n, layout));
  if (!c->device_ready) return fail(c, ACMPC_ESTATE, "acmpc_rollout_device must run first");
  const int blocks = c->prm.mode == ACMPC_MODE_DYNAMIC ? acmpc::dynamic_blocks_per_problem(P, N, c->vehicles.K)
                                                       : acmpc::choose_shape(P, N, layout, c->prm.mode, n, c->opt).blocks_per_problem;
  return finalize(c, d_keys, nullptr, d_x0, d_U, P, N, n, layout, index_offset, d_records, blocks,
                  static_cast<hipStream_t>(stream));
}

int acmpc_solve_device(acmpc_ctx* c, const float* d_x0, const float* d_U, int32_t P, int32_t N, int32_t n,
                       int32_t layout, float* d_costs, int64_t* d_keys, float* d_records, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_x0 == nullptr || d_U == nullptr) return fail(c, ACMPC_EINVAL, "null device pointer");
  if (d_keys == nullptr && d_records == nullptr) return fail(c, ACMPC_EINVAL, "need d_keys and/or d_records");
  ACMPC_TRY(check_shape(c, P, N, n, layout));
  if (!use_solo(c, P, N, n, layout)) ACMPC_TRY(check_vector_alignment(c, P, N, n, layout, d_U, d_costs));
  ACMPC_TRY(ensure_device(c));
  hipStream_t s = static_cast<hipStream_t>(stream);
  ACMPC_TRY(upload_tables(c, s));
  if (use_solo(c, P, N, n, layout)) return solve_solo(c, d_x0, d_U, P, N, n, layout, d_costs, d_keys, d_records, s);
  return solve_batched(c, d_x0, d_U, P, N, n, layout, d_costs, d_keys, d_records, s, nullptr);
}

int acmpc_solve_sampled_device(acmpc_ctx* c, const float* d_x0, const float* d_U, const float* d_centre,
                               int32_t centre_stride, const float* d_u_ref, int32_t P, int32_t N, int32_t n, int32_t layout,
                               double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round, float* d_costs,
                               int64_t* d_keys, float* d_records, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_x0 == nullptr || d_U == nullptr || d_centre == nullptr || d_records == nullptr)
    return fail(c, ACMPC_EINVAL, "null device pointer");
  if (centre_stride < 2 * n) return fail(c, ACMPC_EINVAL, "centre_stride must be at least 2 n");
  ACMPC_TRY(check_shape(c, P, N, n, layout));
  ACMPC_TRY(check_vector_alignment(c, P, N, n, layout, d_U, d_costs));
  ACMPC_TRY(ensure_device(c));
  hipStream_t s = static_cast<hipStream_t>(stream);
  ACMPC_TRY(upload_tables(c, s));
  ACMPC_TRY(upload_segments(c, n, s));
  const Regenerate regen{d_centre, centre_stride, d_u_ref, make_spec(c, sigma_v, sigma_kappa, seed, round)};
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) {   // two launches: the rollout of d_U, the finalize that re-draws the winners
    acmpc::LaunchShape used;
    ACMPC_TRY(rollout(c, d_x0, d_U, P, N, n, layout, 0, d_costs, s, &used));
    return finalize(c, nullptr, d_keys, d_x0, nullptr, P, N, n, layout, 0, d_records, used.blocks_per_problem, s, &regen);
  }
  return solve_batched(c, d_x0, d_U, P, N, n, layout, d_costs, d_keys, d_records, s, &regen);
}

static_assert(ACMPC_ROLLOUT_STEP == 0 && ACMPC_ROLLOUT_TILE == 1 && ACMPC_ROLLOUT_ROWS_LDS == 2 && ACMPC_ROLLOUT_ROWS_SCALAR == 3,
              "include/acmpc.h");

int acmpc_describe_rollout(const acmpc_ctx* c, int32_t P, int32_t N, int32_t n, int32_t layout, int32_t out[8]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "mode D has its own rollout: no launch shapes of these forms");
  if (P < 1 || N < 1 || n < 1) return fail(c, ACMPC_EINVAL, "P, N and n must be positive");
  if (layout != ACMPC_LAYOUT_CANDIDATE_MAJOR && layout != ACMPC_LAYOUT_STEP_MAJOR) return fail(c, ACMPC_EINVAL, "unknown layout");
  if (P > c->prm.max_problems || N > c->prm.max_candidates || n > c->prm.max_steps)
    return fail(c, ACMPC_ECAPACITY, "shape exceeds the handle's capacity");
  const int mode = c->prm.mode;
  const acmpc::LaunchShape shape = acmpc::choose_shape(P, N, layout, mode, n, c->opt);
  // the finalize a batch of this shape leaves pending for the next call of a stream (acmpc_solve_stream_device: records
  // wanted, the partial keys its own, the winners re-drawn or read from the same layout); only whether a pointer is null counts
  static float some_records;
  acmpc::FinalizeArgs pending{};
  pending.records = &some_records;
  pending.P = P;
  pending.N = N;
  pending.n = n;
  pending.blocks_per_problem = shape.blocks_per_problem;
  const bool rows = shape.tile && shape.tile_waves == 4;   // (launch_rollout_ml; there also: the matrix on a 16-byte boundary)
  out[0] = shape.block;
  out[1] = shape.cpt;
  out[2] = shape.cpt >= 2 ? shape.pack : 1;
  out[3] = shape.blocks_per_problem;
  out[4] = rows ? (acmpc::tile_rows_table_in_lds(shape, P, n) ? ACMPC_ROLLOUT_ROWS_LDS : ACMPC_ROLLOUT_ROWS_SCALAR)
                : shape.tile ? ACMPC_ROLLOUT_TILE : ACMPC_ROLLOUT_STEP;
  out[5] = acmpc::tailed_rollout_fits(mode, layout, shape, n) ? 1 : 0;
  out[6] = acmpc::chained_rollout_fits(mode, layout, shape, P, pending, layout) ? 1 : 0;
  out[7] = use_solo(c, P, N, n, layout) ? 1 : 0;
  return ACMPC_OK;
}

int acmpc_solve_stream_flush(acmpc_ctx* c, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (!c->stream_pending) return ACMPC_OK;
  c->stream_pending = false;
  ACMPC_HIP(c, acmpc::launch_finalize(c->prm.mode, c->stream_fin_layout, c->stream_fin, static_cast<hipStream_t>(stream), c->opt));
  return ACMPC_OK;
}

int acmpc_solve_stream_device(acmpc_ctx* c, const float* d_x0, const float* d_U, const float* d_centre,
                              int32_t centre_stride, const float* d_u_ref, int32_t P, int32_t N, int32_t n, int32_t layout,
                              double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round, float* d_costs,
                              int64_t* d_keys, float* d_records, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode == ACMPC_MODE_DYNAMIC)
    return fail(c, ACMPC_ESTATE, "mode D has no stream of batches: use acmpc_solve_device / acmpc_solve_sampled_device");
  if (d_x0 == nullptr || d_U == nullptr || d_records == nullptr) return fail(c, ACMPC_EINVAL, "null device pointer");
  if (d_centre != nullptr && centre_stride < 2 * n) return fail(c, ACMPC_EINVAL, "centre_stride must be at least 2 n");
  ACMPC_TRY(check_shape(c, P, N, n, layout, true));
  ACMPC_TRY(check_vector_alignment(c, P, N, n, layout, d_U, d_costs));
  ACMPC_TRY(ensure_device(c));
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the pending finalize reads the tables its batch was rolled with: new ones go up behind it
  // (and the sampler's knot table of its horizon: upload_segments rewrites it in place for another)
  if (c->stream_pending && (c->tables_dirty || c->frames_dirty || (d_centre != nullptr && c->segments_n != n))) {
    ACMPC_TRY(acmpc_solve_stream_flush(c, stream));
  }
  ACMPC_TRY(upload_tables(c, s));
  if (d_centre != nullptr) {
    ACMPC_TRY(upload_segments(c, n, s));
  }
  const acmpc::LaunchShape shape = acmpc::choose_shape(P, N, layout, c->prm.mode, n, c->opt);
  const int set = c->stream_pending ? (c->stream_set ^ 1) : 0;
  const acmpc::RolloutArgs a = rollout_args(c, d_x0, d_U, d_costs, P, N, n, 0, set);
  const Regenerate regen{d_centre, centre_stride, d_u_ref, make_spec(c, sigma_v, sigma_kappa, seed, round)};
  const acmpc::FinalizeArgs f = finalize_args(c, d_centre != nullptr ? &regen : nullptr, nullptr, d_keys, d_x0,
                                              d_centre != nullptr ? nullptr : d_U, P, N, n, 0, d_records,
                                              shape.blocks_per_problem, set);
  hipEvent_t e0, e1;
  next_event_pair(c, &e0, &e1);
  if (c->stream_pending &&
      acmpc::chained_rollout_fits(c->prm.mode, layout, shape, P, c->stream_fin, c->stream_fin_layout) && !c->sw.no_chained_stream) {
    c->stream_pending = false;
    ACMPC_HIP(c, acmpc::launch_rollout_chained(layout, shape, a, c->stream_fin, c->stream_fin_layout, s, e0, e1));
  } else {
    ACMPC_TRY(acmpc_solve_stream_flush(c, stream));
    ACMPC_HIP(c, acmpc::launch_rollout(c->prm.mode, layout, shape, a, s, e0, e1));
  }
  c->stream_fin = f;
  c->stream_fin_layout = layout;
  c->stream_set = set;
  c->stream_pending = true;
  return ACMPC_OK;
}

int acmpc_solve(acmpc_ctx* c, const float* x0, const float* U, int32_t P, int32_t N, int32_t n, int32_t layout,
                float* costs, int32_t* best_idx, float* records) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (x0 == nullptr || U == nullptr) return fail(c, ACMPC_EINVAL, "null input");
  ACMPC_TRY(check_shape(c, P, N, n, layout));
  ACMPC_TRY(ensure_device(c));
  ACMPC_TRY(ensure_staging(c));
  hipStream_t s = c->stream;
  ACMPC_TRY(upload_tables(c, s));
  if (c->prm.mode == ACMPC_MODE_DYNAMIC) return solve_dynamic_host(c, x0, U, P, N, n, layout, costs, best_idx, records);
  const size_t cand = static_cast<size_t>(P) * N;
  const size_t rec_bytes = static_cast<size_t>(P) * acmpc_record_floats(n) * sizeof(float);
  // Nothing small crosses the host link as a copy of its own (round 4): the start states are written into the handle's
  // page-locked block and READ THERE by the kernels, keys and records are written there BY the kernels (page-locked host
  // memory is device-addressable: what acmpc_control_tick does with its tick block) - each of those copies was a packet of
  // ~4 us in the stream.  The control matrix is read in place too when the caller built it in page-locked memory
  // (acmpc_host_alloc): the rollout then streams it over the host link while it computes, instead of behind a copy of the
  // whole matrix; from pageable memory it is staged into device memory as before.  ACMPC_NO_ZERO_COPY=1: every transfer a copy.
  float* h_x0 = c->h_io;
  float* h_records = c->h_io + ((static_cast<size_t>(P) * 3 + 3) & ~static_cast<size_t>(3));   // (16-byte aligned)
  std::memcpy(h_x0, x0, static_cast<size_t>(P) * 3 * sizeof(float));
  const bool solo = use_solo(c, P, N, n, layout);
  // (the one-launch solve: a few workgroups, latency is everything.  A batch of thousands of problems keeps its small
  // copies - every workgroup fetching its start state over the host link would be thousands of requests for one packet)
  const bool in_place = !c->sw.no_zero_copy && solo;
  const float* d_x0 = c->d_x0;
  const float* d_U = c->d_U;
  int64_t* d_keys = c->d_keys;
  float* d_records = records != nullptr ? c->d_records : nullptr;
  if (in_place) {
    d_x0 = h_x0;
    d_keys = c->h_keys;
    if (records != nullptr) d_records = h_records;
  } else {
    ACMPC_HIP(c, hipMemcpyAsync(c->d_x0, h_x0, static_cast<size_t>(P) * 3 * sizeof(float), hipMemcpyHostToDevice, s));
  }
  if (!c->sw.no_zero_copy) {
    hipPointerAttribute_t where{};
    if (hipPointerGetAttributes(&where, U) == hipSuccess && where.type == hipMemoryTypeHost && where.devicePointer != nullptr) {
      d_U = static_cast<const float*>(where.devicePointer);
    } else {
      (void)hipGetLastError();   // (pageable memory is not an error here)
    }
  }
  if (d_U == c->d_U) ACMPC_HIP(c, hipMemcpyAsync(c->d_U, U, cand * n * 2 * sizeof(float), hipMemcpyHostToDevice, s));
  if (solo) {
    ACMPC_TRY(solve_solo(c, d_x0, d_U, P, N, n, layout, costs != nullptr ? c->d_costs : nullptr, d_keys, d_records, s));
  } else {
    acmpc::LaunchShape shape;
    ACMPC_TRY(check_vector_alignment(c, P, N, n, layout, d_U, nullptr));   // (a matrix read in place may be a view)
    ACMPC_TRY(rollout(c, d_x0, d_U, P, N, n, layout, 0, costs != nullptr ? c->d_costs : nullptr, s, &shape));
    ACMPC_TRY(finalize(c, nullptr, d_keys, d_x0, d_U, P, N, n, layout, 0, d_records, shape.blocks_per_problem, s));
  }
  if (!in_place) {
    ACMPC_HIP(c, hipMemcpyAsync(c->h_keys, c->d_keys, static_cast<size_t>(P) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (records != nullptr) ACMPC_HIP(c, hipMemcpyAsync(h_records, c->d_records, rec_bytes, hipMemcpyDeviceToHost, s));
  }
  if (costs != nullptr) ACMPC_HIP(c, hipMemcpyAsync(costs, c->d_costs, cand * sizeof(float), hipMemcpyDeviceToHost, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  if (records != nullptr) std::memcpy(records, h_records, rec_bytes);
  if (best_idx != nullptr)
    for (int p = 0; p < P; ++p) best_idx[p] = static_cast<int32_t>(acmpc_key_index(c->h_keys[p]));
  return ACMPC_OK;
}

int acmpc_sample_device(acmpc_ctx* c, const float* d_centre, int32_t centre_stride, const float* d_u_ref, int32_t P,
                        int32_t N, int32_t n, int32_t layout, int64_t index_offset, double sigma_v, double sigma_kappa,
                        uint64_t seed, uint32_t round, float* d_U, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_centre == nullptr || d_U == nullptr) return fail(c, ACMPC_EINVAL, "null device pointer");
  if (centre_stride < 2 * n) return fail(c, ACMPC_EINVAL, "centre_stride must be at least 2 n");
  if (index_offset < 0 || index_offset + N > 0xffffffffLL) return fail(c, ACMPC_EINVAL, "global index exceeds 32 bits");
  // (allowed while a batch of acmpc_solve_stream_device is pending: drawing the next batch's candidates touches neither
  // the tables nor the partial keys the pending finalize reads)
  ACMPC_TRY(check_shape(c, P, N, n, layout, true));
  ACMPC_TRY(ensure_device(c));
  return sample(c, d_centre, centre_stride, d_u_ref, P, N, n, layout, index_offset, sigma_v, sigma_kappa, seed, round,
                d_U, static_cast<hipStream_t>(stream));
}

int acmpc_finalize_sampled_device(acmpc_ctx* c, const int64_t* d_keys, const float* d_x0, const float* d_centre,
                                  int32_t centre_stride, const float* d_u_ref, int32_t P, int32_t N, int32_t n,
                                  double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round, float* d_records,
                                  void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_x0 == nullptr || d_centre == nullptr || d_records == nullptr) return fail(c, ACMPC_EINVAL, "null device pointer");
  if (centre_stride < 2 * n) return fail(c, ACMPC_EINVAL, "centre_stride must be at least 2 n");
  ACMPC_TRY(check_shape(c, P, N, n, ACMPC_LAYOUT_STEP_MAJOR));
  if (!c->device_ready) return fail(c, ACMPC_ESTATE, "acmpc_rollout_device must run first");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ACMPC_TRY(upload_segments(c, n, s));
  Regenerate regen{d_centre, centre_stride, d_u_ref, make_spec(c, sigma_v, sigma_kappa, seed, round)};
  const int blocks = c->prm.mode == ACMPC_MODE_DYNAMIC
                         ? acmpc::dynamic_blocks_per_problem(P, N, c->vehicles.K)
                         : acmpc::choose_shape(P, N, ACMPC_LAYOUT_STEP_MAJOR, c->prm.mode, n, c->opt).blocks_per_problem;
  return finalize(c, d_keys, nullptr, d_x0, nullptr, P, N, n, ACMPC_LAYOUT_STEP_MAJOR, 0, d_records, blocks, s, &regen);
}

int acmpc_rollout_sampled_device(acmpc_ctx* c, const float* d_x0, const float* d_centre, int32_t centre_stride,
                                 const float* d_u_ref, int32_t P, int32_t N, int32_t n, int64_t index_offset,
                                 double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round, float* d_costs,
                                 int64_t* d_keys, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_x0 == nullptr || d_centre == nullptr) return fail(c, ACMPC_EINVAL, "null device pointer");
  if (c->prm.mode != ACMPC_MODE_DYNAMIC)
    return fail(c, ACMPC_ESTATE, "acmpc_rollout_sampled_device is mode D's: modes S and T draw inside acmpc_optimize");
  if (centre_stride < 2 * n) return fail(c, ACMPC_EINVAL, "centre_stride must be at least 2 n");
  if (index_offset < 0 || index_offset + N > 0xffffffffLL) return fail(c, ACMPC_EINVAL, "global index exceeds 32 bits");
  ACMPC_TRY(check_shape(c, P, N, n, ACMPC_LAYOUT_STEP_MAJOR));
  ACMPC_TRY(ensure_device(c));
  hipStream_t s = static_cast<hipStream_t>(stream);
  ACMPC_TRY(upload_tables(c, s));
  const int rc = rollout_sampled_dynamic(c, d_x0, d_centre, centre_stride, d_u_ref, P, N, n, index_offset, sigma_v, sigma_kappa, seed,
                               round, d_costs, s);
  if (rc != ACMPC_OK || d_keys == nullptr) return rc;
  return finalize(c, nullptr, d_keys, d_x0, nullptr, P, N, n, ACMPC_LAYOUT_STEP_MAJOR, index_offset, nullptr,
                  acmpc::dynamic_blocks_per_problem(P, N, c->vehicles.K), s);
}

int acmpc_rollout_start_clocks(acmpc_ctx* c, uint64_t* out, int32_t capacity, int32_t* count) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out == nullptr || count == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  *count = c->start_clock_count;
  if (c->start_clock_count == 0) return ACMPC_OK;
  if (capacity < c->start_clock_count) return fail(c, ACMPC_ECAPACITY, "start clocks: capacity below the launch's workgroups");
  ACMPC_HIP(c, hipDeviceSynchronize());
  ACMPC_HIP(c, hipMemcpy(out, c->d_start_clock, static_cast<size_t>(c->start_clock_count) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return ACMPC_OK;
}

int acmpc_profile_enable(acmpc_ctx* c, int32_t capacity) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (capacity < 0) return fail(c, ACMPC_EINVAL, "negative capacity");
  ACMPC_TRY(ensure_device(c));
  while (static_cast<int32_t>(c->prof_start.size()) < capacity) {
    hipEvent_t e0, e1;
    ACMPC_HIP(c, hipEventCreate(&e0));
    ACMPC_HIP(c, hipEventCreate(&e1));
    c->prof_start.push_back(e0);
    c->prof_stop.push_back(e1);
  }
  while (static_cast<int32_t>(c->prof_start.size()) > capacity) {
    (void)hipEventDestroy(c->prof_start.back());
    (void)hipEventDestroy(c->prof_stop.back());
    c->prof_start.pop_back();
    c->prof_stop.pop_back();
  }
  c->prof_used = 0;
  return ACMPC_OK;
}

int acmpc_profile_collect(acmpc_ctx* c, float* out_ms, int32_t capacity, int32_t* count) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out_ms == nullptr || count == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  const int32_t used = static_cast<int32_t>(c->prof_used);
  const int32_t take = used < capacity ? used : capacity;
  for (int32_t i = 0; i < take; ++i) {
    ACMPC_HIP(c, hipEventSynchronize(c->prof_stop[i]));
    ACMPC_HIP(c, hipEventElapsedTime(&out_ms[i], c->prof_start[i], c->prof_stop[i]));
  }
  *count = take;
  c->prof_used = 0;
  return ACMPC_OK;
}

int acmpc_softmin_device(acmpc_ctx* c, const float* d_costs, const int64_t* d_keys, const float* d_U, int32_t P,
                         int32_t N, int32_t n, int32_t layout, float* d_mean, double* d_weight_sum, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_costs == nullptr || d_keys == nullptr || d_U == nullptr || d_mean == nullptr)
    return fail(c, ACMPC_EINVAL, "null device pointer");
  ACMPC_TRY(check_shape(c, P, N, n, layout));
  if (!(c->prm.softmin_lambda > 0.0)) return fail(c, ACMPC_EINVAL, "softmin_lambda must be positive");
  ACMPC_TRY(ensure_device(c));
  const acmpc::SoftminArgs a = softmin_args(c, d_costs, d_keys, d_U, P, N, n, d_mean, d_weight_sum);
  ACMPC_HIP(c, acmpc::launch_softmin(layout, a, static_cast<hipStream_t>(stream)));
  return ACMPC_OK;
}

int acmpc_softmin_sampled_device(acmpc_ctx* c, const float* d_costs, const int64_t* d_keys, const float* d_centre,
                                 int32_t centre_stride, const float* d_u_ref, int32_t P, int32_t N, int32_t n,
                                 int64_t index_offset, double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round,
                                 float* d_mean, double* d_weight_sum, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (d_costs == nullptr || d_keys == nullptr || d_centre == nullptr || d_mean == nullptr)
    return fail(c, ACMPC_EINVAL, "null device pointer");
  if (centre_stride < 2 * n) return fail(c, ACMPC_EINVAL, "centre_stride must be at least 2 n");
  if (index_offset < 0 || index_offset + N > 0xffffffffLL) return fail(c, ACMPC_EINVAL, "global index exceeds 32 bits");
  if (!(c->prm.softmin_lambda > 0.0)) return fail(c, ACMPC_EINVAL, "softmin_lambda must be positive");
  ACMPC_TRY(check_shape(c, P, N, n, ACMPC_LAYOUT_STEP_MAJOR));
  ACMPC_TRY(ensure_device(c));
  return softmin_sampled(c, d_costs, d_keys, d_centre, centre_stride, d_u_ref, P, N, n, index_offset, sigma_v, sigma_kappa,
                         seed, round, d_mean, d_weight_sum, static_cast<hipStream_t>(stream));
}

static_assert(ACMPC_SOFTMIN_CANDIDATE_MAJOR == ACMPC_LAYOUT_CANDIDATE_MAJOR && ACMPC_SOFTMIN_STEP_MAJOR == ACMPC_LAYOUT_STEP_MAJOR,
              "include/acmpc.h");

int acmpc_describe_softmin(const acmpc_ctx* c, int32_t P, int32_t N, int32_t n, int32_t form, int32_t out[8]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  // what check_shape refuses of a shape alone, and the softmin calls after it
  if (c->prm.mode == ACMPC_MODE_DYNAMIC && !c->has_dynamics)
    return fail(c, ACMPC_ESTATE, "mode D: acmpc_set_dynamics has not been called");
  if (P < 1 || N < 1 || n < 1) return fail(c, ACMPC_EINVAL, "P, N and n must be positive");
  if (form != ACMPC_SOFTMIN_CANDIDATE_MAJOR && form != ACMPC_SOFTMIN_STEP_MAJOR && form != ACMPC_SOFTMIN_SAMPLED)
    return fail(c, ACMPC_EINVAL, "unknown form");
  if (P > c->prm.max_problems || N > c->prm.max_candidates || n > c->prm.max_steps)
    return fail(c, ACMPC_ECAPACITY, "shape exceeds the handle's capacity");
  if (!(c->prm.softmin_lambda > 0.0)) return fail(c, ACMPC_EINVAL, "softmin_lambda must be positive");
  for (int q = 0; q < 8; ++q) out[q] = 0;
  out[0] = acmpc::softmin_chunks(N);
  if (form == ACMPC_SOFTMIN_CANDIDATE_MAJOR) {
    const acmpc::SoftminRows rows = acmpc::softmin_rows(n);
    out[1] = rows.groups;
    out[2] = rows.passes;
  } else if (form == ACMPC_SOFTMIN_SAMPLED) {
    std::vector<float> seg;
    int knot_begin[acmpc::kKnots + 1];
    knot_table(n, seg, knot_begin);
    const int items = acmpc::softmin_item_count(knot_begin);
    const acmpc::SoftminItems walk = acmpc::softmin_items(out[0], P, items);
    out[3] = items;
    out[4] = walk.grid_z;
    out[5] = walk.per_wave;
  }
  return ACMPC_OK;
}

}  // extern "C"
