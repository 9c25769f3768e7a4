/*
 * acmpc.h - C ABI of the MI355X (gfx950) rollout-and-cost engine for the ac-mpc controller.
 *
 * This is the drop-in boundary of SURVEY.md section 8(b).  The reference is pure Python, so there is no
 * FFI to bind to; each entry point names the reference interface whose work it takes over
 * (paths relative to /root/reference/).  Host code stays Python and calls these through ctypes
 * (`ac-mpc_amd/acmpc_amd/_capi.py`; reference-side stub in INTEGRATION.md).
 *
 * Conventions
 *   - every function returns 0 on success or a negative ACMPC_E* code; no exception crosses the ABI;
 *     `acmpc_last_error()` gives the message of the last failure on that handle;
 *   - a handle is not thread-safe; buffers passed in are only read for the duration of the call;
 *   - a handle lives on ONE device (`acmpc_params.device`, or the thread's current device when -1): the calling
 *     thread's current HIP device must be that device on every call (one process per GPU does this once);
 *   - `acmpc_create`, `acmpc_set_paths` and `acmpc_get_coefficients` do no device work: the reference builds
 *     its MPC objects in the parent process and then forks the ControlProcess
 *     (src/acmpc/control/controller.py:94-100,293-297), so the HIP context is created lazily on the first call
 *     that needs the GPU, in whichever process makes it;
 *   - "n" is the number of control steps = horizon - 1 = len(ReferencePath)
 *     (src/acmpc/control/spatial_mpc.py:133-134), "N" the number of candidate control sequences per problem,
 *     "P" the number of independent problems (poses) evaluated by one launch;
 *   - a candidate is n pairs (v, kappa): the decision variables u of the reference QP
 *     (src/acmpc/control/solvers/control.py:26-28); steering angle = atan(kappa * wheelbase)
 *     (spatial_mpc.py:195-196).
 *
 * Rollout arithmetic is float32 in one fixed operation order with no implicit FMA contraction: mode S uses no
 * fused multiply-add at all, mode T uses exactly the ones its specification names (the
 * oracle calls fmaf / emulates it exactly), so results are bit-identical to oracle/acmpc_oracle.{py,c}.
 * The per-tick prologue (acmpc_control_tick) is float64; its tolerances are stated in DESIGN.md section 2.
 */
#ifndef ACMPC_H
#define ACMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACMPC_OK 0
#define ACMPC_EINVAL (-1)    /* bad argument (null pointer, size out of range, unknown mode/layout)      */
#define ACMPC_EHIP (-2)      /* a HIP runtime call failed; message carries hipGetErrorString             */
#define ACMPC_ENODEVICE (-3) /* no usable GPU / HIP runtime: the product path never falls back to the CPU */
#define ACMPC_ECAPACITY (-4) /* P, N or n exceeds what the handle was created for                         */
#define ACMPC_ESTATE (-5)    /* call order violated (e.g. solve before set_paths)                          */

/* Rollout model. */
#define ACMPC_MODE_SPATIAL 0  /* x_{i+1} = A_i x_i + B_i (u_i - u_ref_i) + f_i, x = (e_y, e_psi, t):
                                 dynamics.py:65-103 + control.py:26-45 ("mode S")                        */
#define ACMPC_MODE_TEMPORAL 1 /* Cartesian kinematic Euler step (localisation/localiser.py:66-95) with
                                 nearest-waypoint Frenet projection (localiser.py:282-289, dynamics.py:23-40)
                                 ("mode T")                                                               */
#define ACMPC_MODE_DYNAMIC 2  /* the six-state dynamic bicycle with Pacejka lateral tyre forces
                                 (control/dynamic_bicycle_model.py:88-160, one explicit Euler step of dt with vx
                                 clipped at 0 after it), scored with mode T's nearest-waypoint projection and cost
                                 ("mode D").  Start states x0 [P][6] = (X, Y, yaw, vx, vy, r); a candidate is n pairs
                                 (delta, pedal), the pedal in [-1, 1]; the vehicle comes from acmpc_set_dynamics,
                                 or K vehicles from acmpc_set_dynamics_ensemble: every candidate is then scored under
                                 each, its cost the weighted MEAN or the MAX of the K costs, its violation the max of
                                 the K violations, the record's x its trajectory under vehicle 0 - through every call
                                 form below, unchanged.
                                 Tables as mode T's (acmpc_set_paths); max_steps <= 512; lq_candidate must be 0.
                                 Takes acmpc_set_paths / acmpc_set_coefficients, acmpc_solve, acmpc_solve_device,
                                 acmpc_rollout_device + acmpc_finalize_device (index_offset, acmpc_reduce_across_ranks),
                                 acmpc_softmin_device, acmpc_sample_device, the calls that re-draw a winner from its
                                 index (acmpc_finalize_sampled_device, acmpc_solve_sampled_device: sigma_v, sigma_kappa
                                 = sigma_delta, sigma_pedal; candidate 2 does not exist), acmpc_rollout_sampled_device
                                 (the rollout that draws its own candidates: no control matrix) and acmpc_optimize
                                 (that rollout + the re-drawing finalize per round, two launches;
                                 ACMPC_DYNAMIC_MATRIX_ROUNDS keeps sample -> rollout -> finalize through the matrix,
                                 the same bits).  With centre_update = 1 acmpc_optimize recentres on the softmin mean
                                 as modes S and T do - the mean of a round is acmpc_softmin_sampled_device's, which
                                 re-draws the candidates instead of reading a matrix (a third launch per round but
                                 the last; under ACMPC_DYNAMIC_MATRIX_ROUNDS acmpc_softmin_device over the matrix, the
                                 same bits).  ACMPC_ESTATE from acmpc_control_tick and acmpc_solve_stream_device.
                                 DESIGN.md section 2 "Mode D". */

/* Memory layout of the control-sample matrix U. */
#define ACMPC_LAYOUT_CANDIDATE_MAJOR 0 /* U[P][N][n][2]  - what NumPy host code naturally holds          */
#define ACMPC_LAYOUT_STEP_MAJOR 1      /* U[P][n][2][N]  - what an on-device sampler writes; lane-coalesced */

/* Width in floats of one row of the packed per-step tables returned by acmpc_get_coefficients. */
#define ACMPC_COEF_STRIDE_SPATIAL 12  /* ds, a21, a31, b31, f3, v_ref, k_ref, ey_lo, ey_hi, 0, 0, 0 */
#define ACMPC_COEF_STRIDE_TEMPORAL 8  /* x, y, cos psi, sin psi, psi, k_ref, v_ref, w/2 - margin     */

/* Header floats of a winner record (see acmpc_record_floats). */
#define ACMPC_REC_COST 0
#define ACMPC_REC_VIOLATION 1
#define ACMPC_REC_NFEASIBLE 2
#define ACMPC_REC_OWNER 3
#define ACMPC_REC_HEADER 4

typedef struct acmpc_ctx acmpc_ctx;

/* Everything SpatialMPC.__init__ / ControlSolver.__setup / SpatialBicycleModel.__init__ hold as scalars
 * (spatial_mpc.py:21-58, control.py:108-158, dynamics.py:10-21). */
typedef struct acmpc_params {
  uint32_t struct_size;  /* sizeof(acmpc_params), for ABI checking                                   */
  int32_t mode;          /* ACMPC_MODE_*                                                              */
  int32_t device;        /* HIP device ordinal                                                        */
  int32_t max_problems;  /* capacity P (<= 65535)                                                     */
  int32_t max_candidates;/* capacity N (per problem)                                                  */
  int32_t max_steps;     /* capacity n (<= 1024)                                                      */
  int32_t nn_back;       /* mode T nearest-waypoint search: the W = nn_back + nn_ahead + 1 consecutive waypoints   */
  int32_t nn_ahead;      /*   from clamp(j_prev - nn_back, 0, n - W), j_prev = the previous step's nearest index (0
                              at the start); nn_ahead < 0 = exhaustive scan of all n waypoints (KDTree.query
                              semantics, localiser.py:282-289)                                                    */
  int32_t centre_update; /* acmpc_optimize: what the next round samples round - 0 = the round's argmin winner,
                            1 = the softmin-weighted mean of the round's candidates (weights exp(-(cost - min) /
                            softmin_lambda), the weighted-reduction form of localiser.py:572-579); in both cases the
                            best candidate so far stays in the pool, so a round never loses it                  */
  int32_t lq_candidate;  /* acmpc_optimize / acmpc_control_tick: 1 = the LAST sampling round's candidate 2 is the LQ plan -
                            the optimum of the reference's control QP (control.py:26-79) without its box rows, a backward
                            Riccati pass over the linearised model (dynamics.py:65-103), rolled forward with its feedback
                            and clipped into the input box (csrc/acmpc_lq.h; host, float64).  acmpc_optimize plans for the
                            paths of acmpc_set_paths and the x0 it is given; acmpc_control_tick, whose table is built on
                            the device, plans on the host meanwhile for this tick's path (acmpc_waypoint_table of `coords`)
                            and pose with this tick's speed profile as well (acmpc_velocity_ceiling +
                            acmpc_speed_profile_exact on that table: the prologue's own two passes; with qp_method 1, or an
                            infeasible profile, the one its PREVIOUS call solved).  With coords = NULL - the path cut
                            out of the map on the device - and a map index the host cuts the same window itself
                            (csrc/acmpc_prologue.h map_path_row: one statement for both sides); with a pose instead, whose
                            nearest map point the device searches, it plans for the previous call's problem as it was (none
                            in a handle's first tick then).  A first tick under qp_method 1 solves the speed profile
                            once on the host (acmpc_speed_profile_qp, cold) to plan with.  The argmin keeps the plan only
                            when it wins.
                            2 = as 1, and where that plan is not already the QP's optimum - a control on the input box, or
                            state rows (corridor control.py:57-60, t >= 0.01 control.py:134) violated beyond the solver's
                            acceptance tolerance - it is refined against the QP WITH its box rows (csrc/acmpc_lq_box.h: the
                            OSQP splitting with the model as a hard constraint of the Riccati z-update; host, float64,
                            iterate kept between calls; at most ACMPC_LQ_BOX_ITERATIONS = 40 iterations per call from a cold start, 12 from a kept iterate) and the
                            cheapest of {LQ plan, the two iterates} under J + w_bound V takes the slot.
                            0 = no such candidate */
  /* real-valued fields are doubles so that Python floats cross the ABI exactly; the device gets float32 */
  double step_cost[3];   /* Q  = diag(step_cost)  on (e_y, e_psi, t)     control.py:126               */
  double r_term[2];      /* R  = diag(r_term)     on (v, kappa)          control.py:127               */
  double final_cost[3];  /* QN = diag(final_cost)                        control.py:128               */
  double u_min[2];       /* QP input box: min_u - (0.1, 0)               control.py:130-139           */
  double u_max[2];       /*               max_u + (0.1, 0)                                           */
  double margin;         /* vehicle width / 2                            dynamics.py:14               */
  double wheelbase;      /* L                                            dynamics.py:11               */
  double t_min;          /* lower bound on the time state, 0.01          control.py:134               */
  double dt;             /* mode T Euler step [s]                                                     */
  double w_bound;        /* penalty weight on squared bound violation (build parameter, default 1e6)  */
  double softmin_lambda; /* temperature of the softmin-weighted mean (build parameter)                */
} acmpc_params;

/* Replaces: SpatialMPC.__init__ + ControlSolver.__setup (spatial_mpc.py:21-58, control.py:108-158).
 * Allocates host state only. */
int acmpc_create(const acmpc_params* params, acmpc_ctx** out);
void acmpc_destroy(acmpc_ctx* ctx);

/* The A/B switches of the tests and the tools (tools/README.md: ACMPC_NO_SOLO, ACMPC_TICK_GRAPH, ACMPC_SHAPE, ...) belong to
 * the handle: acmpc_create reads them from the environment ONCE, and this call sets one afterwards (`name` as the
 * environment spells it; value NULL, "" or - for the on / off ones - "0" restores the default).  No launch path reads the
 * environment.  ACMPC_EINVAL for an unknown name. */
int acmpc_set_option(acmpc_ctx* ctx, const char* name, const char* value);
/* One of them is for deployment rather than for A/B runs: "ACMPC_CONFORMANT_SYNC" = "1".  The default forms of the latency
 * paths lean on what gfx950 does rather than on what HIP and the HSA memory model promise (csrc/acmpc_kernels_impl.h, top):
 * values cross workgroups inside a launch as relaxed agent-scope atomics ordered by s_waitcnt vmcnt(0), waves of a
 * workgroup end while the others still meet at s_barrier, and acmpc_control_tick learns of completion from a flag the
 * last kernel writes into page-locked memory.  With the option on, every solve / round / batch is separate launches
 * ordered by the stream (rollout, then finalize), rounds run on one wave per workgroup, and completion is
 * hipStreamSynchronize - the same bits (tests/test_gpu_conformant.py), a few microseconds more per call
 * (INTEGRATION.md section 6).  Equivalent to ACMPC_NO_SOLO + ACMPC_NO_FUSED_FINALIZE + ACMPC_NO_CHAINED_STREAM +
 * ACMPC_TICK_NO_FLAG (and no ACMPC_TAILED_ROLLOUT). */

/* The LQ plan of acmpc_params::lq_candidate for one path, on the host (csrc/acmpc_lq.h): table [7][n] float64 in the
 * reference's row order, x0 = (e_y, e_psi, t), weights as in acmpc_params, the input box as the kernels hold it;
 * plan [n][2] float32 (v, kappa).  ACMPC_ESTATE when the problem has no finite plan.  No handle, no GPU work. */
int acmpc_lq_plan(const double* table, int32_t n, const double x0[3], const double step_cost[3], const double r_term[2],
                  const double final_cost[3], const float u_min[2], const float u_max[2], float* plan);

/* The plan of acmpc_params::lq_candidate = 2 for one path, on the host (csrc/acmpc_lq_box.h): arguments as acmpc_lq_plan,
 * `margin` / `w_bound` as in acmpc_params, at most `iterations` splitting iterations (12 when that is more and the iterate
 * handed in is a warm one).  `state` [1 + 8 n]: the iterate -
 * state[0] = n marks a warm one (wx, wu, lx, lu [n][2] each behind it), anything else starts cold; written back (state[0]
 * = 0 when the call kept none).  `info` [5]: iterations run (negative: a non-finite iterate), which plan took the slot
 * (0 the LQ plan, 1 the box iterate, 2 the clipped dynamics iterate), whether the refinement was triggered, and the
 * chosen plan's tracking cost J and summed squared state-row excess V (float64 rollout).  ACMPC_ESTATE when the
 * problem has no finite LQ plan.  No handle, no GPU work. */
int acmpc_lq_box_plan(const double* table, int32_t n, const double x0[3], const double step_cost[3], const double r_term[2],
                      const double final_cost[3], const float u_min[2], const float u_max[2], double margin, double w_bound,
                      int32_t iterations, double* state, float* plan, double* info);
/* What the handle's last lq_candidate = 2 plan did: `info` [5] as acmpc_lq_box_plan's. */
int acmpc_lq_box_stats(const acmpc_ctx* ctx, double info[5]);

/* Message of the last failing call on `ctx` (or of the last failing acmpc_create when ctx is NULL). */
const char* acmpc_last_error(const acmpc_ctx* ctx);

/* Replaces: ControlSolver._update_references + _update_problem_bounds (control.py:26-33,47-70), i.e.
 * SpatialBicycleModel.linearise (dynamics.py:65-103) and the corridor bounds, for P reference paths at once.
 * `tables` is P consecutive 7 x n float64 ReferencePath arrays in the reference's row order
 * [x, y, psi, kappa, ds, width, v] (control/paths.py:4-72).  Coefficients are computed in float64 on the host,
 * stored as float32, and uploaded by the next device call.  No device work. */
int acmpc_set_paths(acmpc_ctx* ctx, const double* tables, int32_t P, int32_t n);

/* The packed float32 tables themselves ([P][n][ACMPC_COEF_STRIDE_* by the handle's mode], the layout
 * acmpc_get_coefficients and acmpc_tick_read_device_tables hand out) instead of paths: for callers that keep their
 * tables packed, and for the tests, which feed a tick's own device-built table to the two-call path so that
 * `acmpc_control_tick == acmpc_set_paths + acmpc_optimize` holds bit for bit whatever the last float32 bit of a host
 * cos / sin was.  CONTRACT for handles with lq_candidate != 0: the LQ plan (candidate 2 of the last round) is computed from
 * float64 paths, which this call does not carry - the float64 tables of an earlier acmpc_set_paths of the SAME shape (P, n)
 * stay and are taken to describe the same paths as `coef` (the caller's responsibility: the packed table is meant to be
 * that acmpc_set_paths' own, re-packed); with no such tables, or after a call with another shape, acmpc_optimize runs
 * without the plan (candidate 2 is then an ordinary sample).  Call acmpc_set_paths again to plan for new paths. */
int acmpc_set_coefficients(acmpc_ctx* ctx, const float* coef, int32_t P, int32_t n);

/* Mode D's vehicle: ACMPC_DYNAMICS_COUNT doubles in this order (the names of control/dynamic_bicycle_model.py:7-77):
 *    0 F_z0   1 Bf   2 Cf   3 Df   4 Ef   5 epsf   6 Br   7 Cr   8 Dr   9 Er   10 epsr
 *   11 mass  12 Iz  13 g   14 lf  15 lr  16 brake_bias
 *   17 Cm1   18 Cm2 19 Cm3  20 Cb1  21 Cb2  22 Cb3  23 Cfric1  24 Cfric2  25 Cfric3
 * Lateral forces are D (1 + eps F_z / F_z0) F_z / F_z0 sin(C atan(B a - E (B a - atan(B a)))) with F_zf = mass g lr /
 * (lr + lf), F_zr = mass g lf / (lr + lf); the drive, brake and friction maps are (Cm1 - Cm2 vx - Cm3 vx^2) max(pedal, 0),
 * (Cb1 - Cb2 vx - Cb3 vx^2) min(pedal, 0) split brake_bias front / 1 - brake_bias rear, and -Cfric1 - Cfric2 vx - Cfric3 vx^2.
 * The block is data: its forces must share one unit with mass and Iz (the reference's literal block does not -
 * DESIGN.md section 2; acmpc_amd.DynamicBicycleParams.reference() is the consistent one).  The host derives the float32
 * constants of the kernels from it (in float64, each rounded once).  No device work.  ACMPC_EINVAL for a count other
 * than ACMPC_DYNAMICS_COUNT, a non-finite value, mass <= 0, Iz <= 0, F_z0 == 0, lf + lr == 0, or a handle whose mode
 * is not ACMPC_MODE_DYNAMIC. */
#define ACMPC_DYNAMICS_COUNT 26
int acmpc_set_dynamics(acmpc_ctx* ctx, const double* coef, int32_t count);

/* Mode D's ensemble (scenario-based robust scoring): K vehicle blocks, coef [K][ACMPC_DYNAMICS_COUNT], each validated as
 * acmpc_set_dynamics validates one, with positive weights [K] (or NULL: equal) and a reduce.  Every candidate is rolled
 * from the same x0 and controls under each vehicle k, giving c_k and V_k; weights are normalised on the host in float64,
 * omega_k = w_k / sum_j w_j, each rounded once to float32 (NULL: float32(1 / K)).  The candidate's cost J is
 *   ACMPC_ENSEMBLE_MEAN  J = omega_0 c_0, then J = fma(omega_k, c_k, J) for k = 1 .. K-1, in that order;
 *   ACMPC_ENSEMBLE_MAX   the largest c_k, NaN if any c_k is NaN;
 * its violation V = max_k V_k (NaN if any is NaN), so a feasible candidate is feasible under every vehicle.  J is what
 * `costs`, the keys and the record's cost hold; the record's violation is V, n_feasible counts V == 0, u is the winner's
 * controls and x its trajectory under vehicle 0 (the nominal one).  K = 1 with MEAN is acmpc_set_dynamics bit for bit,
 * and acmpc_set_dynamics after an ensemble goes back to one vehicle.  No device work.  ACMPC_EINVAL for a handle whose
 * mode is not ACMPC_MODE_DYNAMIC, K outside 1 .. ACMPC_MAX_VEHICLES, an unknown reduce, a weight that is not finite or
 * not > 0, or any block acmpc_set_dynamics refuses; the handle then keeps its previous vehicle(s).  DESIGN.md section 2
 * "Mode D", "Ensembles". */
#define ACMPC_MAX_VEHICLES 8
#define ACMPC_ENSEMBLE_MEAN 0
#define ACMPC_ENSEMBLE_MAX 1
int acmpc_set_dynamics_ensemble(acmpc_ctx* ctx, const double* coef, int32_t K, const double* weights, int32_t reduce);

/* Mode D's integration setting: how a control step of dt is integrated.  Off by default - (1, 0, 0): one explicit Euler
 * step, the reference's - and independent of the vehicle: it survives acmpc_set_dynamics and acmpc_set_dynamics_ensemble
 * and applies to every member of an ensemble with that member's lf, lr.
 *   substeps   M in 1 .. ACMPC_MAX_SUBSTEPS: M Euler steps of h = float32(dt / M) (the quotient in float64, rounded
 *              once; M = 1: h == dt) under the same (delta, pedal), vx clipped at 0 after each.  Nearest waypoint, cost,
 *              the record's x row and the terminal cost stay once per control step, on the state after the M-th.
 *   blend      [blend_lo, blend_hi] m/s with 0 <= blend_lo < blend_hi, both finite; 0, 0 is off.  After each sub-step,
 *              lam = clamp((vx - blend_lo) / (blend_hi - blend_lo), 0, 1) and (vy, r) become lam (vy, r) + (1 - lam)
 *              (lr r_k, r_k) with r_k = vx tan(delta) / (lf + lr), the kinematic bicycle's: the dynamic model above
 *              blend_hi bit for bit, the kinematic one below blend_lo.
 * The single Euler step is linearly unstable below about 7.5 m/s for the default vehicle and chatters up to about 12:
 * turn this on (4 sub-steps, blend 3 .. 5) for plans that can fall below that.  Every call form of mode D takes it from
 * the handle.  No device work.  ACMPC_EINVAL for a handle whose mode is not ACMPC_MODE_DYNAMIC, substeps outside
 * 1 .. ACMPC_MAX_SUBSTEPS, or a blend that is neither 0, 0 nor 0 <= lo < hi finite; the handle then keeps its previous
 * setting.  DESIGN.md section 2 "Mode D", "Sub-steps and the low-speed blend". */
#define ACMPC_MAX_SUBSTEPS 16
int acmpc_set_dynamics_integration(acmpc_ctx* ctx, int32_t substeps, double blend_lo, double blend_hi);

/* Mode D's rate and slip terms: what a plan pays for moving its controls quickly and for sliding.  Off by default.  Per
 * control step i, after the stage cost of that step and on the same state:
 *   rd = (delta_i - delta_{i-1}) / dt, rp = (pedal_i - pedal_{i-1}) / dt     the controls' rates; step 0 against the
 *                                                                          previous control (acmpc_set_previous_control)
 *   b  = (r lr - vy) / (vx + 1e-3)                                          the rear slip ratio, lr of the vehicle rolled
 *   J += 1/2 (rate_weight[0] rd^2 + rate_weight[1] rp^2 + slip_weight b^2)
 *   V += max(|rd| - rate_max[0], 0)^2 + max(|rp| - rate_max[1], 0)^2 + max(|b| - slip_max, 0)^2
 * so a plan over a limit is infeasible (V > 0) as one outside the input box is.  Weights are finite and >= 0; limits are
 * > 0, +inf (INFINITY) meaning none; every value is rounded to float32 once.  The rate part is on when a rate weight is
 * not 0 or a rate limit finite, the slip part when slip_weight is not 0 or slip_max finite; a part that is off computes
 * nothing, and with both off the handle runs exactly what it ran before the call.  The setting belongs to the handle: it
 * survives acmpc_set_dynamics, acmpc_set_dynamics_ensemble and acmpc_set_dynamics_integration, every member of an
 * ensemble carries it (the slip part with its own lr), and every call form of mode D takes it from the handle.  b
 * divides by vx + 1e-3: below the speeds where the single Euler step chatters, use the slip part together with the
 * low-speed blend of acmpc_set_dynamics_integration, which drives r lr - vy to 0 there.  No device work.  ACMPC_EINVAL for
 * a handle whose mode is not ACMPC_MODE_DYNAMIC, a null array, a weight that is negative or not finite, a limit that is
 * not > 0 (NaN included); the handle then keeps its previous setting.  DESIGN.md section 2 "Mode D", "Rate and slip
 * terms". */
int acmpc_set_dynamics_terms(acmpc_ctx* ctx, const double rate_weight[2], const double rate_max[2], double slip_weight,
                             double slip_max);

/* Mode D's objective: a terminal progress reward and a per-step speed ceiling, a third and a fourth part of the terms
 * above, both off by default.
 *   progress: with s the arc length made good at the last control step - the arc length of the nearest waypoint j that
 *   step's cost used plus the along-track offset from it, s = fma(sin psi_j, Y, fma(cos psi_j, X, q_j)) with the progress
 *   table q of acmpc_get_progress_table - the cost ends with J = fma(-float32(progress_weight), s, J), between the stage and
 *   terminal sums and the violations' term.  The distance made good over the horizon is the minimum-time objective; it is
 *   the one term that is not a square: COSTS MAY BE NEGATIVE.  Keys, argmin and softmin order negative costs as floats;
 *   -inf, like every non-finite cost, ranks last.  Past the last waypoint j stays n - 1 and s keeps growing linearly.
 *   ceiling: speed_ceiling = (scale, offset), or NULL for none; per control step, after the rate and slip lines,
 *   cap = fma(float32(scale), v_ref_j, float32(offset)); V += max(vx - cap, 0)^2: a plan faster than the ceiling is
 *   infeasible.  A NaN v_ref is no ceiling at that step.  The ceiling is what stops a finite-horizon progress reward from
 *   ending flat out before a corner: give it the speed profile (whose backward pass knows the corner) scaled by what the
 *   tyres allow over what the profile assumed, with weights.r_term[0] = 0 and a slip_max.
 * The progress part is on when progress_weight is not 0, the ceiling part when speed_ceiling is not NULL; a part that is
 * off computes nothing, and with all four parts off the handle runs exactly what it ran before the call.  The setting
 * belongs to the handle: it survives acmpc_set_dynamics, _ensemble, _integration and _terms, every member of an ensemble
 * carries it with its own end state, and every call form of mode D takes it from the handle.  No device work.
 * ACMPC_ESTATE for a handle whose mode is not ACMPC_MODE_DYNAMIC; ACMPC_EINVAL for a weight that is negative or not finite,
 * a scale that is negative or not finite, an offset that is not finite (each as a float32); the handle then keeps its
 * previous setting.  DESIGN.md section 2 "Mode D, progress and ceiling". */
int acmpc_set_dynamics_objective(acmpc_ctx* ctx, double progress_weight, const double speed_ceiling[2] /* NULL: none */);

/* Mode D's tyre coupling: a friction ellipse between each axle's longitudinal and lateral force.  Off by default, when the
 * drive and brake maps do not know the tyres' grip and the Pacejka side force does not know the pedal.  ratio = (rho_f,
 * rho_r), each > 0 and finite, or +inf (INFINITY) for no coupling on that axle, each rounded to float32 once; NULL turns the
 * setting off.  In every Euler step (every sub-step of acmpc_set_dynamics_integration), after the two longitudinal forces and
 * before the accelerations, per axle with P that axle's peak factor (Pf or Pr of the vehicle rolled), all float32, nothing
 * fused:
 *   cap = rho P;  F_x = max(min(F_x, cap), -cap);  u = F_x / cap;  g = sqrt(1 - u u);  F_y = F_y g
 * so an axle cannot push or brake harder than rho times its lateral peak, a saturated axle (|u| = 1) has no side force left,
 * and because P carries Df / Dr a grip scale (DynamicBicycleParams.with_grip, an ensemble's members, the hypotheses of
 * acmpc_score_grips, each with its OWN peaks) now shortens braking and traction too.  pedal == 0 and rho = +inf give the
 * uncoupled step bit for bit.  The friction map is drag, not tyre force, and is left alone.  rho near 1 is a tyre as good
 * along as across.  The setting belongs to the handle: it survives acmpc_set_dynamics, _ensemble, _integration, _terms and
 * _objective, and every call form of mode D takes it from the handle.  While it is on every vehicle of the handle must have
 * Pf, Pr finite and > 0 as float32: whichever call would break that - this one, acmpc_set_dynamics or
 * acmpc_set_dynamics_ensemble - returns ACMPC_EINVAL and leaves the handle as it was.  No device work.  ACMPC_ESTATE for a
 * handle whose mode is not ACMPC_MODE_DYNAMIC; ACMPC_EINVAL for a ratio that is 0, negative or NaN (as a float32).
 * DESIGN.md section 2 "Mode D, tyre coupling". */
int acmpc_set_dynamics_coupling(acmpc_ctx* ctx, const double ratio[2] /* NULL: off */);

/* Mode D's longitudinal load transfer: each axle's load, and with it its Pacejka peak factor and its coupling cap, follows
 * the longitudinal tyre force.  Off by default, when the peaks are those of the static axle loads.  setting = (h_cg, w_frac):
 * h_cg >= 0 and finite, the height of the centre of gravity in the vehicle block's length unit; 0 < w_frac < 1, the most load
 * that may move as a fraction of the lighter axle's static load; NULL turns the setting off.  Per vehicle of the handle the
 * host derives in float64, each rounded to float32 once:
 *   c_h = h_cg / (lf + lr);  w_max = w_frac min(F_zf, F_zr);  e_a = eps_a / F_z0;  N_a = F_za + e_a F_za^2;
 *   a1_a = (1 + 2 e_a F_za) / N_a;  a2_a = e_a / N_a                                   (a = f, r)
 * so that P_a(F_za + x) / P_a(F_za) = 1 + x (a1_a + a2_a x) exactly, whatever D_a (a grip scale).  In every Euler step (every
 * sub-step of acmpc_set_dynamics_integration), after the two longitudinal forces and before anything uses a peak, all
 * float32, nothing fused, min / max the IEEE minNum / maxNum, Pf, Pr the peaks the step would otherwise use and rho the
 * coupling's ratios (+inf on both axles while it is off):
 *   e_f = max(min(F_fx, rho_f Pf), -(rho_f Pf));  e_r likewise         the demands clipped at the STATIC caps
 *   w = c_h (e_f + e_r);  w = max(min(w, w_max), -w_max)               the load moved to the rear (negative: braking)
 *   x_f = -w;  x_r = w;  phi_a = 1 + x_a (a1_a + a2_a x_a);  Pf' = Pf phi_f;  Pr' = Pr phi_r
 * then the side forces with Pf', Pr' in front of the unchanged Pacejka shape, and the coupling block on the original F_fx,
 * F_rx with Pf', Pr' in place of Pf, Pr.  One explicit pass at the algebraic loop between force and load: no carried state.
 * h_cg = 0 and pedal == 0 give the step without the setting bit for bit (for finite forces).  The friction map is left out
 * of w.  acmpc_score_grips applies vehicle 0's factors to each hypothesis' own peaks.  The setting belongs to the handle: it
 * survives every other acmpc_set_dynamics* call, and every call form of mode D takes it from the handle.  While it is on,
 * every vehicle of the handle must have N_a != 0, phi_a > 0 (in float64) at x = +-w_max and at the vertex -a1_a / (2 a2_a)
 * where a2_a > 0 and the vertex lies inside, and Pf, Pr finite and > 0 as float32: whichever call would break that - this
 * one, acmpc_set_dynamics or acmpc_set_dynamics_ensemble - returns ACMPC_EINVAL and leaves the handle as it was.  No device
 * work.  ACMPC_ESTATE for a handle whose mode is not ACMPC_MODE_DYNAMIC; ACMPC_EINVAL for an h_cg that is negative or not
 * finite, or a w_frac outside (0, 1).  DESIGN.md section 2 "Mode D, load transfer". */
int acmpc_set_dynamics_load_transfer(acmpc_ctx* ctx, const double setting[2] /* NULL: off */);

/* Mode D's aerodynamic downforce: each axle's load, and with it its Pacejka peak factor and its coupling cap, grows with the
 * square of the speed.  Off by default, when the axle loads are the static weights at every speed.  setting = (k_f, k_r,
 * v_sat): k_f, k_r >= 0 and finite as float32, the downforce on the front and the rear axle per vx^2 in the vehicle block's
 * force unit per (m/s)^2; v_sat > 0 and finite, the speed at which the downforce stops growing (vx is unbounded in a rollout
 * and the peak factor must stay positive: the load range it is checked over has to be closed); each of the three is rounded to
 * float32 once; NULL turns the setting off.  Per vehicle the host derives a1_a, a2_a as acmpc_set_dynamics_load_transfer does
 * (they do not depend on h_cg); c_h = w_max = 0 while the load transfer is off.  In every Euler step (every sub-step), after
 * the two longitudinal forces and before anything uses a peak, all float32, nothing fused, min / max the IEEE minNum / maxNum,
 * vx the step's incoming speed, Pf, Pr the peaks the step would otherwise use, rho the coupling's ratios (+inf while it is off):
 *   va = min(vx, v_sat);  q = va va;  d_f = k_f q;  d_r = k_r q            the downforce: it depends on the state alone
 *   psi_a = 1 + d_a (a1_a + a2_a d_a);  Pf0 = Pf psi_f;  Pr0 = Pr psi_r     the peaks at this speed before any tyre force
 *   e_f = max(min(F_fx, rho_f Pf0), -(rho_f Pf0));  e_r likewise            the demands clipped at the caps AT THIS SPEED
 *   w = c_h (e_f + e_r);  w = max(min(w, w_max), -w_max)
 *   x_f = d_f - w;  x_r = d_r + w;  phi_a = 1 + x_a (a1_a + a2_a x_a);  Pf' = Pf phi_f;  Pr' = Pr phi_r
 * then exactly the step of the load transfer: the side forces with Pf', Pr', the coupling block on the original F_fx, F_rx
 * with Pf', Pr'.  The drag stays in the friction map; the step carries no new state.  k_f = k_r = 0, and vx = 0 within one
 * sub-step, give the step without the setting bit for bit (for finite forces); above v_sat the peaks are those at v_sat; a NaN
 * vx takes va = v_sat.  acmpc_score_grips applies the setting and vehicle 0's factors to each hypothesis' own peaks.  The
 * setting belongs to the handle: it survives every other acmpc_set_dynamics* call and acmpc_set_obstacles, and every call
 * form of mode D takes it from the handle.  While it is on, every vehicle of the handle must have N_a != 0 and finite, Pf, Pr
 * finite and > 0 as float32, and 1 + x (a1_a + a2_a x) > 0 (in float64) at x = -w_max, at x = w_max + k_a v_sat^2 and at the
 * vertex -a1_a / (2 a2_a) when that lies strictly between the two, whatever the sign of a2_a: whichever call would break that
 * - this one, acmpc_set_dynamics_load_transfer, acmpc_set_dynamics or acmpc_set_dynamics_ensemble - returns ACMPC_EINVAL and
 * leaves the handle as it was.  No device work.  ACMPC_ESTATE for a handle whose mode is not ACMPC_MODE_DYNAMIC; ACMPC_EINVAL
 * for a k that is negative or not finite, or a v_sat that is not finite and > 0.  DESIGN.md section 2 "Mode D, downforce". */
int acmpc_set_dynamics_downforce(acmpc_ctx* ctx, const double setting[3] /* NULL: off */);

/* The control applied just before each problem's plan starts: u_prev host [P][2] = (delta, pedal), what step 0's rates
 * are taken against; NULL clears it (P is then ignored), and step 0's own control stands for it: an increment of +0.
 * Staged on the host; it travels to the device with the tables, on the next call's stream (acmpc_sync_tables covers it),
 * and stays until replaced or cleared.  Every round of acmpc_optimize uses the same one.  Not read while the rate part
 * of acmpc_set_dynamics_terms is off.  The values are not checked: a NaN makes step 0's rate NaN.  ACMPC_EINVAL for a
 * handle whose mode is not ACMPC_MODE_DYNAMIC or P outside 1 .. max_problems; a later mode D call whose P is not the
 * stored one returns ACMPC_ESTATE. */
int acmpc_set_previous_control(acmpc_ctx* ctx, const float* u_prev, int32_t P);

/* Mode D, moving obstacles: up to ACMPC_MAX_OBSTACLES discs per problem that the candidates are to keep clear of, each with a
 * position per control step.  positions host [P][n][K][2] in the caller's frame: row i is where disc k is at the state AFTER
 * control step i (time (i + 1) dt), the state that step's cost sees.  radii host [P][K]: the obstacle's radius plus the ego's -
 * the ego is one disc at the state's (X, Y).  positions == NULL or K == 0 clears the data (the other arguments are then
 * ignored).  Per control step, after that step's cost and after the rate, slip and ceiling lines where those are on, for
 * k = 0 .. K - 1 in that order, all float32, nothing fused but the named FMAs, max the IEEE maxNum, sqrt correctly rounded:
 *   ox = o_x[i][k] - x_0;  oy = o_y[i][k] - y_0           (x_0, y_0): the first waypoint of the problem's packed rows
 *   dx = X - ox;  dy = Y - oy;  d = sqrt(fma(dy, dy, dx dx))
 *   h = max(R_k - d, 0);           V = fma(h, h, V)              hard: the penetration depth, like the corridor hinge
 *   g = max((R_k + mg) - d, 0);    E = fma(hwo g, g, E)          soft: only with a weight (acmpc_set_dynamics_clearance)
 * The hard part is on while obstacles are set, the soft part while they are set and the clearance weight is not 0; the cost's
 * stage = stage + E is executed when the rate, the slip or the soft part is on.  A NaN or infinite coordinate gives h = g = 0:
 * disc k does not exist at step i.  R_k = 0 never violates.  Under an ensemble every vehicle's cost and violation carry the
 * lines with that vehicle's own trajectory.  acmpc_score_grips does not read obstacles.  Staged on the host; the data travels
 * to the device with the tables, on the next call's stream (acmpc_sync_tables covers it), and stays until replaced or
 * cleared.  The positions are not checked.  No device work.  ACMPC_ESTATE for a handle whose mode is not ACMPC_MODE_DYNAMIC;
 * ACMPC_EINVAL for K outside 0 .. ACMPC_MAX_OBSTACLES, P outside 1 .. max_problems, n outside 1 .. max_steps, a NULL radii or
 * a radius that is negative or not finite - the handle then keeps what it had; a later mode D call whose P or n is not the
 * stored one returns ACMPC_ESTATE.  DESIGN.md section 2 "Mode D, obstacles". */
#define ACMPC_MAX_OBSTACLES 8
int acmpc_set_obstacles(acmpc_ctx* ctx, const float* positions, const float* radii, int32_t P, int32_t n, int32_t K);

/* Mode D, the soft part of the obstacles' lines: hwo = 0.5f float32(weight) (an exact product), mg = float32(margin), each
 * double rounded to float32 once.  (0, 0) by default: the soft part is off.  The setting belongs to the handle: it survives
 * every other acmpc_set_dynamics* call and acmpc_set_obstacles.  No device work.  ACMPC_ESTATE for a handle whose mode is not
 * ACMPC_MODE_DYNAMIC; ACMPC_EINVAL for a weight or margin that is negative or not finite (as a float32) - the handle then
 * keeps its previous setting. */
int acmpc_set_dynamics_clearance(acmpc_ctx* ctx, double weight, double margin);

/* Mode D, surface: a grip map along the path.  grip host [P][n][2] float32 (mu_f, mu_r): row m scales the front and the rear
 * axle's peak factor at waypoint m of problem p's path (P and n those of acmpc_set_paths).  NULL clears the setting (the other
 * arguments are then ignored).  With j_i the nearest waypoint that control step i's cost used and j_{-1} = 0 (the path is cut at
 * the car, and the windowed search starts from 0 as well), control step i of a candidate runs all of its sub-steps on
 *   Pf_s = Pf mu_f[j_{i-1}];   Pr_s = Pr mu_r[j_{i-1}]        one float32 multiply each, once per control step
 * with Pf, Pr the peaks the step would otherwise start from (the vehicle's, or each ensemble member's own; every vehicle follows
 * its own trajectory's j, the table is shared).  THE SCALE LAGS THE POSITION BY ONE CONTROL STEP: step i is driven on the grip of
 * where step i - 1 ended.  Pf_s, Pr_s stand wherever the step reads the peaks - the downforce's psi, the caps, the loaded peaks,
 * the Pacejka factor; B, C, E and the load transfer's a1, a2 are untouched.  The step under the setting is the top-tier step
 * (the downforce's), whatever else the handle has on; a tier that is off gets its neutral value - rho = +inf (coupling), c_h =
 * w_max = 0 (load transfer), k_f = k_r = 0 with a finite v_sat (downforce) - which gives the lower tiers' bits for finite forces.
 * Costs, violations, keys, records and the softmin are otherwise untouched; the finalize's re-roll and acmpc_trace_plans run the
 * same step (in a trace, slot 0 of the previous row names the waypoint whose scale a step used).  acmpc_score_grips does not read
 * the table: a log has no pose.  Staged on the host; the table travels to the device with the tables, on the next call's stream
 * (acmpc_sync_tables covers it), and stays until replaced or cleared; it survives every acmpc_set_dynamics* call and
 * acmpc_set_obstacles.  No device work.  ACMPC_ESTATE for a handle whose mode is not ACMPC_MODE_DYNAMIC; ACMPC_EINVAL for P
 * outside 1 .. max_problems, n outside 1 .. max_steps or a value that is not finite and > 0 - the handle then keeps what it had; a
 * later mode D call (acmpc_trace_plans included) whose P or n is not the stored one returns ACMPC_ESTATE.  DESIGN.md section 2
 * "Mode D, surface". */
int acmpc_set_surface(acmpc_ctx* ctx, const float* grip /* [P][n][2], NULL: off */, int32_t P, int32_t n);

/* Mode D, road: grade and banking along the path.  road host [P][n][3] float32 (a_x, a_y, n_z): row m is the road at waypoint m of
 * problem p's path (P and n those of acmpc_set_paths) - a_x gravity's acceleration along the body's forward axis in m/s^2
 * (downhill positive), a_y along the body's left axis (positive where the road falls to the left: banked for a left-hand
 * corner), n_z > 0 the factor on the normal load.  With theta the grade (uphill positive) and beta the bank (left side lower
 * positive): a_x = -g sin theta, a_y = g cos theta sin beta, n_z = cos theta cos beta; the caller derives them (no trigonometry
 * here: an ensemble's vehicles and a replaced vehicle keep the table valid).  NULL clears the setting (the other arguments are
 * then ignored).  With j_i the nearest waypoint that control step i's cost used and j_{-1} = 0 - the surface table's lag, THE ROW
 * LAGS THE POSITION BY ONE CONTROL STEP - control step i of a candidate runs all of its sub-steps on
 *   Pf_r = Pf_s n_z[j_{i-1}];   Pr_r = Pr_s n_z[j_{i-1}]        one float32 multiply each, once per control step
 * with Pf_s, Pr_s the peaks under the surface table (acmpc_set_surface; the vehicle's own while none is set), and adds, in every
 * Euler sub-step, after xd3 and xd4 are formed and before the multiply by the step,
 *   xd3 = xd3 + a_x[j_{i-1}];   xd4 = xd4 + a_y[j_{i-1}]        one float32 add each
 * Pf_r, Pr_r stand wherever the step reads the peaks - the downforce's psi, the caps, the loaded peaks, the Pacejka factor.
 * Nothing else of the step changes: the kinematic blend, F_fric, the vx >= 0 clip and xd5 are as they are; gravity is applied
 * along the body axes (not rotated by the heading error), the peak scales linearly with n_z, and a_x does not enter the load
 * transfer.  The step under the setting is the top-tier step, as under acmpc_set_surface (a tier that is off at its neutral
 * value).  Costs, violations, keys, records, the softmin and the sampler are otherwise untouched; the finalize's re-roll and
 * acmpc_trace_plans run the same step (in a trace, slot 0 of the previous row names the waypoint whose row a step used).
 * acmpc_score_grips does not read the table.  Staged on the host; the table travels to the device with the tables, on the next
 * call's stream (acmpc_sync_tables covers it), and stays until replaced or cleared; it survives every acmpc_set_dynamics* call,
 * acmpc_set_obstacles, acmpc_set_surface and the actuator setters.  No device work.  ACMPC_ESTATE for a handle whose mode is not
 * ACMPC_MODE_DYNAMIC; ACMPC_EINVAL for P outside 1 .. max_problems, n outside 1 .. max_steps, a value that is not finite or an
 * n_z <= 0 - the handle then keeps what it had; a later mode D call (acmpc_trace_plans included) whose P or n is not the stored
 * one returns ACMPC_ESTATE.  DESIGN.md section 2 "Mode D, road". */
int acmpc_set_road(acmpc_ctx* ctx, const float* road /* [P][n][3], NULL: off */, int32_t P, int32_t n);

/* Mode D, actuator lag: the steering rack and the pedal actuator follow their commands as first-order lags.  tau host [2] =
 * (tau_d, tau_p) in seconds for the steering and the pedal channel, each finite and >= 0; NULL turns the setting off.  With dt
 * the handle's control step the host derives per channel, in float64, each rounded to float32 once
 *   k_c = exp(-dt / tau_c)            what is left of an error after one control step      (tau_c = 0: k_c = 0)
 *   m_c = (tau_c / dt) (1 - k_c)      the mean of what is left over the step's interval    (tau_c = 0: m_c = 0)
 * so that 0 < k_c < m_c < 1 for tau_c > 0.  A candidate carries the two actuator positions (a_d, a_p).  At the top of control
 * step i, before anything of the step runs, in float32 and with nothing fused (the pedal channel likewise with k_p, m_p, a_p):
 *   e       = delta_i - a_d
 *   delta_x = delta_i - m_d e         what the vehicle is driven on during step i: the interval mean of the exact first-order
 *                                     response to a held command
 *   a_d     = delta_i - k_d e         the position at the end of the step (the exact zero-order-hold discretisation)
 * The control step reads the APPLIED control (delta_x, pedal_x) and nothing else of the command: the control's terms, all M
 * sub-steps and the low-speed blend's tan(delta); the update happens once per control step, not per sub-step.  The COMMAND
 * (delta_i, pedal_i) stays what the cost's input box and dk, the rate terms (step 0 against acmpc_set_previous_control as ever),
 * the records' u, the softmin mean, the keys and the sampler see: what the optimiser chooses and what the caller sends.  Every
 * vehicle of an ensemble carries the same filter.  The step under the setting is the top-tier step (the downforce's, or the
 * surface's while a table is set), whatever else the handle has on; a tier that is off gets its neutral value as under
 * acmpc_set_surface.  tau = (0, 0) is ON with k = m = 0: the applied control equals the command (up to the sign of a zero), not
 * the same as off.  The finalize's re-roll and acmpc_trace_plans run the same step (a trace's slots 4 to 6 and 8 to 9 are on the
 * command; its states are the lagged trajectory).  acmpc_score_grips does NOT apply the setting: a log should hold the measured
 * actuator positions as its controls.  A pure dead time is not modelled: roll the start state forward under the controls
 * already sent.  The setting belongs to the handle and survives every other acmpc_set_dynamics* call, acmpc_set_obstacles and
 * acmpc_set_surface.  No device work.  ACMPC_ESTATE for a handle whose mode is not ACMPC_MODE_DYNAMIC; ACMPC_EINVAL for a tau
 * that is negative or not finite - the handle then keeps what it had.  DESIGN.md section 2 "Mode D, actuator". */
int acmpc_set_dynamics_actuator(acmpc_ctx* ctx, const double tau[2] /* NULL: off */);

/* Mode D, actuator lag: the measured actuator positions at the start of the plan, a0 host [P][2] float32 = (a_d, a_p) per
 * problem; NULL clears them (P is then ignored).  While cleared, step 0's own command stands for them: e = +0 and the first step
 * has no lag - the convention of a null previous control.  Values are not checked.  Staged on the host; they travel to the
 * device with the tables, on the next call's stream (acmpc_sync_tables covers it), as the previous control does, and stay until
 * replaced or cleared.  Not read while acmpc_set_dynamics_actuator is off.  ACMPC_ESTATE for a handle whose mode is not
 * ACMPC_MODE_DYNAMIC; ACMPC_EINVAL for P outside 1 .. max_problems; a later mode D call (acmpc_trace_plans included) with another
 * P returns ACMPC_ESTATE. */
int acmpc_set_actuator_state(acmpc_ctx* ctx, const float* a0 /* [P][2], NULL: clear */, int32_t P);

/* Mode D, grip identification: which vehicle did a logged stretch of driving come from?  K hypotheses - the handle's
 * vehicle 0 (the block of acmpc_set_dynamics, or member 0 of acmpc_set_dynamics_ensemble) with Df scales[k][0] and
 * Dr scales[k][1], derived as every block is (the two peaks in float64, rounded once; everything else vehicle 0's own
 * floats, so scales (1, 1) is vehicle 0 bit for bit) - are rolled over the log and scored by their prediction error.
 *   states    host [W + 1][3] float32 (vx, vy, r); controls host [W][2] float32 (delta, pedal), 1 <= W <=
 *             ACMPC_MAX_LOG_STEPS; control j was applied between state j and state j + 1 (no pose: the velocity rows of
 *             the step do not read it)
 *   dt        the LOG's period (need not be the handle's): a control step is the handle's integration setting (M, blend)
 *             with h = float32(dt / M)
 *   segment   L in 1 .. W: segment s covers steps [s L, min((s + 1) L, W)), starts from the LOGGED state s L, rolls
 *             open-loop under the logged controls and adds, after every control step j,
 *             weights[0] dvx^2 + weights[1] dvy^2 + weights[2] dr^2 of (rolled - logged state j + 1); L = 1: one-step-ahead
 *             residuals, L = W: one open-loop roll
 *   errors    [K] (or NULL): E_k = the segments' sums added in segment order (float32); a NaN or inf in the log makes E_k
 *             NaN or inf
 *   best      min_k acmpc_pack_key(E_k, k): ties go to the lower index, non-finite errors rank last
 * Host pointers; the call blocks and makes one round trip.  It changes nothing a later solve reads.  Refused before any
 * device work: ACMPC_EINVAL for a null pointer (errors may be), W, K < 1 or segment out of range, dt not finite and
 * positive, a scale that is not finite and > 0, a weight that is not finite and >= 0 (as a float32), or all weights 0;
 * ACMPC_ESTATE for a handle that is not mode D or has no vehicle, or while a batch of acmpc_solve_stream_device is
 * pending; ACMPC_ECAPACITY for K > ACMPC_MAX_GRIP_HYPOTHESES or ceil(W / segment) K > 2^22.  DESIGN.md section 2 "Mode D,
 * grip identification". */
#define ACMPC_MAX_LOG_STEPS 512
#define ACMPC_MAX_GRIP_HYPOTHESES 65536
int acmpc_score_grips(acmpc_ctx* ctx, const float* states, const float* controls, int32_t W, double dt, int32_t segment,
                      const double weights[3], const double* scales /* [K][2] front, rear */, int32_t K,
                      float* errors /* [K] or NULL */, int64_t* best);

/* Mode D, plan trace: what does a plan do, step by step, under every vehicle of the handle?  M plans per problem are
 * re-rolled from x0 with ALL of the handle's settings - paths (acmpc_set_paths: n must be theirs), vehicle or ensemble,
 * integration, terms, previous control, objective, coupling, load transfer, downforce, obstacles and clearance - by the
 * arithmetic of the kernels that score candidates, one wavefront per (problem, plan, vehicle), and every control step
 * leaves what it saw.  K = the handle's vehicles (1 after acmpc_set_dynamics).
 *   x0      host [P][6] float32 (X, Y, yaw, vx, vy, r);  U host [P][M][n][2] float32 (delta, pedal)
 *   states  [P][M][K][n + 1][6] float32 (X, Y, yaw, vx, vy, r): row 0 the start, row i + 1 the state after control step i,
 *           positions in the caller's frame (a record's x is columns 0 .. 2 of vehicle 0)
 *   totals  [P][M][K][2] float32 (c_k, V_k): vehicle k's cost and violation of that plan, before the ensemble's reduction
 *   terms   [P][M][K][n][ACMPC_TRACE_TERM_FLOATS] float32, one row per control step on the state that step's cost saw:
 *             0        the nearest waypoint j (as a float: exact)
 *             1, 2     e_y, e_psi                    3, 4   dv = vx - v_ref_j, dk = delta - delta_ref_j
 *             5, 6     the input box: u - med3(u, lo, hi) of steering and of pedal (signed)
 *             7        the corridor: max(|e_y| - half-width_j, 0)
 *             8, 9     the rate limits of steering and pedal     10   the slip limit     11   the speed ceiling
 *             12 .. 19 disc q's penetration depth, q < the obstacles' K; +0 beyond
 *             20       V after this step                         21   E after this step (+0 without terms)
 *           Slots 5 .. 19 are the float32 hinges the cost squares into V, a part that is off leaves +0: from the previous
 *           step's slot 20 (+0 at step 0), V = fma(h, h, V) over slots 5, 6, .., 19 in that order gives this step's slot 20
 *           bit for bit, and the last step's is V_k.  A plan is infeasible exactly where a slot of 5 .. 19 is not 0.
 * Any of the three outputs may be NULL (not all).  Host pointers; the call blocks and makes one round trip on the handle's
 * stream, the inputs travelling with the tables as in acmpc_optimize.  Its device scratch is the call's own, kept between
 * calls and regrown when a later call needs more.  It changes nothing a later call reads.  Refused before any device work,
 * the handle as it was: ACMPC_ESTATE for a handle that is not mode D, has no vehicle or no paths, whose stored previous
 * controls or obstacles are of another shape, or while a batch of acmpc_solve_stream_device is pending; ACMPC_EINVAL for a
 * null x0 or U, three null outputs, P, M or n below 1, or P, n other than the paths'; ACMPC_ECAPACITY for P or n beyond the
 * handle's, or outputs beyond 1 GiB in all.  DESIGN.md section 2 "Mode D, plan trace". */
#define ACMPC_TRACE_TERM_FLOATS 22
int acmpc_trace_plans(acmpc_ctx* ctx, const float* x0, const float* U, int32_t P, int32_t M, int32_t n, float* states,
                      float* totals, float* terms);

/* Copies the packed float32 table of problem `problem` (n rows of ACMPC_COEF_STRIDE_* floats) to `out`.
 * Host only; lets CPU tests pin the host-side arithmetic against the oracle. */
int acmpc_get_coefficients(const acmpc_ctx* ctx, int32_t problem, float* out, int32_t capacity_floats);

/* Mode D: copies the progress table of problem `problem` (n floats) to `out`.  Derived from the packed float32 rows
 * (x_m, y_m, c_m = cos psi_m, s_m = sin psi_m) whenever acmpc_set_paths or acmpc_set_coefficients change them, in float64
 * in the order written, no fused multiply-add:
 *   S_0 = 0,  S_m = S_{m-1} + sqrt(dx dx + dy dy),  q_m = float32(S_m - (c_m (x_m - x_0) + s_m (y_m - y_0))).
 * Host only, like acmpc_get_coefficients.  ACMPC_ESTATE for a handle that is not mode D or has no paths. */
int acmpc_get_progress_table(const acmpc_ctx* ctx, int32_t problem, float* out, int32_t capacity_floats);

/* Floats in one winner record: ACMPC_REC_HEADER + 2 n + 3 (n + 1) =
 *   [cost, violation, n_feasible, owner, u_0 .. u_{n-1} (2 each), x_0 .. x_n (3 each)]
 * x is (e_y, e_psi, t) in mode S and (X, Y, phi) in modes T and D (u = (delta, pedal) in mode D).  The u / x blocks are what
 * spatial_mpc.py:193-202 slices out of OSQP's dec.x ([x_0..x_n ; u_0..u_{n-1}], control.py:121-158). */
int32_t acmpc_record_floats(int32_t n);

/* Replaces: ControlSolver.solve (control.py:15-24) for host-resident inputs - one blocking call doing H2D,
 * rollout + cost + argmin, and D2H.
 *   x0        [P][3]   mode S: t2s(...) output (e_y, e_psi, t) (dynamics.py:23-40); mode T: pose (X, Y, phi);
 *             [P][6]   mode D: (X, Y, yaw, vx, vy, r)
 *   U         control-sample matrix in `layout`
 *   costs     [P][N] or NULL
 *   best_idx  [P] index of the cheapest candidate (lowest index on ties; non-finite costs rank last)
 *   records   [P][acmpc_record_floats(n)] or NULL
 */
int acmpc_solve(acmpc_ctx* ctx, const float* x0, const float* U, int32_t P, int32_t N, int32_t n,
                int32_t layout, float* costs, int32_t* best_idx, float* records);

/* Page-locked host memory for acmpc_solve's control matrix.  A matrix in ordinary (pageable) memory is staged into
 * device memory by a copy in front of the rollout (~40 us for the 1.6 MB of 4 096 candidates x horizon 50); one built in
 * memory these calls return is READ IN PLACE by the rollout, which streams it over the host link while it computes - a
 * 4 096-candidate solve 58 us instead of 74 (measured through the Python wrapper, tools/archive/time_host_solve.py).  Start states,
 * keys and records of a one-launch solve never travel as copies of their own either way: the kernels read and write them
 * in the handle's page-locked block.  acmpc_host_alloc initialises the HIP runtime: call it in the process that solves
 * (after the fork of controller.py:94-100), never before.  The closed loop does not need it: acmpc_control_tick samples
 * on the device and moves 2 kB per tick. */
int acmpc_host_alloc(void** out, uint64_t bytes);
int acmpc_host_free(void* memory);

/* Same work with every buffer already resident in device memory, asynchronous on `stream`
 * (a hipStream_t, NULL = the null stream).  `d_keys` [P] receives the packed (cost, index) keys - see
 * acmpc_rollout_device - and `d_records` [P][acmpc_record_floats(n)] the winner records.
 * Device buffers are what hipMalloc returns, or views into it on their element type's boundary (gfx950 serves a
 * 16-byte load on any 4-byte boundary); buffers that start 16-byte aligned are served fastest - e.g. a candidate-major
 * `d_U` then takes the faster of the two tile kernels, any other start the slower one, with the same results.
 * One exception, refused with ACMPC_EINVAL before any device work: a step-major launch that gives a lane two or four
 * adjacent candidates (modes S and T; acmpc_describe_rollout out[1]) reads their controls and writes their costs as one
 * 8- or 16-byte vector, so there `d_U` and `d_costs` must start on an 8- / 16-byte boundary (N is then a multiple of two /
 * four, so every row of the matrix does too).  This holds for every call that takes a step-major `d_U`:
 * acmpc_solve_device, acmpc_rollout_device, acmpc_solve_sampled_device, acmpc_solve_stream_device, and acmpc_solve on a
 * matrix it reads in place.  What hipMalloc returns always qualifies. */
int acmpc_solve_device(acmpc_ctx* ctx, const float* d_x0, const float* d_U, int32_t P, int32_t N, int32_t n,
                       int32_t layout, float* d_costs, int64_t* d_keys, float* d_records, void* stream);

/* Sharded form: each rank rolls out its own N candidates whose global indices start at
 * `index_offset`, and gets per-problem keys
 *     key = (ordered_int32(cost) << 32) | uint32(global index)
 * that order like (cost, index) under signed 64-bit comparison, so ONE RCCL all-reduce(MIN) over `d_keys`
 * yields the global argmin with lowest-index tie-breaking.  acmpc_finalize_device then writes the winner's
 * record on the rank that owns it and zeros elsewhere (owner flag 0), plus every rank's feasible count, so an
 * all-reduce(SUM) of the records gives every rank the selected controls.
 * `d_keys` may be NULL in both calls on a single GPU: the rollout then leaves its per-workgroup partial keys in
 * the handle and the finalize step reduces those itself (two launches in total; acmpc_solve_device does the same
 * work in ONE launch for mode S problems of up to 65 536 candidates in all, and in these two launches otherwise). */
int acmpc_rollout_device(acmpc_ctx* ctx, const float* d_x0, const float* d_U, int32_t P, int32_t N, int32_t n,
                         int32_t layout, int64_t index_offset, float* d_costs, int64_t* d_keys, void* stream);
int acmpc_finalize_device(acmpc_ctx* ctx, const int64_t* d_keys, const float* d_x0, const float* d_U, int32_t P,
                          int32_t N, int32_t n, int32_t layout, int64_t index_offset, float* d_records,
                          void* stream);

/* Softmin-weighted mean control sequence, sum_c w_c U_c / sum_c w_c with w_c = exp(-(cost_c - min)/lambda)
 * (the weighted-reduction form of localiser.py:572-579).  `d_costs` [P][N] and `d_keys` [P] come from a
 * previous rollout; `d_mean` [P][n][2] (float32), `d_weight_sum` [P] (float64) or NULL.  Partial sums are
 * combined in a fixed order: results are bitwise reproducible. */
int acmpc_softmin_device(acmpc_ctx* ctx, const float* d_costs, const int64_t* d_keys, const float* d_U,
                         int32_t P, int32_t N, int32_t n, int32_t layout, float* d_mean, double* d_weight_sum,
                         void* stream);

/* Uploads pending tables now (otherwise done by the next device call) and blocks until resident, so that a
 * timed region contains no host-to-device traffic. */
int acmpc_sync_tables(acmpc_ctx* ctx, void* stream);

/* On-device candidate generation.  Candidate c of problem p is
 *     U_c = clip(centre_p + a_c * (sigma_v, sigma_kappa) * smooth_noise_c, input box),   a_c = ((c mod 8) + 1) / 8,
 * smooth_noise = raised-cosine blend along the horizon of 8 x 2 standard normals drawn with Philox4x32-10 at
 * counter (global candidate index, problem, round, draw) and key = seed, so every rank regenerates the same
 * candidate from its index alone.  Candidate 0 is the centre itself, candidate 1 is `d_u_ref` when given.
 * `d_centre` holds P rows of `centre_stride` floats whose first 2n are (v, kappa) per step - the u block of a
 * winner record qualifies (centre_stride = acmpc_record_floats(n), pointer = records + ACMPC_REC_HEADER). */
int acmpc_sample_device(acmpc_ctx* ctx, const float* d_centre, int32_t centre_stride, const float* d_u_ref,
                        int32_t P, int32_t N, int32_t n, int32_t layout, int64_t index_offset, double sigma_v,
                        double sigma_kappa, uint64_t seed, uint32_t round, float* d_U, void* stream);

/* Finalize for sampled candidates: the winner's controls are re-drawn from the global index in its key (same
 * arithmetic as acmpc_sample_device, bit-identical), so after ONE all-reduce(MIN) of `d_keys` every rank writes
 * the complete winner record itself - no second collective, no owner.  `d_keys` may be NULL on a single GPU
 * (the handle's partial keys of the preceding rollout are reduced instead).  n_feasible in the record is this
 * rank's count.  Arguments after `d_x0` must be those the candidates were sampled with. */
int acmpc_finalize_sampled_device(acmpc_ctx* ctx, const int64_t* d_keys, const float* d_x0, const float* d_centre,
                                  int32_t centre_stride, const float* d_u_ref, int32_t P, int32_t N, int32_t n,
                                  double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round,
                                  float* d_records, void* stream);

/* acmpc_rollout_device + acmpc_finalize_sampled_device as ONE call for a rank that has all the candidates (no all-reduce
 * between them): `d_U` holds what acmpc_sample_device wrote for (centre, u_ref, sigma, seed, round); rollout, argmin and
 * the winners' records - re-drawn from their indices - without a host round trip between them: two launches, or with
 * the handle's ACMPC_TAILED_ROLLOUT option one (mode S, step-major: the last workgroup of every problem finalizes it,
 * csrc/acmpc_kernels.hip rollout_tailed_kernel - measured slower on the headline's batch, so not the default).
 * d_costs [P][N] or NULL, d_keys [P] or NULL, d_records [P][acmpc_record_floats(n)].  The same bits either way. */
int acmpc_solve_sampled_device(acmpc_ctx* ctx, const float* d_x0, const float* d_U, const float* d_centre,
                               int32_t centre_stride, const float* d_u_ref, int32_t P, int32_t N, int32_t n, int32_t layout,
                               double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round, float* d_costs,
                               int64_t* d_keys, float* d_records, void* stream);

/* Mode D only: acmpc_sample_device into a matrix + acmpc_rollout_device of it WITHOUT the matrix - every lane draws its
 * candidate (global index index_offset + c: the same candidate as acmpc_sample_device's, bit for bit) inside the rollout
 * kernel and blends each step's control as it goes (csrc/acmpc_dynamic_kernels.h rollout_dynamic_sampled_kernel).  d_x0 [P][6];
 * d_centre / centre_stride / d_u_ref / sigma_v, sigma_kappa (= sigma_delta, sigma_pedal) / seed / round as
 * acmpc_sample_device takes them; d_costs [P][N] or NULL and d_keys [P] or NULL as acmpc_rollout_device leaves them - the
 * same bits.  Follow it with acmpc_finalize_sampled_device (after acmpc_reduce_across_ranks when the candidates are spread
 * over ranks).  ACMPC_ESTATE on a mode S or mode T handle (their rounds draw inside acmpc_optimize), and without a vehicle or
 * paths; ACMPC_EINVAL for a null pointer, ACMPC_ECAPACITY for a shape beyond the handle's - all before any device work. */
int acmpc_rollout_sampled_device(acmpc_ctx* ctx, const float* d_x0, const float* d_centre, int32_t centre_stride,
                                 const float* d_u_ref, int32_t P, int32_t N, int32_t n, int64_t index_offset,
                                 double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round, float* d_costs,
                                 int64_t* d_keys, void* stream);

/* acmpc_sample_device (step-major) into a matrix + acmpc_softmin_device of it WITHOUT the matrix: the softmin kernel re-draws
 * candidate index_offset + c from its global index (the same candidate as acmpc_sample_device's, bit for bit; global
 * candidate 0 = the centre, 1 = d_u_ref when given) and sums in the matrix kernel's order, so d_mean [P][n][2] and
 * d_weight_sum [P] (or NULL) are the same bits (csrc/acmpc_softmin.hip softmin_sampled_partial_kernel).  d_costs [P][N] and
 * d_keys [P] come from the rollout of those candidates (acmpc_rollout_sampled_device in mode D; d_keys after
 * acmpc_reduce_across_ranks when the candidates are spread over ranks: the weights are relative to the GLOBAL minimum);
 * d_centre / centre_stride / d_u_ref / sigma / seed / round as acmpc_sample_device takes them.  The sampler is the same in
 * every mode: accepted on mode S, T and D handles.  ACMPC_EINVAL for a null pointer, centre_stride < 2 n, a global index
 * beyond 32 bits or softmin_lambda <= 0, ACMPC_ECAPACITY for a shape beyond the handle's - all before any device work. */
int acmpc_softmin_sampled_device(acmpc_ctx* ctx, const float* d_costs, const int64_t* d_keys, const float* d_centre,
                                 int32_t centre_stride, const float* d_u_ref, int32_t P, int32_t N, int32_t n,
                                 int64_t index_offset, double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round,
                                 float* d_mean, double* d_weight_sum, void* stream);

/* A STREAM of batches on one rank: acmpc_solve_device (d_centre NULL: the winners are read from d_U) or
 * acmpc_solve_sampled_device (d_centre given: re-drawn) with the argmin and the winners' records of one call DEFERRED -
 * they are computed inside the NEXT call's rollout launch (csrc/acmpc_kernels.hip rollout_chained_kernel: one row in
 * every few of the grid finalizes four problems of the previous batch per workgroup while the other rows stream), or by
 * acmpc_solve_stream_flush behind the last one.  Behind the headline's rollout the finalize of 4 096 problems is a launch
 * of its own - 13 us and a launch boundary per 1.0 ms step; inside the next rollout nobody waits for it.
 *   d_keys / d_records of call k are complete once call k + 1 on the same stream, or the flush, has completed;
 *   until then the caller leaves call k's d_x0, d_centre / d_u_ref - and d_U when d_centre is NULL - as they were;
 *   d_costs of call k are complete with call k itself.
 * The same bits as acmpc_solve_device / acmpc_solve_sampled_device (tests/test_gpu_tailed_rollout.py).  Shapes the one
 * launch does not take (mode T, the candidate-major layout, horizons whose finalize would cost the rollout its
 * occupancy) run the pending finalize as a launch of its own in front of the rollout.  While a batch is pending every
 * other solve on the handle returns ACMPC_ESTATE (acmpc_sample_device - drawing the next batch's candidates - is allowed);
 * new tables (acmpc_set_paths) are uploaded behind the pending finalize. */
int acmpc_solve_stream_device(acmpc_ctx* ctx, const float* d_x0, const float* d_U, const float* d_centre,
                              int32_t centre_stride, const float* d_u_ref, int32_t P, int32_t N, int32_t n, int32_t layout,
                              double sigma_v, double sigma_kappa, uint64_t seed, uint32_t round, float* d_costs,
                              int64_t* d_keys, float* d_records, void* stream);
int acmpc_solve_stream_flush(acmpc_ctx* ctx, void* stream);

/* The one collective of the multi-GPU step, for hosts that drive RCCL themselves rather than through
 * torch.distributed: in-place all-reduce(MIN) of the P packed keys over `rccl_comm` (an `ncclComm_t` the host
 * created, one rank per GPU), enqueued on `stream`.  Call between acmpc_rollout_device and
 * acmpc_finalize_sampled_device / acmpc_finalize_device.  RCCL is resolved at the first call: the copy already loaded
 * in the process if there is one (the one that owns `rccl_comm`), else `librccl.so.1` (or $ACMPC_RCCL_LIBRARY);
 * the library itself does not link RCCL.  ACMPC_ESTATE when no RCCL can be found, ACMPC_EHIP when RCCL fails. */
int acmpc_reduce_across_ranks(acmpc_ctx* ctx, void* rccl_comm, int64_t* d_keys, int32_t P, void* stream);
/* A communicator for it out of the same copy of RCCL (a process may hold two - the system's and the one PyTorch bundles -
 * and a communicator only works with the copy that made it): acmpc_rccl_unique_id on ONE rank (ncclGetUniqueId; 128
 * bytes, handed to the others by whatever channel the host has - bench.py uses the torch.distributed store),
 * acmpc_rccl_comm_create on EVERY rank (ncclCommInitRank: collective, returns when all `n_ranks` have called it; `device`
 * >= 0 is made current first, one rank per GPU), acmpc_rccl_comm_destroy at the end.  ACMPC_ESTATE when no RCCL can be
 * found, ACMPC_EHIP when RCCL fails, ACMPC_ENODEVICE for a device that cannot be selected.  No handle. */
#define ACMPC_RCCL_UNIQUE_ID_BYTES 128
int acmpc_rccl_unique_id(void* id_out);
int acmpc_rccl_comm_create(const void* id, int32_t n_ranks, int32_t rank, int32_t device, void** comm_out);
int acmpc_rccl_comm_destroy(void* comm);

/* Replaces: ControlSolver.solve (control.py:15-24) end to end on the device - `rounds` rounds of
 * sample -> rollout + cost -> argmin, each round sampling round the previous winner with the spread shrunk by
 * `shrink`, one host round trip in total (x0, centre, u_ref up; the final records down).  Host pointers:
 * x0 [P][3], centre [P][n][2], u_ref [P][n][2] or NULL, sigma[2], records [P][acmpc_record_floats(n)]. */
int acmpc_optimize(acmpc_ctx* ctx, const float* x0, const float* centre, const float* u_ref, int32_t P, int32_t N,
                   int32_t n, int32_t rounds, const double sigma[2], double shrink, uint64_t seed, float* records);

/* Replaces: the whole of SpatialMPC.get_control (spatial_mpc.py:170-217) for one tick of the control loop, as ONE host
 * round trip: the H x 3 reference path, the constraints and the centre sequence go up in one copy; the device runs
 *   prologue (one wavefront): construct_waypoints (spatial_mpc.py:125-154) -> velocity ceiling + speed-profile QP
 *     (speed_profile.py:26-59, tridiagonal ADMM warm-started from the state the handle keeps on the device) -> t2s
 *     (dynamics.py:23-40) -> linearise + corridor rows (dynamics.py:65-103, control.py:57-60) -> reference controls,
 *   `rounds` rounds of sample -> rollout + cost -> argmin (as acmpc_optimize),
 * all nodes of one captured hipGraph; the winner's record, the 7 x n table and the QP status come back through pinned
 * host memory, and the tail of get_control (acmpc_unpack_decision) runs before the call returns.  Handles with
 * centre_update = 0 and horizon - 1 <= 128 only (ACMPC_ESTATE otherwise: use acmpc_set_paths + acmpc_optimize).
 * Mode T handles (the Cartesian rollout with nearest-waypoint projection, north_star's literal shape) take the same
 * call: the prologue then leaves the pose (offset, 0, pi / 2) as the start state and the [n][8] waypoint rows as the
 * table, the rounds roll them with the handle's search window (nn_back / nn_ahead; exhaustive when nn_ahead < 0) and
 * the plan is unpacked by acmpc_unpack_decision_temporal. */
typedef struct acmpc_tick {
  uint32_t struct_size;        /* sizeof(acmpc_tick)                                                            */
  int32_t horizon;             /* H = rows of `coords`; n = H - 1                                               */
  int32_t localised;           /* != 0: LocalisedSpeedProfileSolver (ceiling = v_max everywhere, no end velocity) */
  int32_t has_end_velocity;    /* != 0: last ceiling entry = end_velocity (speed_profile.py:42-43)              */
  int32_t n_candidates;        /* N per round                                                                   */
  int32_t rounds;
  int32_t centre_is_reference; /* != 0: sample round the reference controls (`centre` is ignored, may be NULL)  */
  int32_t qp_max_iter;         /* speed-profile QP: iteration cap (the reference passes 4000, spatial_mpc.py:17) */
  int32_t qp_check_every;      /* stopping test every this many iterations (<= 0: 10)                           */
  int32_t qp_method;           /* speed-profile QP: 0 = its exact optimum in two passes (acmpc_speed_profile_exact), the
                                  splitting below only where that does not apply (a rate bound of the wrong sign: solved
                                  there; an infeasible or misshapen problem: status 1 after qp_max_iter iterations);
                                  1 = always the OSQP splitting (acmpc_speed_profile_qp), warm-started between ticks    */
  double offset;               /* lateral displacement of the car: pose (offset, 0, pi/2), spatial_mpc.py:187   */
  double v_min, v_max, a_min, a_max, ay_max, ki_min, end_velocity; /* speed_profile_constraints, read every tick */
  double sigma[2];             /* first round's spread of (v, kappa); round r uses sigma * shrink^r             */
  double shrink;
  double qp_eps_abs, qp_eps_rel;
  uint64_t seed;
  /* reference path from the map bound with acmpc_bind_map instead of from `coords` (pass coords = NULL) */
  int32_t map_index;           /* first map waypoint of the look-ahead window; < 0: the map point nearest to the pose  */
  int32_t centreline_points;   /* length of the resampled centre line (500, controller.py:102-108); multiple of horizon */
  double pose_x, pose_y;       /* map frame; read when map_index < 0                                                  */
  double lateral_offset;       /* subtracted from the window's lateral coordinate (the car's offset from the line)    */
} acmpc_tick;

/* Replaces: the path from the map to get_control's argument for a pose on a known map - nearest map
 * point (what the localiser's KD-tree query returns, localiser.py:282-289), the next 150 m of centre line
 * (perception/tracks.py:14) in the vehicle frame, resampled to `centreline_points` float32 points (controller.py:102-108),
 * every (points / H)-th kept with widths linspace(10, 6, H) (ControlProcess._reference_path, controller.py:256-267).
 * acmpc_bind_map copies the centre polyline [M][2] float64 (utils/load.py:9-35 order x, y; `spacing` = metres between map
 * points, mapping/map_maker.py:203); no device work.  acmpc_control_tick with coords = NULL then runs the window kernel
 * in front of the prologue; acmpc_map_reference_path runs it alone (blocking; coords [H][3] out, *first_index out). */
int acmpc_bind_map(acmpc_ctx* ctx, const double* centre, int32_t M, double spacing);
int acmpc_map_reference_path(acmpc_ctx* ctx, int32_t map_index, double pose_x, double pose_y, double lateral_offset,
                             int32_t horizon, int32_t centreline_points, double* coords, int32_t* first_index);

/* coords [H][3] float64 (x, y, width) in the vehicle frame, or NULL with a bound map (then `coords_out` [H][3], if not
 * NULL, receives the path the device built); centre [n][2] float32 (v, kappa) or NULL.
 * Outputs (all required): table [7][n] float64 (rows x, y, psi, kappa, ds, width, v); record
 * [acmpc_record_floats(n)]; decision [5n + 3] = dec.x ([x_0..x_n ; u_0..u_{n-1}], control.py:121-158);
 * projected_control [2][n], prediction [n][2], cum_time [n], times / accelerations / steer_rates [n - 1] as
 * acmpc_unpack_decision writes them; info [8] = {cost, violation, n_feasible, max |dec.x|, QP status (0 = solved,
 * 1 = maximum iterations), QP iterations, first map index of the window or -1, 1 when the cost, the violation or an
 * entry of the plan is not finite (the reference's solver would not report such a solve as solved) else 0}. */
int acmpc_control_tick(acmpc_ctx* ctx, const acmpc_tick* tick, const double* coords, const float* centre, double* table,
                       float* record, double* decision, double* projected_control, double* prediction,
                       double* cum_time, double* times, double* accelerations, double* steer_rates, double* info,
                       double* coords_out);

/* Test hooks of the tick path.  acmpc_tick_read_device_tables copies what the last tick's prologue left on the device
 * for the rollout - x0 [3], u_ref [n][2], the packed table [n][ACMPC_COEF_STRIDE_SPATIAL or _TEMPORAL, by the handle's
 * mode] - back to the host.
 * acmpc_tick_read_device_frames: the frames of the verified nearest-waypoint search the prologue tabulated for that
 * table (mode T handles with the exhaustive search; acmpc_search_frame_floats(n) floats) - the same arithmetic as
 * acmpc_search_frames, run by the prologue's lanes.
 * acmpc_speed_profile_qp_device runs the prologue's ADMM alone on the GPU (host pointers, blocking): same arguments
 * and, bit for bit, the same results as acmpc_speed_profile_qp. */
int acmpc_tick_read_device_tables(acmpc_ctx* ctx, float* x0, float* u_ref, float* coef);
int acmpc_tick_read_device_frames(acmpc_ctx* ctx, float* out, int64_t capacity_floats);
int acmpc_speed_profile_qp_device(acmpc_ctx* ctx, const double* v_hi, const double* ds, int32_t n, double a_min,
                                  double a_max, double v_min, int32_t max_iter, int32_t check_every, double eps_abs,
                                  double eps_rel, double* v, double* y, int32_t warm_start, int32_t* iterations);

/* Test hook of the sampled rounds (modes S and T): which form the rounds of acmpc_optimize(P, N, n) - and of a tick of
 * n + 1 points with N candidates - take on this handle, with its mode, search window and switches.  The answer comes
 * from the functions the launches themselves ask; no device work, the GPU is not initialised.  out[8] =
 *   [0] ACMPC_ROUND_* below: the kernel of a round; -1 when the rounds go through the control matrix (centre_update = 1,
 *       ACMPC_NO_FUSED_SAMPLING)
 *   [1] the last workgroup of a problem finalizes inside the round's launch (else a finalize launch follows)
 *   [2] ... by copying the record out of the winning workgroup's trace (else it re-draws and re-rolls the winner)
 *   [3] rounds before the last are chained: no finalize, the next launch finds the winner
 *   [4] the verified search's frames ride in the round's LDS (acmpc_optimize; a tick's do whenever [7] is set)
 *   [5] acmpc_set_paths tabulates those frames at this n
 *   [6] acmpc_control_tick accepts this n and N
 *   [7] ... and its prologue tabulates the frames
 * ACMPC_ECAPACITY beyond the handle's capacities, ACMPC_ESTATE in mode D. */
#define ACMPC_ROUND_SINGLE 0 /* one wave per workgroup */
#define ACMPC_ROUND_PAIR 1   /* mode S, two waves */
#define ACMPC_ROUND_QUAD 2   /* mode S, four waves */
#define ACMPC_ROUND_TRIO 3   /* mode T, three waves */
int acmpc_describe_rounds(const acmpc_ctx* ctx, int32_t P, int32_t N, int32_t n, int32_t out[8]);

/* Test hook of the rollouts over a caller's control matrix (modes S and T): the launch acmpc_rollout_device,
 * acmpc_solve_device, acmpc_solve_sampled_device, acmpc_solve_stream_device and acmpc_solve make for (P, N, n, layout) on
 * this handle, with its mode and switches (ACMPC_SHAPE, ACMPC_T_PACK, ACMPC_NO_TILE, ACMPC_TILE_ROWS, ACMPC_TILE_TABLE,
 * ACMPC_NO_SOLO).  The answer comes from the functions the launches themselves ask (csrc: choose_shape,
 * tailed_rollout_fits, chained_rollout_fits, tile_rows_table_in_lds, solo_fits); no device work, the GPU is not
 * initialised.  out[8] =
 *   [0] threads per workgroup
 *   [1] candidates per lane (1; step-major also 2 or 4: adjacent candidates, 8- / 16-byte loads and stores)
 *   [2] candidates per arithmetic state: 2 = packed pairs, 1 = plain float32 (always 1 with one candidate per lane)
 *   [3] workgroups per problem = partial keys per problem (what acmpc_finalize_device / acmpc_finalize_sampled_device
 *       expect of the rollout before them; the rows kernel launches a quarter as many workgroups, of four waves)
 *   [4] ACMPC_ROLLOUT_* below: the kernel family
 *   [5] the one-launch rollout + finalize (ACMPC_TAILED_ROLLOUT) takes this shape
 *   [6] a stream of batches of this shape chains: batch k's finalize inside batch k + 1's rollout launch
 *       (unless ACMPC_NO_CHAINED_STREAM)
 *   [7] acmpc_solve_device and acmpc_solve do NOT make this launch here: they take the one-launch solve
 *       (rollout_solo_kernel) at this size
 * One thing the hook cannot see: the rows kernel moves 16-byte pieces, so a launch whose `d_U` does not start on a
 * 16-byte boundary takes the LDS-tile kernel instead, whatever [4] says - that is decided at the launch, from the pointer.
 * ACMPC_ECAPACITY beyond the handle's capacities, ACMPC_ESTATE in mode D. */
#define ACMPC_ROLLOUT_STEP 0         /* rollout_kernel: a lane walks its candidates' steps, controls straight from memory */
#define ACMPC_ROLLOUT_TILE 1         /* candidate-major: one wave per workgroup, its 64 rows staged in LDS */
#define ACMPC_ROLLOUT_ROWS_LDS 2     /* candidate-major, mode S: rows in registers, the table's rows from LDS */
#define ACMPC_ROLLOUT_ROWS_SCALAR 3  /* ... the table's rows by scalar loads */
int acmpc_describe_rollout(const acmpc_ctx* ctx, int32_t P, int32_t N, int32_t n, int32_t layout, int32_t out[8]);

/* Test hook of the softmin mean (any mode): the launches acmpc_softmin_device (`form` = the matrix's layout) and
 * acmpc_softmin_sampled_device (`form` = ACMPC_SOFTMIN_SAMPLED) make for (P, N, n) on this handle.  The answer comes from
 * the functions the launchers themselves ask (csrc: softmin_chunks, softmin_rows, softmin_item_count, softmin_items) and,
 * for the sampled form, from the sampler's knot table of this horizon; no device work, the GPU is not initialised.  out[8] =
 *   [0] chunks of 1 024 candidates per problem: the partial kernel's workgroups per problem (and per gridDim.z)
 *   [1] candidate-major: thread groups that sum rows side by side, 256 / 2n (1 from n = 65 on)
 *   [2] candidate-major: passes of 256 entries over a row of 2n floats (1 up to n = 128)
 *   [3] sampled: items - runs of at most 8 steps that share a left knot
 *   [4] sampled: workgroups per chunk (gridDim.z), four waves each
 *   [5] sampled: the most items one wave walks, ceil(items / (4 gridDim.z))
 *   [6], [7] 0; so are the entries of the other forms
 * Refuses what the calls refuse of a shape: ACMPC_EINVAL for a size below 1, an unknown form or a softmin_lambda that is
 * not positive, ACMPC_ECAPACITY beyond the handle's capacities, ACMPC_ESTATE on a mode D handle without a vehicle.  (That
 * n is the horizon of the tables set - at least 2 - is the calls' own check.) */
#define ACMPC_SOFTMIN_CANDIDATE_MAJOR 0 /* = ACMPC_LAYOUT_CANDIDATE_MAJOR */
#define ACMPC_SOFTMIN_STEP_MAJOR 1      /* = ACMPC_LAYOUT_STEP_MAJOR */
#define ACMPC_SOFTMIN_SAMPLED 2
int acmpc_describe_softmin(const acmpc_ctx* ctx, int32_t P, int32_t N, int32_t n, int32_t form, int32_t out[8]);

/* Test hook of the grip identification (mode D): the grid acmpc_score_grips launches for a log of W steps cut into
 * segments of `segment` steps and K hypotheses, from the function the launcher itself asks (csrc: identify_grid); no
 * device work, the GPU is not initialised.  out[8] =
 *   [0] S = ceil(W / segment) segments
 *   [1] blocks = ceil(K / 256): workgroups along the hypotheses = partial keys
 *   [2] rows = min(S, 2048 / blocks): the runs of segments aimed at
 *   [3] run = ceil(S / rows): segments one workgroup rolls
 *   [4] grid.y = ceil(S / run)
 *   [5] segments in the last run, 1 .. run
 *   [6] steps in the last segment, 1 .. segment
 *   [7] 0
 * Refuses what acmpc_score_grips refuses of a shape, with its codes: ACMPC_ESTATE off mode D or without a vehicle,
 * ACMPC_EINVAL for W outside 1 .. ACMPC_MAX_LOG_STEPS, segment outside 1 .. W or K < 1, ACMPC_ECAPACITY for
 * K > ACMPC_MAX_GRIP_HYPOTHESES or S K > 2^22. */
int acmpc_describe_score_grips(const acmpc_ctx* ctx, int32_t W, int32_t segment, int32_t K, int32_t out[8]);

/* Host-side float64 helpers round one solve (csrc/acmpc_host_path.cpp; no GPU work, no handle).
 * Replaces: SpatialMPC.construct_waypoints (spatial_mpc.py:125-154).  coords [H][3] = (x, y, width) ->
 * table [7][n], n = H - 1, rows [x, y, psi, kappa, ds, width, v = 0]. */
int acmpc_waypoint_table(const double* coords, int32_t H, double eps, double* table);
/* Replaces: the v_max vector of SpeedProfileSolver / LocalisedSpeedProfileSolver (speed_profile.py:26-43,131-150):
 * max(v_min, min(sqrt(ay_max / (|kappa| + 1e-12)), v_max)) + 2 with v_max where |kappa| < ki_min, last entry =
 * end_velocity when given; `localised` != 0: v_max everywhere. */
int acmpc_velocity_ceiling(const double* kappa, int32_t n, double ay_max, double ki_min, double v_min, double v_max,
                           int32_t localised, int32_t has_end_velocity, double end_velocity, double* ceiling);
/* Replaces: the tail of SpatialMPC.get_control (spatial_mpc.py:156-168,195-211).  z = dec.x ([x_0..x_n ; u_0..u_{n-1}],
 * 5n + 3 doubles), table [7][n] -> projected_control [2][n] = (v, atan(kappa L)), prediction [n][2] (s2t),
 * cum_time [n], times / accelerations / steer_rates [n - 1]. */
int acmpc_unpack_decision(const double* z, int32_t n, const double* table, double wheelbase, double* projected_control,
                          double* prediction, double* cum_time, double* times, double* accelerations,
                          double* steer_rates);
/* The same for a mode T plan (build-defined: the reference has no temporal rollout).  z's states are the poses
 * (X, Y, phi) after each Euler step of `dt` seconds: prediction [n][2] = the first n of them, cum_time [i] = i dt,
 * times = dt, and the derivatives are those of the plan's own controls: accelerations = dv / dt, steer_rates =
 * d(delta) / dt. */
int acmpc_unpack_decision_temporal(const double* z, int32_t n, double dt, double wheelbase, double* projected_control,
                                   double* prediction, double* cum_time, double* times, double* accelerations,
                                   double* steer_rates);

/* Host side of mode T's verified nearest-waypoint search (exhaustive semantics, localiser.py:282-289: the first minimum
 * over ALL waypoints), as acmpc_set_paths tabulates it for the kernels: coef = P packed [n][8] waypoint rows
 * (acmpc_get_coefficients) -> per problem acmpc_search_frame_floats(n) floats: for every window of
 * acmpc_search_window(NULL) consecutive waypoints [t_x, t_y, k_along, k_across, slab, tube, far, -slack].  The kernel
 * accepts the window's first minimum j as the global one when
 *     |fma(Y, Y, fma(X, X, key_j))| < min(fma(across, across, fma(along, along, -slack)), far),
 * alpha = fma(t_x, X, fma(t_y, Y, k_along)), beta = fma(t_x, Y, fma(-t_y, X, k_across)), along = med3(alpha,
 * slab - alpha, 0), across = med3(|beta| - tube, 0, 32), and scans the whole path otherwise.  No device work: lets
 * tests check on the CPU that an accepted index is always the exhaustive one.  n < the window: ACMPC_EINVAL. */
int32_t acmpc_search_window(int32_t* back);
int32_t acmpc_search_frame_floats(int32_t n);
int acmpc_search_frames(const float* coef, int32_t P, int32_t n, float* out, int64_t capacity_floats);

/* The generator itself, on the host (same code as the kernels): lets tests pin the integer stream. */
void acmpc_philox4x32(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/* Replaces: the osqp calls of SpeedProfileSolver (src/acmpc/control/solvers/speed_profile.py:61-86).  Solves
 *     min 1/2 |v|^2 - v_hi'v   s.t.  a_min <= (v[i+1] - v[i]) / (2 ds[i]) <= a_max,  v_min <= v <= v_hi
 * on the host with the OSQP splitting specialised to the problem's tridiagonal structure: O(n) per iteration, so the
 * whole-lap profile (n ~ 1e4, spatial_mpc.py:60-87) is as cheap per iteration as the horizon's.  `v` [n] and `y`
 * [2n - 1] hold the primal/dual iterate: read when warm_start != 0, always written.  The stopping test (OSQP's, at
 * eps_abs / eps_rel) runs every `check_every` iterations (<= 0: 10).  Returns 0 = solved, 1 = maximum iterations
 * reached, ACMPC_EINVAL on bad arguments.  A problem without an optimum - some v_hi[i] < v_min (a box row with l > u), a
 * spacing that is not positive and finite - is never reported solved: the iteration runs to max_iter (returns 1,
 * *iterations = max_iter).  No GPU work.  The device prologue of acmpc_control_tick runs the same
 * statement of the algorithm (csrc/acmpc_admm.h) on one wavefront: same float64 operations in the same order. */
int acmpc_speed_profile_qp(const double* v_hi, const double* ds, int32_t n, double a_min, double a_max, double v_min,
                           int32_t max_iter, int32_t check_every, double eps_abs, double eps_rel, double* v, double* y,
                           int32_t warm_start, int32_t* iterations);

/* The same QP solved EXACTLY, without iterating (csrc/acmpc_admm.h exact_profile): its objective is 1/2 |v - v_hi|^2 up to a
 * constant and v_hi is also the upper bound, so the optimum is the pointwise largest feasible profile - v_hi cut down by a
 * forward sweep (a_max) and a backward sweep (a_min).  Returns 0 with v [n] = the optimum and y [2n - 1] = 0; 1 when the
 * problem is not of that shape (a_min > 0, a_max < 0, a spacing that is not positive and finite, a non-finite ceiling) or
 * infeasible (some v below v_min) - v and y are then left exactly as they were, so a warm iterate in them is still there
 * for acmpc_speed_profile_qp, which solves the problems with a rate bound of the wrong sign and reports the others as not
 * solved; ACMPC_EINVAL on bad arguments.  acmpc_control_tick's prologue does exactly this on the device (qp_method 0).
 * No GPU work. */
int acmpc_speed_profile_exact(const double* v_hi, const double* ds, int32_t n, double a_min, double a_max, double v_min,
                              double* v, double* y);

/* Diagnostic: with acmpc_set_option(ctx, "ACMPC_START_CLOCKS", "1") every workgroup of a rollout launch
 * (acmpc_rollout_device and the calls built on it; not the candidate-major tile kernels) leaves the 100 MHz wall clock of
 * its first instruction on the device; this copies the LAST launch's out (after a device synchronise): `count` = its
 * workgroups, P x blocks per problem, problem-major.  A launch that fits the chip in one generation should start all of
 * them within a couple of microseconds; workgroups that start tens of microseconds late are what a dispatcher that
 * over-subscribes some compute units looks like.  *count = 0: no stamped launch yet. */
int acmpc_rollout_start_clocks(acmpc_ctx* ctx, uint64_t* out, int32_t capacity, int32_t* count);

/* Measurement hooks.  After acmpc_profile_enable(ctx, K) the next K rollout launches of this handle carry a HIP
 * event pair attached to the dispatch itself (hipExtLaunchKernel: the kernel's own begin/end timestamps on the
 * stream it is launched on, no marker packets between launches); acmpc_profile_collect waits for them, writes the
 * per-launch durations in milliseconds and re-arms the K pairs.  K = 0 disables. */
int acmpc_profile_enable(acmpc_ctx* ctx, int32_t capacity);
int acmpc_profile_collect(acmpc_ctx* ctx, float* out_ms, int32_t capacity, int32_t* count);

/* Key helpers (host side; same packing as the kernels). */
int64_t acmpc_pack_key(float cost, uint32_t index);
float acmpc_key_cost(int64_t key);
uint32_t acmpc_key_index(int64_t key);

/* ---- particle-filter localiser: scoring on the GPU -------------------------------------
 * Replaces the data-parallel part of LocalisationProcess._update_particles (src/acmpc/localisation/localiser.py:
 * 255-410): three nearest-point queries per particle against the centre / left / right map polylines (what the
 * reference's scipy KD-trees answer), the heading offset, the observed track limits placed in every particle's
 * frame against the map limits ahead of it, the Gaussian score and the validity mask (localiser.py:453-462).
 * Resampling (sequential, random) stays with the caller.  Same conventions as above; no device work at create. */
typedef struct acmpc_pf acmpc_pf;

typedef struct acmpc_pf_params {
  uint32_t struct_size;
  int32_t device;                   /* HIP device ordinal, -1 = current                                      */
  int32_t max_particles;            /* localisation.n_particles (configs/monza.yaml:47)                       */
  int32_t max_observation_points;   /* left + right observed limit points after downsampling                 */
  double score_mean, score_sigma;   /* localisation.score_distribution (monza.yaml:61-63)                     */
  double threshold_rotation;        /* [rad]  localisation.thresholds.rotation * pi / 180 (localiser.py:616)  */
  double threshold_offset;          /* [m]    localisation.thresholds.offset                                  */
  double threshold_error;           /* [m]    localisation.thresholds.track_limit                             */
  double wheelbase;                 /* for acmpc_pf_advance (localiser.py:83, 94)                             */
} acmpc_pf_params;

/* centre / left / right: map polylines [m][2] float64 (utils/load.py:9-35 order x, y); copied. */
int acmpc_pf_create(const acmpc_pf_params* params, const double* centre, int32_t m_centre, const double* left,
                    int32_t m_left, const double* right, int32_t m_right, acmpc_pf** out);
void acmpc_pf_destroy(acmpc_pf* handle);
const char* acmpc_pf_last_error(const acmpc_pf* handle);
double acmpc_pf_score_scale(const acmpc_pf* handle); /* max pdf over linspace(-10, 10, 100), localiser.py:655-661 */

/* states [P][3] float32 (x, y, yaw); obs_left [k_left][2], obs_right [k_right][2] float32 in the vehicle frame
 * (x right, y forward), already downsampled and cut at y < 50 (localiser.py:246-253,336-337).  Outputs per particle:
 * track_indices [P][3] (centre, left, right), minimum_offset, heading_offset, observation_error, score (float64 as
 * in the reference), valid (0/1).  Blocking; host pointers. */
int acmpc_pf_score(acmpc_pf* handle, const float* states, int32_t P, const float* obs_left, int32_t k_left,
                   const float* obs_right, int32_t k_right, int32_t* track_indices, double* minimum_offset,
                   double* heading_offset, double* observation_error, double* score, uint8_t* valid);

/* states += (v cos phi, v sin phi, v tan(delta) / L) * dt with per-particle delta, v (localiser.py:66-95). */
int acmpc_pf_advance(acmpc_pf* handle, float* states, const float* delta, const float* velocity, int32_t P, double dt);

/* Score-weighted mean state with the NaN -> uniform fallback, and the largest distance / yaw difference of any
 * particle to it - the two numbers the convergence flag compares with its limits (localiser.py:561-579). */
int acmpc_pf_estimate(acmpc_pf* handle, const float* states, const float* scores, int32_t P, double estimate[3],
                      double* max_distance, double* max_angle);

/* ---- device-resident particle filter: one host round trip per update ------------------------------------------------
 * The reference's update cycle with the particles living on the GPU: Localiser.step (localiser.py:41-77: every particle
 * moves with its own noisy control), then _score_particles (localiser.py:234-239): score, publish the scores, resample
 * (keep the valid particles in order; fewer than `minimum_particles` left -> _reset_filter, localiser.py:468-485;
 * otherwise top up to `n_desired` with copies of kept particles drawn in proportion to their score, plus Gaussian
 * noise, localiser.py:486-545), estimate and convergence numbers (localiser.py:561-579).  The random draws are
 * Philox4x32-10 at counter (index, `counter`, tag, draw) with key `seed` - NOT NumPy's global stream, whose call order a
 * kernel cannot follow: the host-side ParticleFilter (NumPy resampling, the reference's draw order) stays the parity
 * mode, this path is pinned by the oracle's restatement of these draws (exact picked indices: integer weights
 * floor(score 2^40), integer prefix sums, mulhi of a 64-bit word with the total). */
typedef struct acmpc_pf_resample {
  uint32_t struct_size;
  int32_t n_desired;          /* n_particles, or n_converged_particles once converged (localiser.py:497-500)         */
  int32_t minimum_particles;  /* thresholds.minimum_particles                                                       */
  uint32_t counter;           /* update number: a fresh set of draws per update                                     */
  uint64_t seed;
  double sigma_x, sigma_y, sigma_yaw;  /* sampling_noise (yaw in radians)                                           */
} acmpc_pf_resample;

/* _reset_filter on the device: `n` particles evenly along the centre line, uniform scores. */
int acmpc_pf_filter_reset(acmpc_pf* handle, int32_t n);
/* Upload / download the live particles (states [n][3], scores [n] float32). */
int acmpc_pf_filter_set(acmpc_pf* handle, const float* states, const float* scores, int32_t n);
int acmpc_pf_filter_get(acmpc_pf* handle, float* states, float* scores, int32_t capacity, int32_t* n);
/* Localiser.step: delta = tyre_angle + N(0, sigma_yaw), speed = |velocity + N(0, sigma_velocity)|, kinematic Euler step.
 * Asynchronous (ordered before the next update on the handle's stream). */
int acmpc_pf_filter_step(acmpc_pf* handle, double tyre_angle, double velocity, double dt, double sigma_yaw,
                         double sigma_velocity, uint64_t seed, uint32_t counter);
/* One _score_particles.  result [8] = {estimate x, y, yaw, max distance, max |yaw difference| to the estimate,
 * live particles after the update, valid particles of this scoring, 1 if the filter was reset}. */
int acmpc_pf_filter_update(acmpc_pf* handle, const float* obs_left, int32_t k_left, const float* obs_right,
                           int32_t k_right, const acmpc_pf_resample* resample, double* result);

/* Library identification: "acmpc-hip <version> gfx950". */
const char* acmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ACMPC_H */
