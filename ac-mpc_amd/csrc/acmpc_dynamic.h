// Mode D: candidates scored through the dynamic (Pacejka) bicycle of the reference (src/acmpc/control/
// dynamic_bicycle_model.py) - device arithmetic and the launchers (acmpc_dynamic.hip) of its kernels
// (acmpc_dynamic_kernels.h).
//
// The float32 "spec order" of DESIGN.md section 2 ("Mode D"), restated bit for bit by tests/dynamic_spec.py: the
// reference's expression tree evaluated left to right, no fused multiply-add except inside the named polynomial kernels
// (atan_spec here, sincos_spec / wrap_spec of acmpc_device.h, the search key and the cost accumulators of mode T),
// divisions IEEE and correctly rounded (hipcc's default for `/` on float: v_div_scale / v_div_fmas / v_div_fixup), no
// library or hardware transcendental.  Every function is written once for F = float (one candidate per lane) and
// F = f32x2 (two candidates per lane in v_pk_* instructions); per element the operations and their order do not depend
// on F.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "acmpc_device.h"
#include "acmpc_kernels.h"

#pragma clang fp contract(off)

namespace acmpc {

constexpr int kDynamicsCount = 26;   // ACMPC_DYNAMICS_COUNT: doubles in the vehicle block of acmpc_set_dynamics
constexpr int kDynamicStateFloats = 6;
constexpr int kDynamicMaxSteps = 512;   // the rollout's LDS tables (64 B per waypoint) and the finalize's record image

// The float32 constants of the step, derived by the host in float64 from the vehicle block and rounded once each
// (acmpc_capi.hip: acmpc_set_dynamics; tests/dynamic_spec.py: derived_constants - same list, same order).  Passed by value
// in the kernel arguments: SGPRs.
struct Vehicle {
  float lf, lr;
  float Bf, Cf, Ef, Pf;   // Pf = Df (1 + epsf F_zf / F_z0) F_zf / F_z0, F_zf = mass g lr / (lr + lf)
  float Br, Cr, Er, Pr;   // Pr = Dr (1 + epsr F_zr / F_z0) F_zr / F_z0, F_zr = mass g lf / (lr + lf)
  float mass, inv_mass, inv_Iz;
  float Cm1, Cm2, Cm3;    // drive map   (Cm1 - Cm2 vx - Cm3 vx^2) max(pedal, 0)
  float Cb1, Cb2, Cb3;    // brake map   (Cb1 - Cb2 vx - Cb3 vx^2) min(pedal, 0), split front / rear by the bias
  float fric0, Cfric2, Cfric3;   // fric0 = -Cfric1: F_fric = (-Cfric1 - Cfric2 vx) - Cfric3 vx^2
  float bias_front, bias_rear;   // brake_bias, 1 - brake_bias
  float wheelbase;        // acmpc_params::wheelbase: delta_ref = atan_spec(wheelbase * k_ref) of the waypoint rows
};

// An ensemble of vehicles (acmpc_set_dynamics_ensemble, DESIGN.md section 2 "Mode D", "Ensembles"): every candidate is
// rolled under each of the K vehicles from the same x0 and controls, and its cost is the MEAN (omega_0 c_0, then
// fma(omega_k, c_k, J) in k order) or the MAX (NaN if any is NaN) of the K costs; its violation is the max of the K
// violations (NaN if any is NaN).  omega = the weights normalised on the host in float64, each rounded once.  One vehicle
// (acmpc_set_dynamics) is K = 1 and runs the single-vehicle kernels.  A kernel argument: the vehicle of a wavefront is
// indexed by a wave-uniform value, so its constants are read by scalar loads into SGPRs, as one Vehicle's are.
constexpr int kMaxVehicles = 8;   // ACMPC_MAX_VEHICLES
constexpr int kEnsembleMean = 0;  // ACMPC_ENSEMBLE_MEAN
constexpr int kEnsembleMax = 1;   // ACMPC_ENSEMBLE_MAX
struct VehicleEnsemble {
  Vehicle v[kMaxVehicles];
  float omega[kMaxVehicles];
  int K;
  int reduce;
};

// J and V of one candidate from its K per-vehicle costs c[k * stride] and violations v[k * stride], in k order
__device__ __forceinline__ void ensemble_combine(const float* c, const float* v, int stride, const VehicleEnsemble& e,
                                                 float& J, float& V) {
  J = (e.reduce == kEnsembleMean) ? e.omega[0] * c[0] : c[0];
  V = v[0];
  for (int k = 1; k < e.K; ++k) {
    const float ck = c[k * stride], vk = v[k * stride];
    J = (e.reduce == kEnsembleMean) ? fma_(e.omega[k], ck, J) : ((ck > J || ck != ck) ? ck : J);
    V = (vk > V || vk != vk) ? vk : V;
  }
}

// atan t = t + t^3 P(t^2) on [0, 1], P of degree 7 in t^2 (tools/fit_atan.py: Lawson-weighted least squares, float32
// coefficients, Horner with fused multiply-adds): |error| < 6.8e-8 on [0, 1], < 2e-7 (1.53e-7 measured) on the real line
constexpr float kAtanC[8] = {-0.33332985639572144f, 0.1999039649963379f,  -0.1418597251176834f,   0.10573919117450714f,
                             -0.0736667662858963f,  0.041121501475572586f, -0.015132308006286621f, 0.0026221852749586105f};
constexpr float kHalfPi = 1.5707963267948966f;
constexpr float kVxEps = 1.0e-3f;   // dynamic_bicycle_model.py:97-98

// Arctangent of the specification, defined for every input: t = |x|, or 1 / |x| (IEEE division) when |x| > 1; the odd
// polynomial; pi/2 - a beyond 1; the sign of x.  atan(+-0) = +-0, atan(+-inf) = +-pi/2, a NaN stays NaN.
template <typename F>
__device__ __forceinline__ F atan_spec(F x) {
  using I = typename IndexOf<F>::type;
  const F ax = abs_(x);
  const auto small = ax <= splat<F>(1.0f);
  const F inv = splat<F>(1.0f) / ax;
  const F t = small ? ax : inv;
  const F t2 = t * t;
  F p = fma_(t2, splat<F>(kAtanC[7]), splat<F>(kAtanC[6]));
#pragma unroll
  for (int q = 5; q >= 0; --q) p = fma_(t2, p, splat<F>(kAtanC[q]));
  const F a = fma_(t * t2, p, t);
  const F r = small ? a : (splat<F>(kHalfPi) - a);
  return __builtin_bit_cast(F, (__builtin_bit_cast(I, r) & 0x7fffffff) | (__builtin_bit_cast(I, x) & I(0x80000000)));
}

template <typename F>
__device__ __forceinline__ F sin_spec(F x) {
  F s, c;
  sincos_spec<F>(x, s, c);
  return s;
}

// The mode-T state (pose in the path's own frame, Frenet errors, cost sums) plus the velocities of the dynamic model.
template <typename F>
struct StateD_ {
  StateT_<F> t;   // t.X, t.Y, t.phi = yaw
  F vx, vy, r;
};
using StateD = StateD_<float>;

// x0 = (X, Y, yaw, vx, vy, r) in the caller's frame; positions move into the path's own frame (start_temporal)
template <typename F>
__device__ __forceinline__ StateD_<F> start_dynamic(const float* __restrict__ x0, const float* __restrict__ coef) {
  StateD_<F> s;
  s.t = start_temporal<F>(x0, coef);
  s.vx = splat<F>(x0[3]);
  s.vy = splat<F>(x0[4]);
  s.r = splat<F>(x0[5]);
  return s;
}

// Pacejka's lateral force of one axle: P sin(C atan(B a - E (B a - atan(B a))))
template <typename F>
__device__ __forceinline__ F pacejka(F alpha, float B, float C, float E, float P) {
  const F ba = B * alpha;
  const F y = ba - E * (ba - atan_spec<F>(ba));
  return P * sin_spec<F>(C * atan_spec<F>(y));
}

// The same with a peak of the lane's own (the load transfer: the loaded peak P' in front of the unchanged shape)
template <typename F>
__device__ __forceinline__ F pacejka_loaded(F alpha, float B, float C, float E, F P) {
  const F ba = B * alpha;
  const F y = ba - E * (ba - atan_spec<F>(ba));
  return P * sin_spec<F>(C * atan_spec<F>(y));
}

// Where a step takes the two axles' peak factors from: the Vehicle's own (every rollout: scalars of the kernel argument,
// read where the step has always read them) or a lane's pair (the grip identification, acmpc_identify.hip: one hypothetical
// vehicle per lane, everything but its two peaks the base Vehicle's).
struct VehiclePeaks {
  __device__ __forceinline__ float front(const Vehicle& k) const { return k.Pf; }
  __device__ __forceinline__ float rear(const Vehicle& k) const { return k.Pr; }
};
struct LanePeaks {
  float Pf, Pr;
  __device__ __forceinline__ float front(const Vehicle&) const { return Pf; }
  __device__ __forceinline__ float rear(const Vehicle&) const { return Pr; }
};

// A lane's pair typed on F (the surface table, acmpc_set_surface: every candidate of a lane under the grip scales of the waypoint
// it is at - two per lane under f32x2): what the step multiplies into per-lane values anyway, so it adds no arithmetic.
template <typename F>
struct SurfacePeaks {
  F Pf, Pr;
  __device__ __forceinline__ F front(const Vehicle&) const { return Pf; }
  __device__ __forceinline__ F rear(const Vehicle&) const { return Pr; }
};

// The tyre coupling of a handle (acmpc_set_dynamics_coupling, DESIGN.md section 2 "Mode D, tyre coupling"): each axle's
// longitudinal force is clipped at rho times that axle's peak factor, and its Pacejka side force scaled by what the friction
// ellipse leaves.  It reaches the step with the peaks, whose multiples its caps are: a peak source (above) with the two ratios
// beside it, each rounded to float32 once (+inf: no coupling on that axle).  Under a plain source the step compiles nothing of
// this (every kernel without the coupling: the code it was).
template <typename PK>
struct CoupledPeaks : PK {
  float rho_f, rho_r;
};
template <typename PK>
struct IsCoupled : std::false_type {};
template <typename PK>
struct IsCoupled<CoupledPeaks<PK>> : std::true_type {};

// correctly rounded float32 square root (what hipcc emits for the builtin under the library's flags: a v_sqrt_f32 seed and an
// FMA fix-up)
__device__ __forceinline__ float sqrt_(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ f32x2 sqrt_(f32x2 a) { return __builtin_elementwise_sqrt(a); }

// One axle under the coupling, in spec order: cap = rho P; F_x = max(min(F_x, cap), -cap); u = F_x / cap (IEEE division);
// g = sqrt(1 - u u); F_y = F_y g.  After the clip |u| <= 1: the square root is never a NaN of its own making; a saturated axle
// has u = +-1 exactly, g = 0; F_x = +-0 (pedal 0) and cap = +inf give g = 1 and F_y back bit for bit.
template <typename F>
__device__ __forceinline__ void couple_axle(F& F_x, F& F_y, float rho, float P) {
  const float cap = rho * P;
  F_x = vmax(__builtin_elementwise_min(F_x, splat<F>(cap)), splat<F>(-cap));
  const F u = F_x / splat<F>(cap);
  const F g = sqrt_(splat<F>(1.0f) - u * u);
  F_y = F_y * g;
}

// The longitudinal load transfer of a handle (acmpc_set_dynamics_load_transfer, DESIGN.md section 2 "Mode D, load transfer"):
// each axle's load, and with it its peak factor and its coupling cap, follows the longitudinal tyre force inside every Euler
// sub-step.  A CoupledPeaks with the six scalars of the vehicle rolled beside it, each derived by the host in float64 and
// rounded once: c_h = h_cg / (lf + lr), w_max = w_frac min(F_zf, F_zr), and per axle (a1, a2) with
// P(F_z + x) / P(F_z) = 1 + x (a1 + a2 x).  rho = +inf on both axles while the coupling is off.  Not an IsCoupled: the step
// has a block of its own for it.
template <typename PK>
struct LoadedPeaks : CoupledPeaks<PK> {
  float c_h, w_max, a1_f, a2_f, a1_r, a2_r;
};
template <typename PK>
struct IsLoaded : std::false_type {};
template <typename PK>
struct IsLoaded<LoadedPeaks<PK>> : std::true_type {};

// couple_axle with the lane's loaded peak: cap = rho P' per lane, the rest as it is
template <typename F>
__device__ __forceinline__ void couple_axle_loaded(F& F_x, F& F_y, float rho, F P) {
  const F cap = rho * P;
  F_x = vmax(__builtin_elementwise_min(F_x, cap), -cap);
  const F u = F_x / cap;
  const F g = sqrt_(splat<F>(1.0f) - u * u);
  F_y = F_y * g;
}

// The two loaded peaks of a sub-step, in spec order: the demands clipped at the STATIC caps, w = c_h (e_f + e_r) clipped at
// +-w_max (the load moved to the rear; negative: braking), x_f = -w, x_r = w, phi = 1 + x (a1 + a2 x) - multiply, add,
// multiply, add - and P' = P phi.  min / max are minNum / maxNum.  h_cg = 0 or pedal 0 give w = +-0, phi = 1, P' = P.
template <typename F, typename PK>
__device__ __forceinline__ void loaded_peaks_of(F F_fx, F F_rx, const Vehicle& k, const LoadedPeaks<PK>& pk, F& Pf, F& Pr) {
  const float cap_f = pk.rho_f * pk.front(k);
  const float cap_r = pk.rho_r * pk.rear(k);
  const F e_f = vmax(__builtin_elementwise_min(F_fx, splat<F>(cap_f)), splat<F>(-cap_f));
  const F e_r = vmax(__builtin_elementwise_min(F_rx, splat<F>(cap_r)), splat<F>(-cap_r));
  F w = pk.c_h * (e_f + e_r);
  w = vmax(__builtin_elementwise_min(w, splat<F>(pk.w_max)), splat<F>(-pk.w_max));
  const F x_f = -w, x_r = w;
  const F phi_f = splat<F>(1.0f) + x_f * (pk.a1_f + pk.a2_f * x_f);
  const F phi_r = splat<F>(1.0f) + x_r * (pk.a1_r + pk.a2_r * x_r);
  Pf = pk.front(k) * phi_f;
  Pr = pk.rear(k) * phi_r;
}

// Aerodynamic downforce of a handle (acmpc_set_dynamics_downforce, DESIGN.md section 2 "Mode D, downforce"): each axle's load
// grows with the square of the sub-step's incoming speed, up to v_sat, and the load transfer then moves load on top of that.  A
// LoadedPeaks with k_f, k_r (force per speed squared) and v_sat beside its six scalars, each rounded to float32 once; c_h = 0 and
// w_max = 0 while the load transfer is off, rho = +inf while the coupling is off.  Not an IsLoaded: a block of its own again.
template <typename PK>
struct AeroPeaks : LoadedPeaks<PK> {
  float k_f, k_r, v_sat;
};
template <typename PK>
struct IsAero : std::false_type {};
template <typename PK>
struct IsAero<AeroPeaks<PK>> : std::true_type {};

// Road grade and banking (acmpc_set_road, DESIGN.md section 2 "Mode D, road"): the surface's peak source - the lane's peaks,
// here the vehicle's scaled by the grip scales and by the road's factor n_z on the normal load - with gravity's two in-plane
// accelerations of the lane's waypoint beside it, typed on F like the peaks.  An IsAero (the step's block is the downforce's, on
// these peaks) and the one IsRoad: dynamic_euler adds a_x to xd3 and a_y to xd4, one float32 add each.
template <typename F>
struct RoadPeaks : AeroPeaks<SurfacePeaks<F>> {
  F ax, ay;
};
template <typename F>
struct IsAero<RoadPeaks<F>> : std::true_type {};
template <typename PK>
struct IsRoad : std::false_type {};
template <typename F>
struct IsRoad<RoadPeaks<F>> : std::true_type {};

// The two peaks of a sub-step under the downforce, in spec order: va = min(vx, v_sat) (minNum: a NaN vx gives v_sat), q = va va,
// d_a = k_a q, psi_a = 1 + d_a (a1_a + a2_a d_a), P_a0 = P_a psi_a - the peaks at this speed before any tyre force; the demands
// clipped at the caps rho_a P_a0 AT THIS SPEED, w = c_h (e_f + e_r) clipped at +-w_max, x_f = d_f - w, x_r = d_r + w,
// phi_a = 1 + x_a (a1_a + a2_a x_a), P_a' = P_a phi_a.  k = 0 gives d = +0, psi = 1, x = -+w: the loaded step's bits.
template <typename F, typename PK>
__device__ __forceinline__ void aero_peaks_of(F vx, F F_fx, F F_rx, const Vehicle& k, const AeroPeaks<PK>& pk, F& Pf, F& Pr) {
  const F va = __builtin_elementwise_min(vx, splat<F>(pk.v_sat));
  const F q = va * va;
  const F d_f = pk.k_f * q, d_r = pk.k_r * q;
  const F psi_f = splat<F>(1.0f) + d_f * (pk.a1_f + pk.a2_f * d_f);
  const F psi_r = splat<F>(1.0f) + d_r * (pk.a1_r + pk.a2_r * d_r);
  const F cap_f = pk.rho_f * (pk.front(k) * psi_f);
  const F cap_r = pk.rho_r * (pk.rear(k) * psi_r);
  const F e_f = vmax(__builtin_elementwise_min(F_fx, cap_f), -cap_f);
  const F e_r = vmax(__builtin_elementwise_min(F_rx, cap_r), -cap_r);
  F w = pk.c_h * (e_f + e_r);
  w = vmax(__builtin_elementwise_min(w, splat<F>(pk.w_max)), splat<F>(-pk.w_max));
  const F x_f = d_f - w, x_r = d_r + w;
  const F phi_f = splat<F>(1.0f) + x_f * (pk.a1_f + pk.a2_f * x_f);
  const F phi_r = splat<F>(1.0f) + x_r * (pk.a1_r + pk.a2_r * x_r);
  Pf = pk.front(k) * phi_f;
  Pr = pk.rear(k) * phi_r;
}

// What a step takes from its control alone: sincos_spec(delta) and the pedal's split.  The same for every sub-step of a
// control step (dynamic_advance_fine computes it once).
template <typename F>
struct ControlTerms {
  F sd, cd, p_neg, p_pos;
};
template <typename F>
__device__ __forceinline__ ControlTerms<F> control_terms(F delta, F pedal) {
  ControlTerms<F> c;
  c.p_neg = __builtin_elementwise_min(pedal, splat<F>(0.0f));
  c.p_pos = vmax(pedal, splat<F>(0.0f));
  sincos_spec<F>(delta, c.sd, c.cd);
  return c;
}

// One explicit Euler step of predict_next_state (dynamic_bicycle_model.py:88-160) with u = (delta, pedal), then
// vx = max(vx, 0) (the reference's loop, :180; maxNum: a NaN vx becomes 0).  HOISTED: the control's terms come in
// through `pre` (the sub-steps of dynamic_advance_fine); otherwise they are computed here, where the single step has
// always computed them - the default setting's kernels are to stay the code they were, instruction for instruction.
// PK: the source of the peak factors (VehiclePeaks or LanePeaks), or a CoupledPeaks of one: the tyre coupling; or a LoadedPeaks
// of one: the coupling with the load transfer in front of it (the side forces then wait for the loaded peaks); or an AeroPeaks
// of one: the same with the downforce of the sub-step's incoming speed under the load moved; or a RoadPeaks: that on the lane's
// own peaks, with gravity's two in-plane accelerations added to xd3 and xd4.
template <bool HOISTED, typename F, typename PK = VehiclePeaks>
__device__ __forceinline__ void dynamic_euler(StateD_<F>& s, F delta, F pedal, const ControlTerms<F>* pre, const Vehicle& k,
                                              float dt, const PK pk = PK{}) {
  const F vx = s.vx, vy = s.vy, r = s.r;
  const F den = vx + kVxEps;
  const F qf = (r * k.lf + vy) / den;
  const F qr = (r * k.lr - vy) / den;
  const F a_f = delta - atan_spec<F>(qf);   // the reference's -atan(q) + delta: the same float
  const F a_r = atan_spec<F>(qr);
  F F_fy, F_ry;
  if constexpr (!IsLoaded<PK>::value && !IsAero<PK>::value) {
    F_fy = pacejka<F>(a_f, k.Bf, k.Cf, k.Ef, pk.front(k));
    F_ry = pacejka<F>(a_r, k.Br, k.Cr, k.Er, pk.rear(k));
  }
  const F vx2 = vx * vx;
  const F F_fric = (k.fric0 - k.Cfric2 * vx) - k.Cfric3 * vx2;
  const F brake = (k.Cb1 - k.Cb2 * vx) - k.Cb3 * vx2;
  const F motor = (k.Cm1 - k.Cm2 * vx) - k.Cm3 * vx2;
  F p_neg, p_pos;
  if constexpr (HOISTED) {
    p_neg = pre->p_neg;
    p_pos = pre->p_pos;
  } else {
    p_neg = __builtin_elementwise_min(pedal, splat<F>(0.0f));
    p_pos = vmax(pedal, splat<F>(0.0f));
  }
  F F_rx = (brake * k.bias_rear) * p_neg + motor * p_pos;
  F F_fx = (brake * k.bias_front) * p_neg;
  if constexpr (IsCoupled<PK>::value) {
    couple_axle<F>(F_fx, F_fy, pk.rho_f, pk.front(k));
    couple_axle<F>(F_rx, F_ry, pk.rho_r, pk.rear(k));
  }
  if constexpr (IsLoaded<PK>::value) {
    F Pf, Pr;
    loaded_peaks_of<F>(F_fx, F_rx, k, pk, Pf, Pr);
    F_fy = pacejka_loaded<F>(a_f, k.Bf, k.Cf, k.Ef, Pf);
    F_ry = pacejka_loaded<F>(a_r, k.Br, k.Cr, k.Er, Pr);
    couple_axle_loaded<F>(F_fx, F_fy, pk.rho_f, Pf);
    couple_axle_loaded<F>(F_rx, F_ry, pk.rho_r, Pr);
  }
  if constexpr (IsAero<PK>::value) {
    F Pf, Pr;
    aero_peaks_of<F>(vx, F_fx, F_rx, k, pk, Pf, Pr);
    F_fy = pacejka_loaded<F>(a_f, k.Bf, k.Cf, k.Ef, Pf);
    F_ry = pacejka_loaded<F>(a_r, k.Br, k.Cr, k.Er, Pr);
    couple_axle_loaded<F>(F_fx, F_fy, pk.rho_f, Pf);
    couple_axle_loaded<F>(F_rx, F_ry, pk.rho_r, Pr);
  }
  F sd, cd, sy, cy;
  if constexpr (HOISTED) {
    sd = pre->sd;
    cd = pre->cd;
  } else {
    sincos_spec<F>(delta, sd, cd);
  }
  sincos_spec<F>(s.t.phi, sy, cy);
  const F xd0 = vx * cy - vy * sy;
  const F xd1 = vx * sy + vy * cy;
  F xd3 = k.inv_mass * ((((F_rx + F_fx) + F_fric) - F_fy * sd) + (k.mass * vy) * r);
  F xd4 = k.inv_mass * ((F_ry + F_fy * cd) - (k.mass * vx) * r);
  if constexpr (IsRoad<PK>::value) {   // (gravity along the body's axes on a road that is not level: acmpc_set_road)
    xd3 = xd3 + pk.ax;
    xd4 = xd4 + pk.ay;
  }
  const F xd5 = k.inv_Iz * ((F_fy * k.lf) * cd - F_ry * k.lr);
  s.t.X = s.t.X + xd0 * dt;
  s.t.Y = s.t.Y + xd1 * dt;
  s.t.phi = s.t.phi + r * dt;
  s.vx = vmax(vx + xd3 * dt, splat<F>(0.0f));
  s.vy = vy + xd4 * dt;
  s.r = r + xd5 * dt;
}

template <typename F>
__device__ __forceinline__ void dynamic_advance(StateD_<F>& s, F delta, F pedal, const Vehicle& k, float dt) {
  dynamic_euler<false, F>(s, delta, pedal, nullptr, k, dt);
}

// The integration setting of a handle (acmpc_set_dynamics_integration, DESIGN.md section 2 "Mode D", "Sub-steps and the
// low-speed blend"): a control step of dt is `substeps` Euler steps of h = float32(dt / substeps) under the same control,
// and after each of them (vy, r) is blended towards the kinematic bicycle's r_k = vx tan(delta) / L, vy_k = lr r_k below
// v_hi, entirely below v_lo.  The host derives every float in float64 and rounds it once.  (1, no blend) is the default
// and runs the kernels without any of this (their FINE = false instantiations); anything else their FINE = true ones,
// and the kernels with the rate and slip terms (Terms, below).
constexpr int kMaxSubsteps = 16;   // ACMPC_MAX_SUBSTEPS
struct Integration {
  int substeps;                 // M
  int blend;                    // 0: off
  float h;                      // float32(dt / M)
  float v_lo, inv_span;         // inv_span = float32(1 / (v_hi - v_lo))
  float inv_L[kMaxVehicles];    // float32(1 / (lf + lr)) of each vehicle
};
__host__ __device__ inline bool is_fine(const Integration& g) { return g.substeps != 1 || g.blend != 0; }

// The control step of a FINE kernel: g.substeps times dynamic_euler with step g.h, the control's terms and tan(delta)
// computed once, and the blend after each sub-step's update and clip.  The sub-step count and the blend switch are
// kernel arguments: a scalar loop and a scalar branch, no divergence.  lam == 1 passes the dynamic (vy, r) through bit for
// bit (1 * a + 0 * b); two multiplies and one add each, no fused multiply-add.  PK: as dynamic_euler's.
template <typename F, typename PK = VehiclePeaks>
__device__ __forceinline__ void dynamic_advance_fine(StateD_<F>& s, F delta, F pedal, const Vehicle& k,
                                                     const Integration& g, float inv_L, const PK pk = PK{}) {
  const ControlTerms<F> c = control_terms<F>(delta, pedal);
  const F td = c.sd / c.cd;
#pragma nounroll
  for (int m = 0; m < g.substeps; ++m) {
    dynamic_euler<true, F, PK>(s, delta, pedal, &c, k, g.h, pk);
    if (g.blend != 0) {
      const F r_k = (s.vx * td) * inv_L;
      const F vy_k = r_k * k.lr;
      const F lam = vmax(__builtin_elementwise_min((s.vx - g.v_lo) * g.inv_span, splat<F>(1.0f)), splat<F>(0.0f));
      const F mu = splat<F>(1.0f) - lam;
      s.vy = lam * s.vy + mu * vy_k;
      s.r = lam * s.r + mu * r_k;
    }
  }
}

// the control step of a kernel instantiated for the default setting (FINE = false: dynamic_advance, as ever) or for
// the others
template <bool FINE, typename F>
__device__ __forceinline__ void dynamic_control_step(StateD_<F>& s, F delta, F pedal, const Vehicle& k, float dt,
                                                     const Integration& g, float inv_L) {
  if constexpr (FINE) dynamic_advance_fine<F>(s, delta, pedal, k, g, inv_L);
  else dynamic_advance<F>(s, delta, pedal, k, dt);
}

// The rate and slip terms of a handle (acmpc_set_dynamics_terms, DESIGN.md section 2 "Mode D", "Rate and slip terms"): per
// control step, after dynamic_cost, the squared rates of the two controls and the squared rear slip ratio
// b = (r lr - vy) / (vx + 1e-3) join a third cost sum E, and their excesses over the limits join V.  The host derives every
// float in float64 and rounds it once; a limit of +inf is no limit.  Two parts, each off (0) when its weights are 0 and
// its limits +inf: a part that is off executes nothing, and with both off the handle launches the kernels it would
// without the setting.  u_prev: the control applied before step 0, [P][2] on the device, or nullptr (step 0's own control
// then stands for it: an increment of +0); not read while the rate part is off.  A kernel argument: SGPRs, and the
// branches on it are scalar.  The kernels take it as a parameter pack `TM... tm` that is empty or one Terms, and touch
// nothing of this under an empty one (`if constexpr`): those are the code they were.  The terms have kernels of their own (the general step of FINE = true plus this), launched
// only when a part is on, and a translation unit of their own (acmpc_dynamic_terms.hip).
struct Terms {
  int rate, slip;
  float inv_dt;                 // float32(1 / dt)
  float hwd, hwp, hws;          // 0.5f * float32(weight): exact
  float rd_max, rp_max, b_max;
  const float* u_prev;
};
__host__ __device__ inline bool has_terms(const Terms& t) { return t.rate != 0 || t.slip != 0; }

// The Terms plus the objective of a handle (acmpc_set_dynamics_objective, DESIGN.md section 2 "Mode D", "Progress and ceiling"): a third
// and a fourth part, off (0) by default like the two above.  A pack type of its own: the kernels instantiated for it hold all
// four parts and run only while the progress or the ceiling part is on; the kernels of a plain Terms stay the code they were
// (inside them the two new parts cost the one-per-lane sampled rollouts a wave per SIMD).  progress: the cost ends with J = fma(nwp, s, J), s the arc
// length made good at the last control step - fma(s_j, Y, fma(c_j, X, q_j)) on the nearest waypoint j that step's
// dynamic_cost used - and nwp = -float32(progress_weight): the only cost term that is not a square, so J may be negative.
// ceiling: per control step the excess of vx over cap = fma(cs, v_ref_j, co) joins V, after the rate and slip lines.
struct TermsObjective : Terms {
  int progress, ceiling;
  float nwp, cs, co;
  const float* q;               // the progress table [P][n] on the device (the host derives it from the packed rows)
};
__host__ __device__ inline bool has_objective(const TermsObjective& t) { return t.progress != 0 || t.ceiling != 0; }

// The TermsObjective plus the tyre coupling of a handle (acmpc_set_dynamics_coupling, DESIGN.md section 2 "Mode D, tyre
// coupling"): a pack type of its own again.  The kernels instantiated for it hold the general step with the coupling block in
// every sub-step and all four term parts behind their scalar switches (any of them may be off), and run only while `coupled`
// is set; every other kernel stays the code it was.  The launchers take the handle's settings as one of these.
struct TermsCoupled : TermsObjective {
  float rho_f, rho_r;
  int coupled;                  // 0: off (rho_f, rho_r not read); the kernels do not read it
};
__host__ __device__ inline bool has_coupling(const TermsCoupled& t) { return t.coupled != 0; }

// The TermsCoupled plus the load transfer of a handle (acmpc_set_dynamics_load_transfer, DESIGN.md section 2 "Mode D, load
// transfer"): a fourth pack type.  The six scalars of LoadedPeaks per vehicle, indexed by the wave-uniform vehicle index as
// Integration::inv_L is.  The kernels instantiated for it (acmpc_dynamic_loaded.hip) run only while `loaded` is set, with
// rho = +inf on both axles while the coupling is off; every other kernel stays the code it was.  The launchers take the
// handle's settings as one of these.
struct TermsLoaded : TermsCoupled {
  float c_h[kMaxVehicles], w_max[kMaxVehicles];
  float a1_f[kMaxVehicles], a2_f[kMaxVehicles], a1_r[kMaxVehicles], a2_r[kMaxVehicles];
  int loaded;                   // 0: off (the arrays not read); the kernels do not read it
};
__host__ __device__ inline bool has_load_transfer(const TermsLoaded& t) { return t.loaded != 0; }

// The TermsLoaded plus the downforce of a handle (acmpc_set_dynamics_downforce, DESIGN.md section 2 "Mode D, downforce"): a fifth
// pack type.  The three floats of AeroPeaks are the handle's, not a vehicle's.  The kernels instantiated for it
// (acmpc_dynamic_aero.hip) run only while `aero` is set, with c_h = w_max = 0 while the load transfer is off (the per-vehicle a1,
// a2 are derived all the same) and rho = +inf while the coupling is off; every other kernel stays the code it was.  The
// launchers take the handle's settings as one of these.
struct TermsAero : TermsLoaded {
  float k_f, k_r, v_sat;
  int aero;                     // 0: off (the three floats not read); the kernels do not read it
};
__host__ __device__ inline bool has_downforce(const TermsAero& t) { return t.aero != 0; }

// The TermsAero plus the surface table of a handle (acmpc_set_surface, DESIGN.md section 2 "Mode D, surface"): a sixth pack type.
// mu [P][n][2] = (mu_f, mu_r) per waypoint, on the device; control step i of a candidate runs all its sub-steps on the peaks
// Pf mu_f[j], Pr mu_r[j], j the nearest waypoint of step i - 1 (waypoint 0 before step 0): the scale lags the position by one
// control step.  The kernels instantiated for it (acmpc_dynamic_surface.hip) run only while `surface` is set, always with the
// aero step: c_h = w_max = 0 while the load transfer is off, rho = +inf while the coupling is off, k_f = k_r = 0 with a finite
// v_sat while the downforce is off (the per-vehicle a1, a2 are derived all the same); every other kernel stays the code it was.
// The launchers take the handle's settings as one of these (under the obstacles' pack, below).
struct TermsSurface : TermsAero {
  const float* mu;
  int surface;                  // 0: off (mu not read); the kernels do not read it
  int mu_P, mu_n;               // what mu was set for: the launchers refuse another shape (the kernels do not read them)
};
__host__ __device__ inline bool has_surface(const TermsSurface& t) { return t.surface != 0; }

// The TermsSurface plus the road table of a handle (acmpc_set_road, DESIGN.md section 2 "Mode D, road"): a seventh pack type.
// road_rows [P][n][4] = (a_x, a_y, n_z, 0) per waypoint, on the device, a row 16 bytes and aligned so; control step i of a
// candidate runs all its sub-steps on the peaks (Pf mu_f[j]) n_z[j], (Pr mu_r[j]) n_z[j] - the mu multiply only while `surface`
// is set, a scalar switch - and adds a_x[j] to xd3 and a_y[j] to xd4 in every sub-step, j the nearest waypoint of step i - 1
// (waypoint 0 before step 0): the surface table's lag.  The kernels instantiated for it (acmpc_dynamic_road.hip,
// acmpc_dynamic_road_actuator.hip) run only while `road` is set, always with the aero step at the neutral values of the tiers that
// are off (as under the surface); every other kernel stays the code it was.  The launchers take the handle's settings as one of
// these (under the obstacles' and the actuator's packs, below).
struct TermsRoad : TermsSurface {
  const float* road_rows;
  int road;                     // 0: off (road_rows not read); the kernels do not read it
  int road_P, road_n;           // what road_rows was set for: the launchers refuse another shape (the kernels do not read them)
};
__host__ __device__ inline bool has_road(const TermsRoad& t) { return t.road != 0; }

// Moving obstacles of a handle (acmpc_set_obstacles, acmpc_set_dynamics_clearance; DESIGN.md section 2 "Mode D, obstacles"): up
// to kMaxObstacles discs per problem, each with a position per control step - row i is where the discs are at the state AFTER
// control step i, the state that step's dynamic_cost sees - and a radius with the ego's folded in.  Per step, after the ceiling
// line, disc k's penetration depth joins V (the hard part, on while K > 0) and its depth into the margin joins E (the soft part,
// on while K > 0 and the weight is not 0).  A pack type again, over the pack of the step the handle would take without obstacles
// (TermsObjective: the general step, TermsCoupled, TermsLoaded, TermsAero; TermsSurface: acmpc_dynamic_surface.hip): the kernels instantiated for the four (acmpc_dynamic_obstacles
// .hip) run only while obstacles are set, every other kernel stays the code it was.  obs [P][n][K][2] in the caller's frame and
// radii [P][K] are read from global memory (problem and step are uniform in every kernel: one broadcast per step, no LDS).
// coef: the packed rows of the launch (the first two floats of a problem's are the origin of the path's own frame,
// start_temporal); the launchers set it from their arguments, the handle leaves it null.
constexpr int kMaxObstacles = 8;   // ACMPC_MAX_OBSTACLES
template <typename Base>
struct WithObstacles : Base {
  const float* obs;
  const float* radii;
  const float* coef;
  int K;                        // 0: none set (nothing else of this is read)
  int soft;                     // 0: the soft part is off (hwo, mg not read)
  int P, n;                     // what obs and radii were set for: the launchers refuse another shape
  float hwo, mg;                // 0.5f * float32(weight): exact; float32(margin)
};
template <typename Base>
__host__ __device__ inline bool has_obstacles(const WithObstacles<Base>& t) { return t.K != 0; }
template <typename TT>
struct PackBase { using type = TT; };
template <typename Base>
struct PackBase<WithObstacles<Base>> { using type = Base; };
// the obstacles' pack over another base (the handle's settings are a WithObstacles<TermsRoad> under the actuator's pack)
template <typename Base, typename From>
inline WithObstacles<Base> obstacles_over(const WithObstacles<From>& t) {
  WithObstacles<Base> r{};
  static_cast<Base&>(r) = static_cast<const Base&>(t);
  r.obs = t.obs;
  r.radii = t.radii;
  r.coef = t.coef;
  r.K = t.K;
  r.soft = t.soft;
  r.P = t.P;
  r.n = t.n;
  r.hwo = t.hwo;
  r.mg = t.mg;
  return r;
}
// whether the soft part adds to E: false for every pack without obstacles (a constant: their finish stays the code it was)
template <typename TT>
__device__ __forceinline__ bool soft_part(const TT&) { return false; }
template <typename Base>
__device__ __forceinline__ bool soft_part(const WithObstacles<Base>& t) { return t.soft != 0; }

// The actuator lag of a handle (acmpc_set_dynamics_actuator, acmpc_set_actuator_state; DESIGN.md section 2 "Mode D, actuator"):
// the steering rack and the pedal follow their commands as first-order lags.  Per channel the host derives k = exp(-dt / tau) -
// what is left of an error after one control step - and m = (tau / dt)(1 - k) - the mean of what is left over the step - in
// float64 and rounds each once (tau = 0: k = m = 0).  A candidate carries the two actuator positions (ActuatorState); at the top
// of control step i, in float32 and unfused,
//   e = delta_i - a_d;   delta_x = delta_i - m_d e;   a_d = delta_i - k_d e          (the pedal channel likewise)
// and the control step - control_terms, every sub-step, the blend's tan(delta) - is driven on (delta_x, pedal_x); dynamic_cost,
// the terms, the records and the sampler stay on the command.  a0 [P][2]: the positions at the start of the plan, on the
// device, or nullptr (step 0's own command then stands for them: e = +0, as with Terms::u_prev).  A wrapper pack like the
// obstacles', over the packs of the top-tier step (TermsAero, TermsSurface, each with or without the obstacles' pack; TermsRoad
// likewise: acmpc_dynamic_road_actuator.hip): the kernels instantiated for the four (acmpc_dynamic_actuator.hip) run only while
// `actuator` is set, with the lower tiers' neutral values where a tier is off (as under the surface); every other kernel stays
// the code it was.  The launchers take the handle's settings as a WithActuator<WithObstacles<TermsRoad>>.
struct ActuatorLag {
  float k_d, m_d, k_p, m_p;
  const float* a0;
  int actuator;                 // 0: off (nothing else of this is read); the kernels do not read it
  int a0_P;                     // what a0 was set for: the launchers refuse another P (the kernels do not read it)
};
template <typename Base>
struct WithActuator : Base {
  ActuatorLag lag;
};
template <typename Base>
__host__ __device__ inline bool has_actuator(const WithActuator<Base>& t) { return t.lag.actuator != 0; }
template <typename Base>
struct PackBase<WithActuator<Base>> { using type = typename PackBase<Base>::type; };   // (sees through both wrappers)
template <typename TT>
struct IsActuatorPack : std::false_type {};
template <typename Base>
struct IsActuatorPack<WithActuator<Base>> : std::true_type {};
template <typename... TM>
constexpr bool kActuatorPack = (IsActuatorPack<typename std::remove_cv<TM>::type>::value || ...);
// the actuator's pack over a base of the handle's settings (TermsAero, TermsSurface), and over the obstacles' pack of one
template <typename Base, typename From>
inline WithActuator<Base> actuator_over(const WithActuator<From>& t) {
  WithActuator<Base> r{};
  static_cast<Base&>(r) = static_cast<const Base&>(t);
  r.lag = t.lag;
  return r;
}
template <typename Base, typename From>
inline WithActuator<WithObstacles<Base>> actuator_over_obstacles(const WithActuator<WithObstacles<From>>& t, const float* coef) {
  WithActuator<WithObstacles<Base>> r{};
  static_cast<WithObstacles<Base>&>(r) = obstacles_over<Base>(t);
  r.coef = coef;
  r.lag = t.lag;
  return r;
}

// what the terms carry from step to step: the previous step's control and the cost sum
template <typename F>
struct TermsState {
  F pd, pp, E;
  typename IndexOf<F>::type j;   // the last control step's nearest waypoint, where the step loop is not the kernel's own
};
template <typename F>
__device__ __forceinline__ TermsState<F> start_terms(int p, const Terms& t) {
  TermsState<F> ts{splat<F>(0.0f), splat<F>(0.0f), splat<F>(0.0f), typename IndexOf<F>::type(0)};
  if (t.rate != 0 && t.u_prev != nullptr) {   // (a wave-uniform address: one scalar load per wave)
    ts.pd = splat<F>(t.u_prev[2 * p]);
    ts.pp = splat<F>(t.u_prev[2 * p + 1]);
  }
  return ts;
}

// `state_of(ts, tm)..., tm...` hands a function the state and the Terms where the pack holds them, nothing where it is empty
template <typename F>
__device__ __forceinline__ TermsState<F>& state_of(TermsState<F>& ts, const Terms&) {
  return ts;
}

// Whether a kernel's pack (`TM...`, or roll_sampled's `TT...` with the terms' state first) holds a TermsCoupled (or the obstacles'
// pack over one: PackBase sees through it), and the peak
// source its control step then takes: dynamic_advance_fine<F, CoupledPeaks<VehiclePeaks>>(..., coupled_peaks(tm...))
template <typename... TM>
constexpr bool kCoupledPack = (std::is_same<typename PackBase<typename std::remove_cv<TM>::type>::type, TermsCoupled>::value || ...);
__device__ __forceinline__ CoupledPeaks<VehiclePeaks> coupled_peaks(const TermsCoupled& t) {
  return CoupledPeaks<VehiclePeaks>{{}, t.rho_f, t.rho_r};
}
template <typename F>
__device__ __forceinline__ CoupledPeaks<VehiclePeaks> coupled_peaks(const TermsState<F>&, const TermsCoupled& t) {
  return coupled_peaks(t);
}

// The same for a TermsLoaded: dynamic_advance_fine<F, LoadedPeaks<VehiclePeaks>>(..., loaded_peaks(vk, tm...)), vk the
// wave-uniform index of the vehicle rolled
template <typename... TM>
constexpr bool kLoadedPack = (std::is_same<typename PackBase<typename std::remove_cv<TM>::type>::type, TermsLoaded>::value || ...);
__device__ __forceinline__ LoadedPeaks<VehiclePeaks> loaded_peaks(int vk, const TermsLoaded& t) {
  return LoadedPeaks<VehiclePeaks>{{{}, t.rho_f, t.rho_r}, t.c_h[vk], t.w_max[vk], t.a1_f[vk], t.a2_f[vk], t.a1_r[vk], t.a2_r[vk]};
}
template <typename F>
__device__ __forceinline__ LoadedPeaks<VehiclePeaks> loaded_peaks(int vk, const TermsState<F>&, const TermsLoaded& t) {
  return loaded_peaks(vk, t);
}

// And for a TermsAero: dynamic_advance_fine<F, AeroPeaks<VehiclePeaks>>(..., aero_peaks(vk, tm...))
template <typename... TM>
constexpr bool kAeroPack = (std::is_same<typename PackBase<typename std::remove_cv<TM>::type>::type, TermsAero>::value || ...);
__device__ __forceinline__ AeroPeaks<VehiclePeaks> aero_peaks(int vk, const TermsAero& t) {
  return AeroPeaks<VehiclePeaks>{{{{}, t.rho_f, t.rho_r}, t.c_h[vk], t.w_max[vk], t.a1_f[vk], t.a2_f[vk], t.a1_r[vk], t.a2_r[vk]},
                                 t.k_f, t.k_r, t.v_sat};
}
template <typename F>
__device__ __forceinline__ AeroPeaks<VehiclePeaks> aero_peaks(int vk, const TermsState<F>&, const TermsAero& t) {
  return aero_peaks(vk, t);
}

// And for a TermsSurface: dynamic_advance_fine<F, AeroPeaks<SurfacePeaks<F>>>(..., surface_peaks<F>(aero_peaks(vk, tm...), veh, p, n,
// j, tm...)) at the top of every control step, j the nearest waypoint(s) of the step before.  One 8-byte load from global
// memory per candidate (the table is read as the progress table and the obstacles' rows are: no LDS) and two multiplies;
// 0 <= j < n always, so there is no bounds code.  Where j is wave-uniform (the finalize, the trace) the load is a scalar one.
template <typename... TM>
constexpr bool kSurfacePack = (std::is_same<typename PackBase<typename std::remove_cv<TM>::type>::type, TermsSurface>::value || ...);
__device__ __forceinline__ void gather_scales(const float* mu, int j, float& mf, float& mr) {
  const f32x2 m = *reinterpret_cast<const f32x2*>(mu + 2 * static_cast<size_t>(j));
  mf = m[0];
  mr = m[1];
}
__device__ __forceinline__ void gather_scales(const float* mu, i32x2 j, f32x2& mf, f32x2& mr) {
  const f32x2 m0 = *reinterpret_cast<const f32x2*>(mu + 2 * static_cast<size_t>(j[0]));
  const f32x2 m1 = *reinterpret_cast<const f32x2*>(mu + 2 * static_cast<size_t>(j[1]));
  mf = f32x2{m0[0], m1[0]};
  mr = f32x2{m0[1], m1[1]};
}
// the scales of problem p's waypoint(s) j: issued ahead of the control's load or draw, multiplied in by surface_peaks
template <typename F>
struct SurfaceScales {
  F mf, mr;
};
template <typename F>
__device__ __forceinline__ SurfaceScales<F> surface_scales(int p, int n, typename IndexOf<F>::type j, const TermsSurface& t) {
  SurfaceScales<F> m;
  gather_scales(t.mu + static_cast<size_t>(p) * n * 2, j, m.mf, m.mr);
  return m;
}
template <typename F>
__device__ __forceinline__ SurfaceScales<F> surface_scales(int p, int n, typename IndexOf<F>::type j, const TermsState<F>&,
                                                           const TermsSurface& t) {
  return surface_scales<F>(p, n, j, t);
}
// Pf_s = Pf mu_f, Pr_s = Pr mu_r - one float32 multiply each, once per control step - in front of the scalars `a` of the vehicle
template <typename F>
__device__ __forceinline__ AeroPeaks<SurfacePeaks<F>> surface_peaks(const AeroPeaks<VehiclePeaks>& a, const Vehicle& k,
                                                                    const SurfaceScales<F>& m) {
  AeroPeaks<SurfacePeaks<F>> pk;
  pk.Pf = k.Pf * m.mf;
  pk.Pr = k.Pr * m.mr;
  pk.rho_f = a.rho_f;
  pk.rho_r = a.rho_r;
  pk.c_h = a.c_h;
  pk.w_max = a.w_max;
  pk.a1_f = a.a1_f;
  pk.a2_f = a.a2_f;
  pk.a1_r = a.a1_r;
  pk.a2_r = a.a2_r;
  pk.k_f = a.k_f;
  pk.k_r = a.k_r;
  pk.v_sat = a.v_sat;
  return pk;
}

// And for a TermsRoad: dynamic_advance_fine<F, RoadPeaks<F>>(..., road_peaks<F>(aero_peaks(vk, tm...), veh, road_row<F>(p, n, j,
// tm...))), at the top of every control step as above.  One aligned 16-byte load from global memory per candidate (two under
// f32x2; a scalar load where j is wave-uniform), no LDS, no bounds code (0 <= j < n), and - while a surface table is set, a scalar
// switch on the kernel argument - the surface's 8-byte load beside it.  Nothing per vehicle: the row is the road's.
template <typename... TM>
constexpr bool kRoadPack = (std::is_same<typename PackBase<typename std::remove_cv<TM>::type>::type, TermsRoad>::value || ...);
__device__ __forceinline__ void gather_road(const float* rows, int j, float& ax, float& ay, float& nz) {
  const f32x4 m = *reinterpret_cast<const f32x4*>(rows + 4 * static_cast<size_t>(j));
  ax = m[0];
  ay = m[1];
  nz = m[2];
}
__device__ __forceinline__ void gather_road(const float* rows, i32x2 j, f32x2& ax, f32x2& ay, f32x2& nz) {
  const f32x4 m0 = *reinterpret_cast<const f32x4*>(rows + 4 * static_cast<size_t>(j[0]));
  const f32x4 m1 = *reinterpret_cast<const f32x4*>(rows + 4 * static_cast<size_t>(j[1]));
  ax = f32x2{m0[0], m1[0]};
  ay = f32x2{m0[1], m1[1]};
  nz = f32x2{m0[2], m1[2]};
}
// the road row of problem p's waypoint(s) j, and the grip scales there (ones while no surface table is set: Pf 1 = Pf bit for
// bit): issued ahead of the control's load or draw, multiplied in by road_peaks
template <typename F>
struct RoadRow {
  F mf, mr, ax, ay, nz;
};
template <typename F>
__device__ __forceinline__ RoadRow<F> road_row(int p, int n, typename IndexOf<F>::type j, const TermsRoad& t) {
  RoadRow<F> m;
  m.mf = m.mr = splat<F>(1.0f);
  if (t.surface != 0) gather_scales(t.mu + static_cast<size_t>(p) * n * 2, j, m.mf, m.mr);
  gather_road(t.road_rows + static_cast<size_t>(p) * n * 4, j, m.ax, m.ay, m.nz);
  return m;
}
template <typename F>
__device__ __forceinline__ RoadRow<F> road_row(int p, int n, typename IndexOf<F>::type j, const TermsState<F>&, const TermsRoad& t) {
  return road_row<F>(p, n, j, t);
}
// Pf_r = (Pf mu_f) n_z, Pr_r = (Pr mu_r) n_z - one float32 multiply each for the surface and one for the road, once per control
// step - in front of the scalars `a` of the vehicle, with the row's two accelerations
template <typename F>
__device__ __forceinline__ RoadPeaks<F> road_peaks(const AeroPeaks<VehiclePeaks>& a, const Vehicle& k, const RoadRow<F>& m) {
  RoadPeaks<F> pk;
  pk.Pf = (k.Pf * m.mf) * m.nz;
  pk.Pr = (k.Pr * m.mr) * m.nz;
  pk.rho_f = a.rho_f;
  pk.rho_r = a.rho_r;
  pk.c_h = a.c_h;
  pk.w_max = a.w_max;
  pk.a1_f = a.a1_f;
  pk.a2_f = a.a2_f;
  pk.a1_r = a.a1_r;
  pk.a2_r = a.a2_r;
  pk.k_f = a.k_f;
  pk.k_r = a.k_r;
  pk.v_sat = a.v_sat;
  pk.ax = m.ax;
  pk.ay = m.ay;
  return pk;
}
// the handle's settings without the road table: what every launcher from before the road takes
inline WithActuator<WithObstacles<TermsSurface>> below_road(const WithActuator<WithObstacles<TermsRoad>>& t) {
  WithActuator<WithObstacles<TermsSurface>> r{};
  static_cast<WithObstacles<TermsSurface>&>(r) = obstacles_over<TermsSurface>(t);
  r.lag = t.lag;
  return r;
}

// one float of the staged waypoint row(s) j, or of a table of one float per waypoint (stride 1)
__device__ __forceinline__ float gather_float(const float* t, int j, int stride, int e) { return t[j * stride + e]; }
__device__ __forceinline__ f32x2 gather_float(const float* t, i32x2 j, int stride, int e) {
  return f32x2{t[j[0] * stride + e], t[j[1] * stride + e]};
}

template <typename F>
__device__ __forceinline__ void keep_nearest(typename IndexOf<F>::type j, TermsState<F>& ts, const Terms&) {
  ts.j = j;
}

// the terms of control step i of problem p, on the state the step's dynamic_cost saw; wp, j: the staged rows and the
// nearest waypoint(s) that dynamic_cost used (the ceiling reads v_ref_j, float 5 of the row, again)
template <typename F, typename TT>
__device__ __forceinline__ void dynamic_terms(StateD_<F>& s, F delta, F pedal, int i, [[maybe_unused]] int p, const Vehicle& k,
                                              [[maybe_unused]] const float* wp, [[maybe_unused]] typename IndexOf<F>::type j,
                                              TermsState<F>& ts, const TT& t) {
  const bool first = i == 0;
  if (t.rate != 0) {
    const bool own = first && t.u_prev == nullptr;
    const F pd = own ? delta : ts.pd;
    const F pp = own ? pedal : ts.pp;
    const F rd = (delta - pd) * t.inv_dt;
    const F rp = (pedal - pp) * t.inv_dt;
    ts.E = fma_(t.hwd * rd, rd, ts.E);
    ts.E = fma_(t.hwp * rp, rp, ts.E);
    const F hd = vmax(abs_(rd) - t.rd_max, splat<F>(0.0f));
    s.t.V = fma_(hd, hd, s.t.V);
    const F hp = vmax(abs_(rp) - t.rp_max, splat<F>(0.0f));
    s.t.V = fma_(hp, hp, s.t.V);
    ts.pd = delta;
    ts.pp = pedal;
  }
  if (t.slip != 0) {
    const F b = (s.r * k.lr - s.vy) / (s.vx + kVxEps);   // dynamic_euler's qr, on the updated state
    ts.E = fma_(t.hws * b, b, ts.E);
    const F hb = vmax(abs_(b) - t.b_max, splat<F>(0.0f));
    s.t.V = fma_(hb, hb, s.t.V);
  }
  if constexpr (std::is_base_of<TermsObjective, TT>::value) {
    if (t.ceiling == 0) return;
    const F cap = fma_(splat<F>(t.cs), gather_float(wp, j, kCoefT, 5), splat<F>(t.co));
    const F h = vmax(s.vx - cap, splat<F>(0.0f));   // (maxNum: a NaN v_ref is no ceiling)
    s.t.V = fma_(h, h, s.t.V);
  }
}

// The same under the obstacles' pack: the base pack's terms, then the discs in k order on a kernel argument - a scalar loop, no
// divergence.  Spec order: ox = o_x - x_0 (one subtraction), dx = X - ox, d = sqrt(fma(dy, dy, dx dx)), h = max(R - d, 0),
// V = fma(h, h, V); and while the soft part is on g = max((R + mg) - d, 0), E = fma(hwo g, g, E).  max is maxNum: a NaN or
// infinite coordinate gives h = g = 0 - that disc does not exist at that step.  Problem and step are wave-uniform: lane k of the
// wave loads disc k of the step's row (one 8-byte load and the radius; the lanes past K - 1 repeat the last disc) and the loop
// broadcasts lane k's three floats with v_readlane - one load's latency per step, not K scalar ones, and nothing of the row in
// the SGPRs, which the step loop has none to spare of.
template <typename F, typename Base>
__device__ __forceinline__ void dynamic_terms(StateD_<F>& s, F delta, F pedal, int i, int p, const Vehicle& k, const float* wp,
                                              typename IndexOf<F>::type j, TermsState<F>& ts, const WithObstacles<Base>& t) {
  const float* __restrict__ coef = t.coef + static_cast<size_t>(p) * t.n * kCoefT;
  const int mine = min(static_cast<int>(__lane_id()), t.K - 1);   // (issued ahead of the base pack's terms: the load's latency)
  const f32x2 at = *reinterpret_cast<const f32x2*>(t.obs + ((static_cast<size_t>(p) * t.n + i) * t.K + mine) * 2);
  const int ox_l = __float_as_int(at[0] - coef[0]), oy_l = __float_as_int(at[1] - coef[1]);
  const int R_l = __float_as_int(t.radii[static_cast<size_t>(p) * t.K + mine]);
  dynamic_terms<F, Base>(s, delta, pedal, i, p, k, wp, j, ts, static_cast<const Base&>(t));
#pragma nounroll
  for (int q = 0; q < t.K; ++q) {
    const float ox = __int_as_float(__builtin_amdgcn_readlane(ox_l, q)), oy = __int_as_float(__builtin_amdgcn_readlane(oy_l, q));
    const float R = __int_as_float(__builtin_amdgcn_readlane(R_l, q));
    const F dx = s.t.X - splat<F>(ox), dy = s.t.Y - splat<F>(oy);
    const F d = sqrt_(fma_(dy, dy, dx * dx));
    const F h = vmax(splat<F>(R) - d, splat<F>(0.0f));
    s.t.V = fma_(h, h, s.t.V);
    if (t.soft != 0) {
      const F g = vmax(splat<F>(R + t.mg) - d, splat<F>(0.0f));
      ts.E = fma_(t.hwo * g, g, ts.E);
    }
  }
}

// finish_temporal (acmpc_device.h) with the terms: stage = stage + E after the last weighted sum when the rate or the slip
// part is on (under a plain Terms one of them is) or the obstacles' soft part is, and J = fma(nwp, s, J) between J = stage + a and the violations' fma when the progress part is on.  wp, j: the
// staged rows and the nearest waypoint(s) of the last control step; p: the problem, whose row of the progress table is read
// from global memory (one gather per candidate).
template <typename F, typename TT>
__device__ __forceinline__ F finish_dynamic_terms(const StateD_<F>& s, const TermsState<F>& ts, [[maybe_unused]] const float* wp,
                                                  [[maybe_unused]] typename IndexOf<F>::type j, [[maybe_unused]] int p, int n,
                                                  const Weights& w, const TT& t) {
  constexpr bool kObjective = std::is_base_of<TermsObjective, TT>::value;
  const StateT_<F>& st = s.t;
  const float tN = static_cast<float>(n) * w.dt;
  F stage = splat<F>(w.hq0) * st.S0;
  stage = fma_(splat<F>(w.hq1), st.S1, stage);
  stage = fma_(splat<F>(w.hr0), st.S2, stage);
  stage = fma_(splat<F>(w.hr1), st.S3, stage);
  if (!kObjective || t.rate != 0 || t.slip != 0 || soft_part(t)) stage = stage + ts.E;
  F a = (w.hqn0 * st.ey) * st.ey;
  a = fma_(w.hqn1 * st.ep, st.ep, a);
  a = fma_(splat<F>(w.hqn2 * tN), splat<F>(tN), a);
  F J = stage + a;
  if constexpr (kObjective) {
    if (t.progress == 0) return fma_(splat<F>(w.wbound), st.V, J);
    const F sj = -gather_float(wp, j, kCoefT, 1);   // the row holds -sin psi_j: the negation is exact
    const F cj = gather_float(wp, j, kCoefT, 2);
    const F qj = gather_float(t.q + static_cast<size_t>(p) * n, j, 1, 0);
    const F prog = fma_(sj, st.Y, fma_(cj, st.X, qj));
    J = fma_(splat<F>(t.nwp), prog, J);
  }
  return fma_(splat<F>(w.wbound), st.V, J);
}

// Under the actuator's pack the terms and the finish are the base pack's, on the COMMAND (the rates, the box and dk belong to
// what the optimiser chooses); the lag touches the control step alone (actuator_step, below).
template <typename F, typename Base>
__device__ __forceinline__ void dynamic_terms(StateD_<F>& s, F delta, F pedal, int i, int p, const Vehicle& k, const float* wp,
                                              typename IndexOf<F>::type j, TermsState<F>& ts, const WithActuator<Base>& t) {
  dynamic_terms<F>(s, delta, pedal, i, p, k, wp, j, ts, static_cast<const Base&>(t));
}
template <typename F, typename Base>
__device__ __forceinline__ F finish_dynamic_terms(const StateD_<F>& s, const TermsState<F>& ts, const float* wp,
                                                  typename IndexOf<F>::type j, int p, int n, const Weights& w,
                                                  const WithActuator<Base>& t) {
  return finish_dynamic_terms<F>(s, ts, wp, j, p, n, w, static_cast<const Base&>(t));
}

// The two actuator positions a candidate carries under a WithActuator pack, a state of its own beside TermsState (which stays
// what the other packs' kernels were compiled with): a0[p] where the caller gave the measured positions - a wave-uniform address,
// one scalar load ahead of the step loop - else whatever, replaced by step 0's command inside actuator_step.
template <typename F>
struct ActuatorState {
  F a_d, a_p;
};
template <typename Base>
__device__ __forceinline__ const ActuatorLag& lag_of(const WithActuator<Base>& t) {
  return t.lag;
}
template <typename F, typename Base>
__device__ __forceinline__ const ActuatorLag& lag_of(const TermsState<F>&, const WithActuator<Base>& t) {
  return t.lag;
}
template <typename F>
__device__ __forceinline__ ActuatorState<F> start_actuator(int p, const ActuatorLag& t) {
  ActuatorState<F> as{splat<F>(0.0f), splat<F>(0.0f)};
  if (t.a0 != nullptr) {
    as.a_d = splat<F>(t.a0[2 * p]);
    as.a_p = splat<F>(t.a0[2 * p + 1]);
  }
  return as;
}
// The top of control step i: the applied control (dx, qx) of the command (delta, pedal) - the interval mean of the exact
// first-order response to a held command - and the positions at the step's end (the exact zero-order-hold discretisation).
// Three float32 operations per channel, none fused; k, m and the a0 switch are scalars.
template <typename F>
__device__ __forceinline__ void actuator_step(int i, F delta, F pedal, ActuatorState<F>& as, const ActuatorLag& t, F& dx, F& qx) {
  const bool own = i == 0 && t.a0 == nullptr;
  const F ad = own ? delta : as.a_d;
  const F ap = own ? pedal : as.a_p;
  const F ed = delta - ad;
  const F ep = pedal - ap;
  dx = delta - t.m_d * ed;
  qx = pedal - t.m_p * ep;
  as.a_d = delta - t.k_d * ed;
  as.a_p = pedal - t.k_p * ep;
}

// mode T's temporal_cost with the input terms of this model: dv = vx - v_ref, dk = delta - delta_ref (row[7], staged
// once per waypoint), the input box on (delta, pedal).  g = a derived waypoint row (stage_dynamic_tables).
template <typename F>
__device__ __forceinline__ void dynamic_cost(StateD_<F>& s, const F (&g)[kCoefT], F delta, F pedal, const Weights& w) {
  StateT_<F>& t = s.t;
  t.ey = fma_(g[2], t.Y, fma_(g[1], t.X, g[0]));
  t.ep = wrap_spec<F>(t.phi - g[3]);
  const F dv = s.vx - g[5];
  const F dk = delta - g[7];
  t.S0 = fma_(t.ey, t.ey, t.S0);
  t.S1 = fma_(t.ep, t.ep, t.S1);
  t.S2 = fma_(dv, dv, t.S2);
  t.S3 = fma_(dk, dk, t.S3);
  const F hd = delta - med3_(delta, splat<F>(w.ulo0), splat<F>(w.uhi0));
  t.V = fma_(hd, hd, t.V);
  const F hp = pedal - med3_(pedal, splat<F>(w.ulo1), splat<F>(w.uhi1));
  t.V = fma_(hp, hp, t.V);
  const F hc = vmax(abs_(t.ey) - g[6], splat<F>(0.0f));
  t.V = fma_(hc, hc, t.V);
}

// mode T's tables (stage_temporal_tables) with delta_ref = atan_spec(wheelbase * k_ref) in the row's eighth float
__device__ __forceinline__ void stage_dynamic_tables(const float* __restrict__ coef, int n, int tid, int threads,
                                                     float wheelbase, float* rows, float* abc) {
  stage_temporal_tables(coef, n, tid, threads, rows, abc);
  for (int m = tid; m < n; m += threads) rows[m * kCoefT + 7] = atan_spec<float>(wheelbase * coef[m * kCoefT + 5]);
}

// ---- launchers (acmpc_dynamic.hip) ----------------------------------------------------------------------------------
// Candidates per lane of the rollout for a launch of P x N (x K vehicles): two (v_pk_* pairs) once the launch fills the
// chip many times over, one below that (a small solve is latency: more lanes, shorter per-lane work).
int dynamic_candidates_per_lane(int P, int N, int K = 1);
// partial keys per problem of the rollout: one per 256-lane workgroup (K = 1), one per K-wave workgroup of 64 lanes (K > 1)
int dynamic_blocks_per_problem(int P, int N, int K = 1);
// rollout: costs [P][N] (or nullptr) and one (cost, index) partial key + feasible count per workgroup, x0 [P][6].  K = 1:
// rollout_dynamic_kernel with the one vehicle; K > 1: rollout_dynamic_ensemble_kernel.
// `integration`: the handle's setting; the default launches the FINE = false instantiations, whose step loop knows nothing
// of it.
// `terms`: the handle's rate and slip terms and its objective; when any part is on, the kernels that hold them run, with the general step whatever the
// integration setting (the default one as M = 1, no blend, h = float32(dt)).  And its tyre coupling: while that is on, the
// coupled kernels run, whatever the parts.  And its load transfer: while that is on, the loaded kernels run, whatever the
// coupling and the parts.  And its downforce: while that is on, the aero kernels run, whatever the load transfer, the coupling and
// the parts.  And its obstacles: while any are set, the obstacle kernels of the step the handle would take
// without them run (the general, the coupled, the loaded or the aero one), looked at first.  And its surface table: while one is
// set, the surface kernels run (the aero step on per-lane peaks, with or without the obstacles' lines), whatever else is on.
// And its actuator lag: while that is on, the actuator kernels run (the aero or the surface step on the lagged control, with or
// without the obstacles' lines), looked at before everything else but the road.  And its road table: while one is set, the road
// kernels run (the surface step with the road's row, with or without the obstacles' lines and the actuator lag), looked at first.
hipError_t launch_rollout_dynamic(int layout, const RolloutArgs& args, const VehicleEnsemble& vehicles,
                                  const Integration& integration, const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);
// the same rollout with the candidates drawn inside the kernel instead of read from args.U (which is ignored): candidate
// index_offset + c of problem p is what launch_sample would write for `sample` - centre, u_ref, centre_stride, spec (seed or
// seed_ptr, round, sigmas = (sigma_delta, sigma_pedal), segments); P / N / n / index_offset must be the rollout's, the spec's
// input box the Weights', u_extra null (hipErrorInvalidValue otherwise).  Same launch shapes, costs, partial keys and counts.
hipError_t launch_rollout_dynamic_sampled(const RolloutArgs& args, const SampleArgs& sample, const VehicleEnsemble& vehicles,
                                          const Integration& integration, const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);
// argmin over the partial keys (or keys_in), keys_out, and the winner's record re-rolled from U: header, u = (delta,
// pedal), x = (X, Y, yaw) in the caller's frame (under vehicle 0).  Reads args.U / x0 / coef / partial_* / keys_in /
// index_offset / n / N / P / blocks_per_problem / w.  With `regenerate` the winner's controls are re-drawn from the global
// index in its key (args.centre / centre_stride / u_ref / spec; U and index_offset are not read) and EVERY rank writes the
// complete record, owner = 1, n_feasible = its own count.  `controls_only` is not supported (hipErrorInvalidValue).
hipError_t launch_finalize_dynamic(int layout, const FinalizeArgs& args, const VehicleEnsemble& vehicles,
                                   const Integration& integration, const WithActuator<WithObstacles<TermsRoad>>& terms, hipStream_t s);

}  // namespace acmpc
