// C ABI, mode D's settings (include/acmpc.h).  This unit owns the vehicle blocks and what is derived from them
// (acmpc_set_dynamics*), the integration setting, the rate and slip terms, the objective, the tyre coupling, the load transfer, the downforce, the previous control, the obstacles and the clearance setting, the surface table, the road table, the actuator lag and the actuator positions, and the grip
// identification (acmpc_score_grips) and the plan trace (acmpc_trace_plans), with the checks that the kernels' limits are the public header's.
#include <algorithm>

#include "acmpc_ctx.h"
#include "acmpc_dynamic_trace.h"
#include "acmpc_identify.h"

using namespace acmpc::capi;

namespace {

static_assert(acmpc::kIdentifyMaxSteps == ACMPC_MAX_LOG_STEPS && acmpc::kIdentifyMaxHypotheses == ACMPC_MAX_GRIP_HYPOTHESES,
              "the grip identification's limits of acmpc_identify.h are the header's");
static_assert(acmpc::kMaxObstacles == ACMPC_MAX_OBSTACLES, "the obstacle limit of acmpc_dynamic.h is the header's");
static_assert(acmpc::kMaxSubsteps == ACMPC_MAX_SUBSTEPS, "the sub-step limit of acmpc_dynamic.h is the header's");
static_assert(acmpc::kMaxVehicles == ACMPC_MAX_VEHICLES && acmpc::kEnsembleMean == ACMPC_ENSEMBLE_MEAN &&
                  acmpc::kEnsembleMax == ACMPC_ENSEMBLE_MAX,
              "the ensemble constants of acmpc_dynamic.h are the header's");

// The two axles' peak factors of a vehicle block whose Df and Dr are scaled by (sf, sr) - (1, 1): the block's own - in
// float64, the reference's association, each rounded to float32 once (the block is checked: derive_vehicle)
void derive_peaks(const double* coef, double sf, double sr, float* Pf, float* Pr) {
  const double F_z0 = coef[0], Df = coef[3] * sf, epsf = coef[5], Dr = coef[8] * sr, epsr = coef[10], mass = coef[11],
               g = coef[13], lf = coef[14], lr = coef[15];
  const double F_zf = mass * g * lr / (lr + lf);
  const double F_zr = mass * g * lf / (lr + lf);
  *Pf = static_cast<float>(Df * (1 + epsf * F_zf / F_z0) * F_zf / F_z0);
  *Pr = static_cast<float>(Dr * (1 + epsr * F_zr / F_z0) * F_zr / F_z0);
}

// mode D's float32 constants of one vehicle block (acmpc_set_dynamics): nullptr, or why the block is refused
const char* derive_vehicle(const double* coef, double wheelbase, acmpc::Vehicle* out) {
  for (int q = 0; q < acmpc::kDynamicsCount; ++q)
    if (!std::isfinite(coef[q])) return "non-finite value in the vehicle block";
  const double F_z0 = coef[0], Bf = coef[1], Cf = coef[2], Ef = coef[4], Br = coef[6], Cr = coef[7], Er = coef[9],
               mass = coef[11], Iz = coef[12], lf = coef[14], lr = coef[15], bias = coef[16];
  if (!(mass > 0.0) || !(Iz > 0.0)) return "mass and Iz must be positive";
  if (F_z0 == 0.0 || lr + lf == 0.0) return "F_z0 and lf + lr must not be zero";
  // float64, the reference's association, each constant rounded to float32 once ("Mode D")
  acmpc::Vehicle& v = *out;
  derive_peaks(coef, 1.0, 1.0, &v.Pf, &v.Pr);
  v.lf = static_cast<float>(lf);
  v.lr = static_cast<float>(lr);
  v.Bf = static_cast<float>(Bf);
  v.Cf = static_cast<float>(Cf);
  v.Ef = static_cast<float>(Ef);
  v.Br = static_cast<float>(Br);
  v.Cr = static_cast<float>(Cr);
  v.Er = static_cast<float>(Er);
  v.mass = static_cast<float>(mass);
  v.inv_mass = static_cast<float>(1.0 / mass);
  v.inv_Iz = static_cast<float>(1.0 / Iz);
  v.Cm1 = static_cast<float>(coef[17]);
  v.Cm2 = static_cast<float>(coef[18]);
  v.Cm3 = static_cast<float>(coef[19]);
  v.Cb1 = static_cast<float>(coef[20]);
  v.Cb2 = static_cast<float>(coef[21]);
  v.Cb3 = static_cast<float>(coef[22]);
  v.fric0 = static_cast<float>(-coef[23]);
  v.Cfric2 = static_cast<float>(coef[24]);
  v.Cfric3 = static_cast<float>(coef[25]);
  v.bias_front = static_cast<float>(bias);
  v.bias_rear = static_cast<float>(1 - bias);
  v.wheelbase = static_cast<float>(wheelbase);
  return nullptr;
}

// the tyre coupling divides by rho P: while it is on, every vehicle's two peaks are finite and positive as float32
bool peaks_couple(const acmpc::VehicleEnsemble& e) {
  for (int k = 0; k < e.K; ++k)
    for (float P : {e.v[k].Pf, e.v[k].Pr})
      if (!std::isfinite(P) || !(P > 0.0f)) return false;
  return true;
}
constexpr const char* kPeaksRefused = "the tyre coupling is on: every vehicle's axle peaks Pf, Pr must be finite and > 0 (as float32)";


// What the load transfer reads of a vehicle block in float64: the static axle loads and e_a = eps_a / F_z0
void derive_axles(const double* coef, double* axle) {
  const double F_z0 = coef[0], epsf = coef[5], epsr = coef[10], mass = coef[11], g = coef[13], lf = coef[14], lr = coef[15];
  axle[0] = mass * g * lr / (lr + lf);
  axle[1] = mass * g * lf / (lr + lf);
  axle[2] = epsf / F_z0;
  axle[3] = epsr / F_z0;
}

// The six float32 scalars of one vehicle under the setting (h_cg, w_frac), derived in float64 and rounded once each (include/
// acmpc.h, acmpc_set_dynamics_load_transfer): nullptr, or why the vehicle is refused - N_a = 0, or a factor phi_a that is not
// > 0 (in float64) at x = +-w_max or at its vertex inside.  `aero`: the downforce's (k_f, k_r, v_sat) as the kernels get them, or
// nullptr while it is off (acmpc_set_dynamics_downforce): axle a's interval then ends at w_max + k_a v_sat^2.
const char* derive_load(const double* setting, const float* aero, double L, const double* axle, float* out) {
  const double c_h = setting[0] / L;
  const double w_max = setting[1] * std::min(axle[0], axle[1]);
  if (!std::isfinite(c_h) || !std::isfinite(w_max)) return "the load transfer's c_h or w_max is not finite";
  out[0] = static_cast<float>(c_h);
  out[1] = static_cast<float>(w_max);
  for (int a = 0; a < 2; ++a) {
    const double F = axle[a], e = axle[2 + a];
    const double N = F + e * F * F;
    if (N == 0.0 || !std::isfinite(N)) return "the load transfer divides by N = F_z + e F_z^2, which is 0 or not finite";
    const double a1 = (1 + 2 * e * F) / N, a2 = e / N;
    const double top = aero == nullptr ? w_max : w_max + static_cast<double>(aero[a]) * aero[2] * aero[2];
    if (!std::isfinite(top)) return "the downforce at v_sat is not finite";
    double probe[3] = {-w_max, top, 0.0};
    int probes = 2;
    if (a2 != 0.0) {   // (with a2 < 0 the vertex is the factor's maximum: looked at all the same, it refuses nothing more)
      const double vertex = -a1 / (2 * a2);
      if (vertex > -w_max && vertex < top) probe[probes++] = vertex;
    }
    for (int q = 0; q < probes; ++q)
      if (!(1 + probe[q] * (a1 + a2 * probe[q]) > 0.0))
        return aero == nullptr ? "the load transfer's peak factor phi is not > 0 over +-w_max"
                               : "the peak factor is not > 0 over the load range -w_max .. w_max + k v_sat^2 of the downforce";
    out[2 + 2 * a] = static_cast<float>(a1);
    out[3 + 2 * a] = static_cast<float>(a2);
  }
  return nullptr;
}

// every vehicle of an ensemble under a load transfer (nullptr: off, c_h = w_max = 0) and a downforce (nullptr: off): the scalars
// into out[k], or why one is refused; with both off nothing is derived or refused
const char* derive_loads(const double* setting, const float* aero, const acmpc::VehicleEnsemble& e, const double* L,
                         const double (*axle)[4], float (*out)[6]) {
  if (setting == nullptr && aero == nullptr) return nullptr;
  if (!peaks_couple(e))
    return setting != nullptr ? "the load transfer is on: every vehicle's axle peaks Pf, Pr must be finite and > 0 (as float32)"
                              : "the downforce is on: every vehicle's axle peaks Pf, Pr must be finite and > 0 (as float32)";
  const double none[2] = {0.0, 0.0};
  for (int k = 0; k < e.K; ++k) {
    const char* why = derive_load(setting != nullptr ? setting : none, aero, L[k], axle[k], out[k]);
    if (why != nullptr) return why;
  }
  return nullptr;
}
const double* load_of(const acmpc_ctx* c) { return c->has_load ? c->load_setting : nullptr; }
const float* aero_of(const acmpc_ctx* c) { return c->has_aero ? c->aero : nullptr; }

}  // namespace

namespace acmpc {
namespace capi __attribute__((visibility("hidden"))) {

void surface_load_const(const acmpc_ctx* c, int k, float* out) {
  const double none[2] = {0.0, 0.0};
  float lc[6] = {};
  if (derive_load(none, nullptr, c->vehicle_L[k], c->vehicle_axle[k], lc) != nullptr) std::memset(lc, 0, sizeof lc);
  std::memcpy(out, lc, sizeof lc);
}

}  // namespace capi
}  // namespace acmpc

extern "C" {

int acmpc_set_dynamics(acmpc_ctx* c, const double* coef, int32_t count) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_EINVAL, "acmpc_set_dynamics needs a mode D handle");
  if (coef == nullptr) return fail(c, ACMPC_EINVAL, "null vehicle block");
  if (count != acmpc::kDynamicsCount) return fail(c, ACMPC_EINVAL, "the vehicle block has ACMPC_DYNAMICS_COUNT = 26 values");
  // an ensemble of one (omega_0 = 1, MEAN): the single-vehicle kernels
  acmpc::VehicleEnsemble e{};
  const char* why = derive_vehicle(coef, c->prm.wheelbase, &e.v[0]);
  if (why != nullptr) return fail(c, ACMPC_EINVAL, why);
  e.omega[0] = 1.0f;
  e.K = 1;
  e.reduce = ACMPC_ENSEMBLE_MEAN;
  if (c->has_coupling && !peaks_couple(e)) return fail(c, ACMPC_EINVAL, kPeaksRefused);
  const double L[1] = {coef[14] + coef[15]};
  double axle[1][4];
  float load[1][6] = {};
  derive_axles(coef, axle[0]);
  if (const char* refused = derive_loads(load_of(c), aero_of(c), e, L, axle, load); refused != nullptr)
    return fail(c, ACMPC_EINVAL, refused);
  c->vehicles = e;
  std::memcpy(c->vehicle_axle[0], axle[0], sizeof axle[0]);
  std::memcpy(c->load_const[0], load[0], sizeof load[0]);
  c->vehicle_L[0] = coef[14] + coef[15];
  std::memcpy(c->vehicle0, coef, sizeof c->vehicle0);
  c->has_dynamics = true;
  return ACMPC_OK;
}

int acmpc_set_dynamics_ensemble(acmpc_ctx* c, const double* coef, int32_t K, const double* weights, int32_t reduce) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_EINVAL, "acmpc_set_dynamics_ensemble needs a mode D handle");
  if (coef == nullptr) return fail(c, ACMPC_EINVAL, "null vehicle blocks");
  if (K < 1 || K > ACMPC_MAX_VEHICLES) return fail(c, ACMPC_EINVAL, "an ensemble has 1 .. ACMPC_MAX_VEHICLES = 8 vehicles");
  if (reduce != ACMPC_ENSEMBLE_MEAN && reduce != ACMPC_ENSEMBLE_MAX) return fail(c, ACMPC_EINVAL, "unknown reduce");
  // everything is checked before anything is kept: a refused ensemble leaves the handle's vehicle(s) as they were
  acmpc::VehicleEnsemble e{};
  double total = 0.0;
  for (int k = 0; k < K; ++k) {
    if (weights != nullptr) {
      if (!std::isfinite(weights[k]) || !(weights[k] > 0.0))
        return fail(c, ACMPC_EINVAL, "vehicle " + std::to_string(k) + ": a weight must be finite and positive");
      total += weights[k];
    }
    const char* why = derive_vehicle(coef + static_cast<size_t>(k) * acmpc::kDynamicsCount, c->prm.wheelbase, &e.v[k]);
    if (why != nullptr) return fail(c, ACMPC_EINVAL, "vehicle " + std::to_string(k) + ": " + why);
  }
  if (weights != nullptr && !std::isfinite(total)) return fail(c, ACMPC_EINVAL, "the weights' sum is not finite");
  // omega_k = w_k / sum_j w_j in float64 (the sum in k order), each rounded once; no weights: float32(1 / K)
  for (int k = 0; k < K; ++k)
    e.omega[k] = static_cast<float>(weights != nullptr ? weights[k] / total : 1.0 / K);
  e.K = K;
  e.reduce = reduce;
  if (c->has_coupling && !peaks_couple(e)) return fail(c, ACMPC_EINVAL, kPeaksRefused);
  double L[acmpc::kMaxVehicles], axle[acmpc::kMaxVehicles][4];
  float load[acmpc::kMaxVehicles][6] = {};
  for (int k = 0; k < K; ++k) {
    const double* ck = coef + static_cast<size_t>(k) * acmpc::kDynamicsCount;
    L[k] = ck[14] + ck[15];
    derive_axles(ck, axle[k]);
  }
  if (const char* refused = derive_loads(load_of(c), aero_of(c), e, L, axle, load); refused != nullptr)
    return fail(c, ACMPC_EINVAL, refused);
  c->vehicles = e;
  std::memcpy(c->vehicle_axle, axle, sizeof(double) * 4 * K);
  std::memcpy(c->load_const, load, sizeof(float) * 6 * K);
  for (int k = 0; k < K; ++k)
    c->vehicle_L[k] = coef[static_cast<size_t>(k) * acmpc::kDynamicsCount + 14] + coef[static_cast<size_t>(k) * acmpc::kDynamicsCount + 15];
  std::memcpy(c->vehicle0, coef, sizeof c->vehicle0);
  c->has_dynamics = true;
  return ACMPC_OK;
}

int acmpc_set_dynamics_integration(acmpc_ctx* c, int32_t substeps, double blend_lo, double blend_hi) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_EINVAL, "acmpc_set_dynamics_integration needs a mode D handle");
  if (substeps < 1 || substeps > ACMPC_MAX_SUBSTEPS) return fail(c, ACMPC_EINVAL, "substeps is 1 .. ACMPC_MAX_SUBSTEPS = 16");
  const bool off = blend_lo == 0.0 && blend_hi == 0.0;
  if (!off && !(std::isfinite(blend_lo) && std::isfinite(blend_hi) && blend_lo >= 0.0 && blend_lo < blend_hi))
    return fail(c, ACMPC_EINVAL, "the low-speed blend is 0, 0 (off) or 0 <= lo < hi, both finite");
  // everything is checked before anything is kept: a refused setting leaves the handle's as it was
  c->substeps = substeps;
  c->blend_lo = off ? 0.0 : blend_lo;   // (-0.0 is 0)
  c->blend_hi = off ? 0.0 : blend_hi;
  return ACMPC_OK;
}

int acmpc_set_dynamics_terms(acmpc_ctx* c, const double rate_weight[2], const double rate_max[2], double slip_weight,
                             double slip_max) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_EINVAL, "acmpc_set_dynamics_terms needs a mode D handle");
  if (rate_weight == nullptr || rate_max == nullptr) return fail(c, ACMPC_EINVAL, "null rate_weight or rate_max");
  const double weights[3] = {rate_weight[0], rate_weight[1], slip_weight};
  const double limits[3] = {rate_max[0], rate_max[1], slip_max};
  for (int q = 0; q < 3; ++q) {
    // float32 is what the kernels get: a weight that overflows it is not finite there
    if (!std::isfinite(static_cast<float>(weights[q])) || !(weights[q] >= 0.0))
      return fail(c, ACMPC_EINVAL, "a weight of the rate and slip terms must be finite and >= 0");
    if (!(static_cast<float>(limits[q]) > 0.0f)) return fail(c, ACMPC_EINVAL, "a limit of the rate and slip terms must be > 0 (INFINITY: none)");
  }
  // everything is checked before anything is kept: a refused setting leaves the handle's as it was
  for (int q = 0; q < 2; ++q) {
    c->rate_weight[q] = weights[q] + 0.0;   // (-0.0 is 0)
    c->rate_max[q] = limits[q];
  }
  c->slip_weight = slip_weight + 0.0;
  c->slip_max = slip_max;
  return ACMPC_OK;
}

int acmpc_set_dynamics_objective(acmpc_ctx* c, double progress_weight, const double speed_ceiling[2]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_dynamics_objective needs a mode D handle");
  // float32 is what the kernels get: a value that overflows it is not finite there
  if (!std::isfinite(static_cast<float>(progress_weight)) || !(progress_weight >= 0.0))
    return fail(c, ACMPC_EINVAL, "progress_weight must be finite and >= 0");
  if (speed_ceiling != nullptr) {
    if (!std::isfinite(static_cast<float>(speed_ceiling[0])) || !(speed_ceiling[0] >= 0.0))
      return fail(c, ACMPC_EINVAL, "the speed ceiling's scale must be finite and >= 0");
    if (!std::isfinite(static_cast<float>(speed_ceiling[1]))) return fail(c, ACMPC_EINVAL, "the speed ceiling's offset must be finite");
  }
  // everything is checked before anything is kept: a refused setting leaves the handle's as it was
  c->progress_weight = progress_weight + 0.0;   // (-0.0 is 0)
  c->has_ceiling = speed_ceiling != nullptr;
  c->speed_ceiling[0] = c->has_ceiling ? speed_ceiling[0] + 0.0 : 0.0;
  c->speed_ceiling[1] = c->has_ceiling ? speed_ceiling[1] : 0.0;
  return ACMPC_OK;
}

int acmpc_set_dynamics_coupling(acmpc_ctx* c, const double ratio[2]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_dynamics_coupling needs a mode D handle");
  if (ratio == nullptr) {
    c->has_coupling = false;
    c->coupling[0] = c->coupling[1] = HUGE_VALF;
    return ACMPC_OK;
  }
  // float32 is what the kernels get: each ratio is rounded once, and must then be > 0 (+inf: no coupling on that axle)
  const float rho[2] = {static_cast<float>(ratio[0]), static_cast<float>(ratio[1])};
  for (int q = 0; q < 2; ++q)   // (a NaN compares false)
    if (!(rho[q] > 0.0f)) return fail(c, ACMPC_EINVAL, "a coupling ratio must be > 0 and finite, or INFINITY (none)");
  if (c->has_dynamics && !peaks_couple(c->vehicles)) return fail(c, ACMPC_EINVAL, kPeaksRefused);
  // everything is checked before anything is kept: a refused setting leaves the handle's as it was
  c->has_coupling = true;
  c->coupling[0] = rho[0];
  c->coupling[1] = rho[1];
  return ACMPC_OK;
}

int acmpc_set_dynamics_load_transfer(acmpc_ctx* c, const double setting[2]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_dynamics_load_transfer needs a mode D handle");
  if (setting == nullptr) {
    // (a smaller load range than the one that holds: nothing to refuse; the downforce's scalars with c_h = w_max = 0)
    float load[acmpc::kMaxVehicles][6] = {};
    if (c->has_dynamics) (void)derive_loads(nullptr, aero_of(c), c->vehicles, c->vehicle_L, c->vehicle_axle, load);
    c->has_load = false;
    c->load_setting[0] = c->load_setting[1] = 0.0;
    std::memcpy(c->load_const, load, sizeof load);
    return ACMPC_OK;
  }
  if (!std::isfinite(setting[0]) || !(setting[0] >= 0.0)) return fail(c, ACMPC_EINVAL, "h_cg must be finite and >= 0");
  if (!(setting[1] > 0.0 && setting[1] < 1.0)) return fail(c, ACMPC_EINVAL, "w_frac must lie inside (0, 1)");
  const double kept[2] = {setting[0] + 0.0, setting[1]};   // (-0.0 is 0)
  float load[acmpc::kMaxVehicles][6] = {};
  if (c->has_dynamics) {
    const char* refused = derive_loads(kept, aero_of(c), c->vehicles, c->vehicle_L, c->vehicle_axle, load);
    if (refused != nullptr) return fail(c, ACMPC_EINVAL, refused);
  }
  // everything is checked before anything is kept: a refused setting leaves the handle's as it was
  c->has_load = true;
  c->load_setting[0] = kept[0];
  c->load_setting[1] = kept[1];
  std::memcpy(c->load_const, load, sizeof load);
  return ACMPC_OK;
}

int acmpc_set_dynamics_downforce(acmpc_ctx* c, const double setting[3]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_dynamics_downforce needs a mode D handle");
  float load[acmpc::kMaxVehicles][6] = {};
  if (setting == nullptr) {
    if (c->has_dynamics) (void)derive_loads(load_of(c), nullptr, c->vehicles, c->vehicle_L, c->vehicle_axle, load);
    c->has_aero = false;
    c->aero[0] = c->aero[1] = c->aero[2] = 0.0f;
    std::memcpy(c->load_const, load, sizeof load);
    return ACMPC_OK;
  }
  // float32 is what the kernels get: each of the three is rounded once
  const float kept[3] = {static_cast<float>(setting[0]) + 0.0f, static_cast<float>(setting[1]) + 0.0f,   // (-0.0 is 0)
                         static_cast<float>(setting[2])};
  for (int a = 0; a < 2; ++a)   // (a NaN compares false)
    if (!std::isfinite(kept[a]) || !(kept[a] >= 0.0f)) return fail(c, ACMPC_EINVAL, "k_f, k_r must be finite and >= 0 (as float32)");
  if (!std::isfinite(kept[2]) || !(kept[2] > 0.0f)) return fail(c, ACMPC_EINVAL, "v_sat must be finite and > 0 (as float32)");
  if (c->has_dynamics) {
    const char* refused = derive_loads(load_of(c), kept, c->vehicles, c->vehicle_L, c->vehicle_axle, load);
    if (refused != nullptr) return fail(c, ACMPC_EINVAL, refused);
  }
  // everything is checked before anything is kept: a refused setting leaves the handle's as it was
  c->has_aero = true;
  std::memcpy(c->aero, kept, sizeof kept);
  std::memcpy(c->load_const, load, sizeof load);
  return ACMPC_OK;
}

int acmpc_set_previous_control(acmpc_ctx* c, const float* u_prev, int32_t P) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_EINVAL, "acmpc_set_previous_control needs a mode D handle");
  if (u_prev == nullptr) {
    c->h_uprev.clear();
    c->uprev_P = 0;
    c->uprev_dirty = false;
    return ACMPC_OK;
  }
  if (P < 1 || P > c->prm.max_problems) return fail(c, ACMPC_EINVAL, "P must be 1 .. max_problems");
  c->h_uprev.assign(u_prev, u_prev + static_cast<size_t>(P) * 2);
  c->uprev_P = P;
  c->uprev_dirty = true;
  return ACMPC_OK;
}

int acmpc_set_obstacles(acmpc_ctx* c, const float* positions, const float* radii, int32_t P, int32_t n, int32_t K) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_obstacles needs a mode D handle");
  if (positions == nullptr || K == 0) {
    c->h_obs.clear();
    c->obs_P = c->obs_n = c->obs_K = 0;
    c->obs_dirty = false;
    return ACMPC_OK;
  }
  if (K < 0 || K > ACMPC_MAX_OBSTACLES) return fail(c, ACMPC_EINVAL, "a problem has 0 .. ACMPC_MAX_OBSTACLES = 8 obstacle discs");
  if (P < 1 || P > c->prm.max_problems) return fail(c, ACMPC_EINVAL, "P must be 1 .. max_problems");
  if (n < 1 || n > c->prm.max_steps) return fail(c, ACMPC_EINVAL, "n must be 1 .. max_steps");
  if (radii == nullptr) return fail(c, ACMPC_EINVAL, "null radii");
  const size_t discs = static_cast<size_t>(P) * K, floats = discs * n * 2;
  for (size_t q = 0; q < discs; ++q)
    if (!std::isfinite(radii[q]) || !(radii[q] >= 0.0f)) return fail(c, ACMPC_EINVAL, "an obstacle's radius must be finite and >= 0");
  // everything is checked before anything is kept: refused data leaves the handle's as it was
  c->h_obs.assign(positions, positions + floats);
  c->h_obs.insert(c->h_obs.end(), radii, radii + discs);
  c->obs_P = P;
  c->obs_n = n;
  c->obs_K = K;
  c->obs_dirty = true;
  return ACMPC_OK;
}

int acmpc_set_surface(acmpc_ctx* c, const float* grip, int32_t P, int32_t n) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_surface needs a mode D handle");
  if (grip == nullptr) {
    c->h_surface.clear();
    c->surf_P = c->surf_n = 0;
    c->surf_dirty = false;
    return ACMPC_OK;
  }
  if (P < 1 || P > c->prm.max_problems) return fail(c, ACMPC_EINVAL, "P must be 1 .. max_problems");
  if (n < 1 || n > c->prm.max_steps) return fail(c, ACMPC_EINVAL, "n must be 1 .. max_steps");
  const size_t floats = static_cast<size_t>(P) * n * 2;
  for (size_t q = 0; q < floats; ++q)   // (a NaN compares false)
    if (!std::isfinite(grip[q]) || !(grip[q] > 0.0f)) return fail(c, ACMPC_EINVAL, "a grip scale must be finite and > 0");
  // everything is checked before anything is kept: a refused table leaves the handle's as it was
  c->h_surface.assign(grip, grip + floats);
  c->surf_P = P;
  c->surf_n = n;
  c->surf_dirty = true;
  return ACMPC_OK;
}

int acmpc_set_road(acmpc_ctx* c, const float* road, int32_t P, int32_t n) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_road needs a mode D handle");
  if (road == nullptr) {
    c->h_road.clear();
    c->road_P = c->road_n = 0;
    c->road_dirty = false;
    return ACMPC_OK;
  }
  if (P < 1 || P > c->prm.max_problems) return fail(c, ACMPC_EINVAL, "P must be 1 .. max_problems");
  if (n < 1 || n > c->prm.max_steps) return fail(c, ACMPC_EINVAL, "n must be 1 .. max_steps");
  const size_t rows = static_cast<size_t>(P) * n;
  for (size_t q = 0; q < 3 * rows; ++q)
    if (!std::isfinite(road[q])) return fail(c, ACMPC_EINVAL, "a road value must be finite");
  for (size_t q = 0; q < rows; ++q)
    if (!(road[3 * q + 2] > 0.0f)) return fail(c, ACMPC_EINVAL, "a road row's n_z must be > 0");
  // everything is checked before anything is kept: a refused table leaves the handle's as it was.  Staged as the device reads
  // it: (a_x, a_y, n_z, 0), one aligned 16-byte row per waypoint
  c->h_road.assign(4 * rows, 0.0f);
  for (size_t q = 0; q < rows; ++q) std::memcpy(&c->h_road[4 * q], road + 3 * q, 3 * sizeof(float));
  c->road_P = P;
  c->road_n = n;
  c->road_dirty = true;
  return ACMPC_OK;
}

int acmpc_set_dynamics_actuator(acmpc_ctx* c, const double tau[2]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_dynamics_actuator needs a mode D handle");
  if (tau == nullptr) {
    c->has_actuator = false;
    c->actuator_k[0] = c->actuator_k[1] = c->actuator_m[0] = c->actuator_m[1] = 0.0f;
    return ACMPC_OK;
  }
  float k[2], m[2];
  for (int ch = 0; ch < 2; ++ch) {   // (a NaN compares false)
    if (!std::isfinite(tau[ch]) || !(tau[ch] >= 0.0)) return fail(c, ACMPC_EINVAL, "tau_d, tau_p must be finite and >= 0");
    // in float64, each rounded once: what is left of an error after one control step, and its mean over the step
    const double kd = tau[ch] > 0.0 ? std::exp(-c->prm.dt / tau[ch]) : 0.0;
    const double md = tau[ch] > 0.0 ? (tau[ch] / c->prm.dt) * (1.0 - kd) : 0.0;
    k[ch] = static_cast<float>(kd);
    m[ch] = static_cast<float>(md);
  }
  // everything is checked before anything is kept: a refused setting leaves the handle's as it was
  c->has_actuator = true;
  std::memcpy(c->actuator_k, k, sizeof k);
  std::memcpy(c->actuator_m, m, sizeof m);
  return ACMPC_OK;
}

int acmpc_set_actuator_state(acmpc_ctx* c, const float* a0, int32_t P) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_actuator_state needs a mode D handle");
  if (a0 == nullptr) {
    c->h_astate.clear();
    c->astate_P = 0;
    c->astate_dirty = false;
    return ACMPC_OK;
  }
  if (P < 1 || P > c->prm.max_problems) return fail(c, ACMPC_EINVAL, "P must be 1 .. max_problems");
  c->h_astate.assign(a0, a0 + static_cast<size_t>(P) * 2);
  c->astate_P = P;
  c->astate_dirty = true;
  return ACMPC_OK;
}

int acmpc_set_dynamics_clearance(acmpc_ctx* c, double weight, double margin) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_set_dynamics_clearance needs a mode D handle");
  // float32 is what the kernels get: a value that overflows it is not finite there
  if (!std::isfinite(static_cast<float>(weight)) || !(weight >= 0.0)) return fail(c, ACMPC_EINVAL, "the clearance weight must be finite and >= 0");
  if (!std::isfinite(static_cast<float>(margin)) || !(margin >= 0.0)) return fail(c, ACMPC_EINVAL, "the clearance margin must be finite and >= 0");
  c->clearance_weight = weight + 0.0;   // (-0.0 is 0)
  c->clearance_margin = margin + 0.0;
  return ACMPC_OK;
}

// the refusals of acmpc_score_grips that its shape alone decides, in the order it makes them (the log's period, the weights
// and the scales come between the second and the third): acmpc_describe_score_grips makes the same three calls
static int grip_handle_ready(const acmpc_ctx* c) {
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_score_grips needs a mode D handle");
  if (!c->has_dynamics) return fail(c, ACMPC_ESTATE, "mode D: acmpc_set_dynamics has not been called");
  return ACMPC_OK;
}

static int grip_shape_valid(const acmpc_ctx* c, int W, int segment, int K) {
  if (W < 1 || W > ACMPC_MAX_LOG_STEPS) return fail(c, ACMPC_EINVAL, "the log has 1 .. ACMPC_MAX_LOG_STEPS = 512 steps");
  if (segment < 1 || segment > W) return fail(c, ACMPC_EINVAL, "segment is 1 .. W");
  if (K < 1) return fail(c, ACMPC_EINVAL, "K must be positive");
  return ACMPC_OK;
}

static int grip_shape_fits(const acmpc_ctx* c, int W, int segment, int K) {
  if (K > ACMPC_MAX_GRIP_HYPOTHESES) return fail(c, ACMPC_ECAPACITY, "at most ACMPC_MAX_GRIP_HYPOTHESES = 65536 hypotheses");
  if (static_cast<int64_t>(acmpc::identify_segments(W, segment)) * K > acmpc::kIdentifyMaxValues)
    return fail(c, ACMPC_ECAPACITY, "segments x hypotheses exceeds 2^22");
  return ACMPC_OK;
}

int acmpc_describe_score_grips(const acmpc_ctx* c, int32_t W, int32_t segment, int32_t K, int32_t out[8]) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (out == nullptr) return fail(c, ACMPC_EINVAL, "null output");
  ACMPC_TRY(grip_handle_ready(c));
  ACMPC_TRY(grip_shape_valid(c, W, segment, K));
  ACMPC_TRY(grip_shape_fits(c, W, segment, K));
  const int S = acmpc::identify_segments(W, segment);
  const acmpc::IdentifyGrid g = acmpc::identify_grid(S, K);
  out[0] = S;
  out[1] = g.blocks;
  out[2] = g.rows;
  out[3] = g.run;
  out[4] = g.grid_y;
  out[5] = S - (g.grid_y - 1) * g.run;   // segments of the last run
  out[6] = W - (S - 1) * segment;        // steps of the last segment
  out[7] = 0;
  return ACMPC_OK;
}

int acmpc_score_grips(acmpc_ctx* c, const float* states, const float* controls, int32_t W, double dt, int32_t segment,
                      const double weights[3], const double* scales, int32_t K, float* errors, int64_t* best) {
  if (c == nullptr) return ACMPC_EINVAL;
  // every refusal comes before any device work
  if (states == nullptr || controls == nullptr || weights == nullptr || scales == nullptr || best == nullptr)
    return fail(c, ACMPC_EINVAL, "acmpc_score_grips: null pointer");
  ACMPC_TRY(grip_handle_ready(c));
  if (c->stream_pending)
    return fail(c, ACMPC_ESTATE, "a batch of acmpc_solve_stream_device is pending: acmpc_solve_stream_flush first");
  ACMPC_TRY(grip_shape_valid(c, W, segment, K));
  if (!std::isfinite(dt) || !(dt > 0.0)) return fail(c, ACMPC_EINVAL, "dt must be finite and positive");
  bool any_weight = false;
  for (int q = 0; q < 3; ++q) {
    // float32 is what the kernel gets: a weight that overflows it is not finite there
    if (!std::isfinite(static_cast<float>(weights[q])) || !(weights[q] >= 0.0))
      return fail(c, ACMPC_EINVAL, "a weight of the residual must be finite and >= 0");
    any_weight = any_weight || static_cast<float>(weights[q]) != 0.0f;
  }
  if (!any_weight) return fail(c, ACMPC_EINVAL, "the residual's weights are all zero");
  ACMPC_TRY(grip_shape_fits(c, W, segment, K));
  const int S = acmpc::identify_segments(W, segment);
  for (int64_t q = 0; q < 2 * static_cast<int64_t>(K); ++q)
    if (!std::isfinite(scales[q]) || !(scales[q] > 0.0))
      return fail(c, ACMPC_EINVAL, "hypothesis " + std::to_string(q / 2) + ": a grip scale must be finite and positive");

  // device block: [256] partial keys | best key | [max K] errors | [max K][2] peaks | [513][3] states | [512][2] controls
  constexpr size_t kMaxK = ACMPC_MAX_GRIP_HYPOTHESES, kMaxW = ACMPC_MAX_LOG_STEPS;
  constexpr size_t kBestAt = 256 * sizeof(int64_t), kErrorsAt = kBestAt + sizeof(int64_t);
  constexpr size_t kUpAt = kErrorsAt + kMaxK * sizeof(float);   // (a multiple of 8: the peaks are read in pairs)
  constexpr size_t kBlockBytes = kUpAt + (2 * kMaxK + 3 * (kMaxW + 1) + 2 * kMaxW) * sizeof(float);
  static_assert(kUpAt % 8 == 0, "the peaks' pairs are 8-byte aligned");
  ACMPC_TRY(ensure_device(c));
  if (c->stream == nullptr) ACMPC_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  hipStream_t s = c->stream;
  ACMPC_HIP(c, alloc_once(&c->d_identify, kBlockBytes));
  const size_t e_floats = static_cast<size_t>(S) * K;
  if (c->identify_e_floats < e_floats) {   // (nothing of an earlier call is in flight: the call blocks)
    (void)hipFree(c->d_identify_e);
    c->d_identify_e = nullptr;
    c->identify_e_floats = 0;
    ACMPC_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_identify_e), e_floats * sizeof(float)));
    c->identify_e_floats = e_floats;
  }
  // one copy up: peaks | states | controls
  const size_t peak_floats = 2 * static_cast<size_t>(K), state_floats = 3 * (static_cast<size_t>(W) + 1),
               control_floats = 2 * static_cast<size_t>(W);
  const size_t up_bytes = (peak_floats + state_floats + control_floats) * sizeof(float);
  const size_t down_bytes = sizeof(int64_t) + (errors != nullptr ? static_cast<size_t>(K) * sizeof(float) : 0);
  c->h_identify.resize(std::max(up_bytes, down_bytes));
  float* up = reinterpret_cast<float*>(c->h_identify.data());
  for (int k = 0; k < K; ++k) derive_peaks(c->vehicle0, scales[2 * k], scales[2 * k + 1], &up[2 * k], &up[2 * k + 1]);
  std::memcpy(up + peak_floats, states, state_floats * sizeof(float));
  std::memcpy(up + peak_floats + state_floats, controls, control_floats * sizeof(float));
  ACMPC_HIP(c, hipMemcpyAsync(c->d_identify + kUpAt, up, up_bytes, hipMemcpyHostToDevice, s));
  acmpc::IdentifyArgs a{};
  a.peaks = reinterpret_cast<const float*>(c->d_identify + kUpAt);
  a.states = a.peaks + peak_floats;
  a.controls = a.states + state_floats;
  a.e = c->d_identify_e;
  a.errors = reinterpret_cast<float*>(c->d_identify + kErrorsAt);
  a.partial_keys = reinterpret_cast<int64_t*>(c->d_identify);
  a.best = reinterpret_cast<int64_t*>(c->d_identify + kBestAt);
  a.W = W;
  a.L = segment;
  a.K = K;
  for (int q = 0; q < 3; ++q) a.w[q] = static_cast<float>(weights[q]);
  // the handle's integration setting with the step of THIS log, under vehicle 0
  acmpc::Integration g = dynamics_integration(c);
  g.h = static_cast<float>(dt / c->substeps);
  // and its tyre coupling, each hypothesis capped by its own peaks
  // and its load transfer: the base vehicle's factors on each hypothesis' own peaks
  const float* lc = c->load_const[0];
  const acmpc::IdentifyLoad load{lc[0], lc[1], lc[2], lc[3], lc[4], lc[5]};
  // and its downforce: the same factors at each sub-step's speed
  const acmpc::IdentifyAero aero{c->aero[0], c->aero[1], c->aero[2]};
  ACMPC_HIP(c, acmpc::launch_identify_grip(a, c->vehicles.v[0], g, c->has_coupling ? c->coupling : nullptr,
                                           c->has_load || c->has_aero ? &load : nullptr, c->has_aero ? &aero : nullptr, s));
  // one copy down: best key | errors
  ACMPC_HIP(c, hipMemcpyAsync(c->h_identify.data(), c->d_identify + kBestAt, down_bytes, hipMemcpyDeviceToHost, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  std::memcpy(best, c->h_identify.data(), sizeof(int64_t));
  if (errors != nullptr) std::memcpy(errors, c->h_identify.data() + sizeof(int64_t), static_cast<size_t>(K) * sizeof(float));
  return ACMPC_OK;
}

int acmpc_trace_plans(acmpc_ctx* c, const float* x0, const float* U, int32_t P, int32_t M, int32_t n, float* states,
                      float* totals, float* terms) {
  if (c == nullptr) return ACMPC_EINVAL;
  // every refusal comes before any device work
  if (c->prm.mode != ACMPC_MODE_DYNAMIC) return fail(c, ACMPC_ESTATE, "acmpc_trace_plans needs a mode D handle");
  if (!c->has_dynamics) return fail(c, ACMPC_ESTATE, "mode D: acmpc_set_dynamics has not been called");
  if (x0 == nullptr || U == nullptr) return fail(c, ACMPC_EINVAL, "acmpc_trace_plans: null x0 or U");
  if (states == nullptr && totals == nullptr && terms == nullptr)
    return fail(c, ACMPC_EINVAL, "acmpc_trace_plans: at least one of states, totals and terms");
  if (M < 1) return fail(c, ACMPC_EINVAL, "P, M and n must be positive");
  // (pending stream, P and n positive, within the handle's capacity and the paths', the previous controls' and the obstacles')
  ACMPC_TRY(check_shape(c, P, 1, n, ACMPC_LAYOUT_CANDIDATE_MAJOR));
  static_assert(acmpc::kTraceTermFloats == ACMPC_TRACE_TERM_FLOATS, "the trace row of acmpc_dynamic_trace.h is the header's");
  const int K = c->vehicles.K;
  // the device block: x0 | U | states | totals | terms, each part a multiple of 16 bytes
  auto padded = [](size_t floats) { return (floats + 3) & ~static_cast<size_t>(3); };
  const size_t plans = static_cast<size_t>(P) * M, rolls = plans * K;
  const size_t x0_floats = static_cast<size_t>(P) * acmpc::kDynamicStateFloats, u_floats = plans * n * 2;
  const size_t state_floats = rolls * (static_cast<size_t>(n) + 1) * acmpc::kDynamicStateFloats, total_floats = rolls * 2,
               term_floats = rolls * n * acmpc::kTraceTermFloats;
  constexpr size_t kMaxOutputBytes = size_t{1} << 30;
  if (plans > 0x7fffffff || (state_floats + total_floats + term_floats) * sizeof(float) > kMaxOutputBytes)
    return fail(c, ACMPC_ECAPACITY, "acmpc_trace_plans: the outputs of one call exceed 1 GiB");
  const size_t at_u = padded(x0_floats), at_states = at_u + padded(u_floats), at_totals = at_states + padded(state_floats),
               at_terms = at_totals + padded(total_floats);
  const size_t bytes = (at_terms + padded(term_floats)) * sizeof(float);

  ACMPC_TRY(ensure_device(c));
  if (c->stream == nullptr) ACMPC_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  hipStream_t s = c->stream;
  if (c->plan_trace_bytes < bytes) {   // (drained first: nothing of an earlier call reads the block that goes)
    ACMPC_HIP(c, hipStreamSynchronize(s));
    (void)hipFree(c->d_plan_trace);
    c->d_plan_trace = nullptr;
    c->plan_trace_bytes = 0;
    ACMPC_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_plan_trace), bytes));
    c->plan_trace_bytes = bytes;
  }
  float* block = reinterpret_cast<float*>(c->d_plan_trace);
  ACMPC_TRY(upload_tables(c, s));
  ACMPC_HIP(c, hipMemcpyAsync(block, x0, x0_floats * sizeof(float), hipMemcpyHostToDevice, s));
  ACMPC_HIP(c, hipMemcpyAsync(block + at_u, U, u_floats * sizeof(float), hipMemcpyHostToDevice, s));
  acmpc::TraceArgs a{};
  a.U = block + at_u;
  a.x0 = block;
  a.coef = c->d_coef;
  a.states = states != nullptr ? block + at_states : nullptr;
  a.totals = totals != nullptr ? block + at_totals : nullptr;
  a.terms = terms != nullptr ? block + at_terms : nullptr;
  a.P = P;
  a.M = M;
  a.n = n;
  a.w = c->w;
  ACMPC_HIP(c, acmpc::launch_trace_dynamic(a, c->vehicles, dynamics_integration(c), dynamics_terms(c), s));
  if (states != nullptr)
    ACMPC_HIP(c, hipMemcpyAsync(states, a.states, state_floats * sizeof(float), hipMemcpyDeviceToHost, s));
  if (totals != nullptr)
    ACMPC_HIP(c, hipMemcpyAsync(totals, a.totals, total_floats * sizeof(float), hipMemcpyDeviceToHost, s));
  if (terms != nullptr) ACMPC_HIP(c, hipMemcpyAsync(terms, a.terms, term_floats * sizeof(float), hipMemcpyDeviceToHost, s));
  ACMPC_HIP(c, hipStreamSynchronize(s));
  return ACMPC_OK;
}

}  // extern "C"
