// The localiser's particle filter on the GPU, C API: the acmpc_pf_* entry points of
// include/acmpc.h, the handle's buffers and the launch sequences.  The kernels and their launchers are in
// acmpc_pf_score.hip (nearest map points, particle scores) and acmpc_pf_filter.hip (step, estimate, resampling), the
// host-only builder of the map's grid in acmpc_pf_grid.cpp, what they share in acmpc_pf.h.
// Two ways in.  Host pointers: acmpc_pf_score / _advance / _estimate take particles from the caller and hand the
// results back; resampling stays with the caller, in the reference's draw order (particle_filter.ParticleFilter).
// Device-resident: acmpc_pf_filter_* keep the particles on the device and resample there on counter-based draws, one
// host round trip per update (particle_filter.DeviceParticleFilter).  The map stays resident in device memory either way.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "acmpc_pf.h"

using namespace acmpc::pf;

namespace {

thread_local std::string g_pf_create_error;

// set and neither empty nor "0"
bool env_flag(const char* name) {
  const char* value = std::getenv(name);
  return value != nullptr && value[0] != '\0' && !(value[0] == '0' && value[1] == '\0');
}

// The reference's particle counts (hundreds): the kernel works straight in the page-locked block the host reads and writes
// (posted writes over the host link; page-locked memory is device-addressable) - no copy packet in front of or behind it.
// Large counts keep the copies: megabytes of 8-byte pieces are better moved as one DMA.  (Not kGridParticles, the count
// from which the grid search is a launch of its own: another decision with, today, the same answer.)
constexpr int kInPlaceParticles = 4096;

template <typename T>
int upload(acmpc_pf* h, T** slot, const std::vector<T>& values) {
  PF_HIP(h, acmpc::alloc_once(slot, values.size() * sizeof(T)));
  PF_HIP(h, hipMemcpy(*slot, values.data(), values.size() * sizeof(T), hipMemcpyHostToDevice));
  return ACMPC_OK;
}

// (hipFree of a null pointer does nothing)
template <typename... T>
void free_device(T*... p) {
  ((void)hipFree(p), ...);
}

// (a step that has failed has left its message in the handle: pass its code on)
#define PF_TRY(call) do { const int rc_ = (call); if (rc_ != ACMPC_OK) return rc_; } while (0)

// Retry-safe, like pf_ensure_filter: after a failure half-way (out of memory) what was obtained stays with the handle, a
// second call allocates only what is missing, and acmpc_pf_destroy frees whatever exists.
int pf_ensure_device(acmpc_pf* h) {
  if (h->device_ready) return ACMPC_OK;
  int count = 0;
  const hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0)
    return pf_fail(h, ACMPC_ENODEVICE, "no HIP device visible: particle scoring has no CPU fallback");
  if (h->prm.device >= 0) PF_HIP(h, hipSetDevice(h->prm.device));
  h->device_chosen = true;
  if (h->stream == nullptr) PF_HIP(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  for (int t = 0; t < 3; ++t) PF_TRY(upload(h, &h->d_track[t], h->h_track[t]));
  const size_t P = h->prm.max_particles, K = h->prm.max_observation_points;
  const PfGrid& grid = h->grid;
  if (grid.geometry.nx > 0) {
    for (int t = 0; t < 3; ++t) {
      PF_TRY(upload(h, &h->d_grid_start[t], grid.start[t]));
      PF_TRY(upload(h, &h->d_grid_index[t], grid.index[t]));
      PF_TRY(upload(h, &h->d_grid_x[t], grid.x[t]));
      PF_TRY(upload(h, &h->d_grid_y[t], grid.y[t]));
    }
    PF_TRY(upload(h, &h->d_block_start, grid.block_start));
    PF_TRY(upload(h, &h->d_block_index, grid.block_index));
    PF_TRY(upload(h, &h->d_block_x, grid.block_x));
    PF_TRY(upload(h, &h->d_block_y, grid.block_y));
    PF_HIP(h, acmpc::alloc_once(&h->d_near_index, P * 3 * sizeof(int32_t)));
    PF_HIP(h, acmpc::alloc_once(&h->d_near_d2, P * 3 * sizeof(double)));
  }
  PF_HIP(h, acmpc::alloc_once(&h->d_states, (P * 3 + K * 2) * sizeof(float)));
  PF_HIP(h, acmpc::host_alloc_once(&h->h_up, (P * 3 + K * 2) * sizeof(float)));
  const size_t down = P * (4 * sizeof(double) + 3 * sizeof(int32_t) + 1);
  PF_HIP(h, acmpc::host_alloc_once(&h->h_down, down));
  PF_HIP(h, acmpc::alloc_once(&h->d_down, down));
  PF_HIP(h, acmpc::alloc_once(&h->d_aux, P * 2 * sizeof(float)));
  PF_HIP(h, acmpc::alloc_once(&h->d_out, 8 * sizeof(double)));
  PF_TRY(query_given_wave_slots(h));
  h->device_ready = true;
  return ACMPC_OK;
}

// the tiled resampling and estimate (pf_resample_tiles_kernel ...) for capacities one workgroup is too slow for; the plan
// kernel holds a tile per thread, which bounds them at 2^20 particles.  ACMPC_PF_NARROW_FILTER=1: one workgroup always (A/B)
bool wide_filter(const acmpc_pf* h) {
  return h->prm.max_particles >= kWideFilter && h->prm.max_particles <= kScanBlock * kScanBlock && !h->narrow_filter;
}

int pf_ensure_filter(acmpc_pf* h) {
  if (h->filter_ready) return ACMPC_OK;
  PF_TRY(pf_ensure_device(h));
  const size_t P = h->prm.max_particles, K = h->prm.max_observation_points;
  for (int b = 0; b < 2; ++b) {
    PF_HIP(h, acmpc::alloc_once(&h->f_states[b], P * 3 * sizeof(float)));
    PF_HIP(h, acmpc::alloc_once(&h->f_scores[b], P * sizeof(float)));
  }
  PF_HIP(h, acmpc::alloc_once(&h->f_obs, K * 2 * sizeof(float)));
  PF_HIP(h, acmpc::alloc_once(&h->f_cdf, P * sizeof(unsigned long long)));
  PF_HIP(h, acmpc::alloc_once(&h->f_kept, P * sizeof(int)));
  PF_HIP(h, acmpc::alloc_once(&h->f_counts, 4 * sizeof(int)));
  if (wide_filter(h)) {
    const size_t tiles = (P + kScanBlock - 1) / kScanBlock, sums = (P + kEstimateTile - 1) / kEstimateTile;
    PF_HIP(h, acmpc::alloc_once(&h->f_wide, (2 * tiles + 6) * sizeof(unsigned long long)));
    PF_HIP(h, acmpc::alloc_once(&h->f_partial, sums * 10 * sizeof(double)));
  }
  PF_HIP(h, hipMemset(h->f_counts, 0, 4 * sizeof(int)));
  PF_HIP(h, acmpc::host_alloc_once(&h->h_result, 8 * sizeof(double) + 4 * sizeof(int)));
  PF_HIP(h, hipStreamSynchronize(nullptr));
  h->filter_ready = true;
  return ACMPC_OK;
}

Track track_of(const acmpc_pf* h, int t) { return Track{h->d_track[t], static_cast<int>(h->h_track[t].size() / 2)}; }

// What a scoring launch reads and where it writes: `out_block` is laid out [4][stride] doubles (minimum offset, heading
// offset, error, score) | [stride][3] int32 (track indices) | [stride] bytes (valid).  The device-resident filter sets
// `live` and `publish` afterwards.
ScoreArgs score_args(const acmpc_pf* h, const float* states, const float* obs, int k_left, int k_right,
                     unsigned char* out_block, size_t stride) {
  ScoreArgs a{};
  a.states = states;
  a.obs = obs;
  a.k_left = k_left;
  a.k_right = k_right;
  a.centre = track_of(h, 0);
  a.left = track_of(h, 1);
  a.right = track_of(h, 2);
  a.mean = h->prm.score_mean;
  a.sigma = h->prm.score_sigma;
  a.scale = h->scale;
  a.thr_rotation = h->prm.threshold_rotation;
  a.thr_offset = h->prm.threshold_offset;
  a.thr_error = h->prm.threshold_error;
  a.minimum_offset = reinterpret_cast<double*>(out_block);
  a.heading_offset = a.minimum_offset + stride;
  a.error = a.heading_offset + stride;
  a.score = a.error + stride;
  a.track_indices = reinterpret_cast<int32_t*>(out_block + 4 * stride * sizeof(double));
  a.valid = reinterpret_cast<uint8_t*>(out_block + 4 * stride * sizeof(double) + stride * 3 * sizeof(int32_t));
  return a;
}

// (the scoring results of the update lie in d_down with the capacity as their stride: see acmpc_pf_filter_update)
FilterArgs filter_args(acmpc_pf* h, const acmpc_pf_resample* rs) {
  FilterArgs f{};
  const size_t P = h->prm.max_particles;
  f.states_in = h->f_states[h->f_cur];
  f.scores_in = h->f_scores[h->f_cur];
  f.score = reinterpret_cast<const double*>(h->d_down) + 3 * P;
  f.valid = reinterpret_cast<const uint8_t*>(h->d_down + 4 * P * sizeof(double) + P * 3 * sizeof(int32_t));
  f.states_out = h->f_states[1 - h->f_cur];
  f.scores_out = h->f_scores[1 - h->f_cur];
  f.cdf = h->f_cdf;
  f.kept = h->f_kept;
  f.counts = h->f_counts;
  f.centre = h->d_track[0];
  f.m_centre = static_cast<int>(h->h_track[0].size() / 2);
  f.capacity = h->prm.max_particles;
  if (rs != nullptr) {
    f.n_desired = rs->n_desired;
    f.minimum_particles = rs->minimum_particles;
    f.sigma_x = rs->sigma_x;
    f.sigma_y = rs->sigma_y;
    f.sigma_yaw = rs->sigma_yaw;
    f.seed_lo = static_cast<uint32_t>(rs->seed);
    f.seed_hi = static_cast<uint32_t>(rs->seed >> 32);
    f.counter = rs->counter;
  }
  return f;
}

}  // namespace

namespace acmpc::pf {

int pf_fail(const acmpc_pf* h, int code, const std::string& msg) {
  if (h != nullptr) {
    h->err = msg;
  } else {
    g_pf_create_error = msg;
  }
  return code;
}

}  // namespace acmpc::pf

extern "C" {

const char* acmpc_pf_last_error(const acmpc_pf* h) { return h != nullptr ? h->err.c_str() : g_pf_create_error.c_str(); }

int acmpc_pf_create(const acmpc_pf_params* params, const double* centre, int32_t m_centre, const double* left,
                    int32_t m_left, const double* right, int32_t m_right, acmpc_pf** out) {
  if (params == nullptr || centre == nullptr || left == nullptr || right == nullptr || out == nullptr)
    return pf_fail(nullptr, ACMPC_EINVAL, "null argument");
  *out = nullptr;
  if (params->struct_size != sizeof(acmpc_pf_params)) return pf_fail(nullptr, ACMPC_EINVAL, "acmpc_pf_params size mismatch");
  if (m_centre < 3 || m_left < 1 || m_right < 1) return pf_fail(nullptr, ACMPC_EINVAL, "map polylines too short");
  if (params->max_particles < 1 || params->max_observation_points < 1 || !(params->score_sigma > 0.0))
    return pf_fail(nullptr, ACMPC_EINVAL, "bad capacities or score_sigma");
  acmpc_pf* h = new (std::nothrow) acmpc_pf();
  if (h == nullptr) return pf_fail(nullptr, ACMPC_EINVAL, "out of host memory");
  h->prm = *params;
  h->no_grid = env_flag("ACMPC_PF_NO_GRID");
  h->workgroup_score = env_flag("ACMPC_PF_WORKGROUP_SCORE");
  h->narrow_filter = env_flag("ACMPC_PF_NARROW_FILTER");
  h->no_blocks = env_flag("ACMPC_PF_NO_BLOCKS");
  h->h_track[0].assign(centre, centre + 2 * static_cast<size_t>(m_centre));
  h->h_track[1].assign(left, left + 2 * static_cast<size_t>(m_left));
  h->h_track[2].assign(right, right + 2 * static_cast<size_t>(m_right));
  h->grid = build_pf_grid(h->h_track);
  // score normaliser: max of the pdf over linspace(-10, 10, 100) (localiser.py:655-661)
  double best = 0.0;
  for (int i = 0; i < 100; ++i) {
    const double x = -10.0 + 20.0 * i / 99.0;
    const double z = (x - params->score_mean) / params->score_sigma;
    best = std::max(best, std::exp(-z * z / 2.0) / std::sqrt(2.0 * kPi) / params->score_sigma);
  }
  h->scale = best;
  *out = h;
  return ACMPC_OK;
}

void acmpc_pf_destroy(acmpc_pf* h) {
  if (h == nullptr) return;
  if (h->device_chosen) {   // (before that nothing was allocated, and a machine without a device is left alone)
    if (h->prm.device >= 0) (void)hipSetDevice(h->prm.device);
    for (int t = 0; t < 3; ++t) free_device(h->d_track[t], h->d_grid_start[t], h->d_grid_index[t], h->d_grid_x[t], h->d_grid_y[t]);
    for (int b = 0; b < 2; ++b) free_device(h->f_states[b], h->f_scores[b]);
    free_device(h->d_block_start, h->d_block_index, h->d_block_x, h->d_block_y, h->d_near_index, h->d_near_d2, h->d_states,
                h->d_down, h->d_aux, h->d_out, h->f_obs, h->f_cdf, h->f_kept, h->f_counts, h->f_wide, h->f_partial);
    for (void* p : {static_cast<void*>(h->h_up), static_cast<void*>(h->h_down), static_cast<void*>(h->h_result)})
      if (p != nullptr) (void)hipHostFree(p);
    if (h->stream != nullptr) (void)hipStreamDestroy(h->stream);
  }
  delete h;
}

double acmpc_pf_score_scale(const acmpc_pf* h) { return h != nullptr ? h->scale : 0.0; }

int acmpc_pf_score(acmpc_pf* h, const float* states, int32_t P, const float* obs_left, int32_t k_left,
                   const float* obs_right, int32_t k_right, int32_t* track_indices, double* minimum_offset,
                   double* heading_offset, double* observation_error, double* score, uint8_t* valid) {
  if (h == nullptr) return ACMPC_EINVAL;
  if (states == nullptr || track_indices == nullptr || minimum_offset == nullptr || heading_offset == nullptr ||
      observation_error == nullptr || score == nullptr || valid == nullptr)
    return pf_fail(h, ACMPC_EINVAL, "null argument");
  if (P < 1 || k_left < 0 || k_right < 0 || k_left + k_right < 1) return pf_fail(h, ACMPC_EINVAL, "empty input");
  if ((k_left > 0 && obs_left == nullptr) || (k_right > 0 && obs_right == nullptr))
    return pf_fail(h, ACMPC_EINVAL, "null observation");
  if (P > h->prm.max_particles || k_left + k_right > h->prm.max_observation_points)
    return pf_fail(h, ACMPC_ECAPACITY, "more particles or observation points than the handle was created for");
  PF_TRY(pf_ensure_device(h));
  hipStream_t s = h->stream;
  const int K = k_left + k_right;
  const size_t up_floats = static_cast<size_t>(P) * 3 + static_cast<size_t>(K) * 2;
  float* up = reinterpret_cast<float*>(h->h_up);
  std::memcpy(up, states, static_cast<size_t>(P) * 3 * sizeof(float));
  if (k_left > 0) std::memcpy(up + 3 * static_cast<size_t>(P), obs_left, static_cast<size_t>(k_left) * 2 * sizeof(float));
  if (k_right > 0)
    std::memcpy(up + 3 * static_cast<size_t>(P) + 2 * static_cast<size_t>(k_left), obs_right,
                static_cast<size_t>(k_right) * 2 * sizeof(float));
  PF_HIP(h, hipMemcpyAsync(h->d_states, up, up_floats * sizeof(float), hipMemcpyHostToDevice, s));
  const bool in_place = P < kInPlaceParticles;
  ScoreArgs a = score_args(h, h->d_states, h->d_states + 3 * static_cast<size_t>(P), k_left, k_right,
                           in_place ? h->h_down : h->d_down, static_cast<size_t>(P));
  (void)hipGetLastError();  // a stale error of an earlier call must not be read as this launch's
  PF_HIP(h, launch_nearest(h, a, P, s));
  launch_score(h, a, P, s);
  PF_HIP(h, hipGetLastError());
  const size_t pd = static_cast<size_t>(P) * sizeof(double);
  const size_t down = 4 * pd + static_cast<size_t>(P) * (3 * sizeof(int32_t) + 1);
  if (!in_place) PF_HIP(h, hipMemcpyAsync(h->h_down, h->d_down, down, hipMemcpyDeviceToHost, s));
  PF_HIP(h, hipStreamSynchronize(s));
  const unsigned char* dn = h->h_down;
  std::memcpy(minimum_offset, dn, pd);
  std::memcpy(heading_offset, dn + pd, pd);
  std::memcpy(observation_error, dn + 2 * pd, pd);
  std::memcpy(score, dn + 3 * pd, pd);
  std::memcpy(track_indices, dn + 4 * pd, static_cast<size_t>(P) * 3 * sizeof(int32_t));
  std::memcpy(valid, dn + 4 * pd + static_cast<size_t>(P) * 3 * sizeof(int32_t), static_cast<size_t>(P));
  return ACMPC_OK;
}

int acmpc_pf_advance(acmpc_pf* h, float* states, const float* delta, const float* velocity, int32_t P, double dt) {
  if (h == nullptr) return ACMPC_EINVAL;
  if (states == nullptr || delta == nullptr || velocity == nullptr) return pf_fail(h, ACMPC_EINVAL, "null argument");
  if (P < 1 || P > h->prm.max_particles) return pf_fail(h, ACMPC_ECAPACITY, "particle count out of range");
  PF_TRY(pf_ensure_device(h));
  hipStream_t s = h->stream;
  const size_t pf = static_cast<size_t>(P) * sizeof(float), n = static_cast<size_t>(P);
  // in place (kInPlaceParticles): every particle is read and written once by its own lane, 20 bytes of the 45 the block
  // holds for it - four copies from and to pageable memory, a synchronous staged copy of ~15 us each whatever its size,
  // were most of this call
  const bool in_place = P < kInPlaceParticles;
  float* block = reinterpret_cast<float*>(h->h_down);
  float* d_states = in_place ? block : h->d_states;
  float* d_delta = in_place ? block + 3 * n : h->d_aux;
  float* d_velocity = in_place ? block + 4 * n : h->d_aux + n;
  if (in_place) {
    std::memcpy(d_states, states, 3 * pf);
    std::memcpy(d_delta, delta, pf);
    std::memcpy(d_velocity, velocity, pf);
  } else {
    PF_HIP(h, hipMemcpyAsync(d_states, states, 3 * pf, hipMemcpyHostToDevice, s));
    PF_HIP(h, hipMemcpyAsync(d_delta, delta, pf, hipMemcpyHostToDevice, s));
    PF_HIP(h, hipMemcpyAsync(d_velocity, velocity, pf, hipMemcpyHostToDevice, s));
  }
  (void)hipGetLastError();  // a stale error of an earlier call must not be read as this launch's
  launch_advance(d_states, d_delta, d_velocity, P, static_cast<float>(h->prm.wheelbase), static_cast<float>(dt), s);
  PF_HIP(h, hipGetLastError());
  if (!in_place) PF_HIP(h, hipMemcpyAsync(states, d_states, 3 * pf, hipMemcpyDeviceToHost, s));
  PF_HIP(h, hipStreamSynchronize(s));
  if (in_place) std::memcpy(states, block, 3 * pf);
  return ACMPC_OK;
}

int acmpc_pf_estimate(acmpc_pf* h, const float* states, const float* scores, int32_t P, double estimate[3],
                      double* max_distance, double* max_angle) {
  if (h == nullptr) return ACMPC_EINVAL;
  if (states == nullptr || scores == nullptr || estimate == nullptr) return pf_fail(h, ACMPC_EINVAL, "null argument");
  if (P < 1 || P > h->prm.max_particles) return pf_fail(h, ACMPC_ECAPACITY, "particle count out of range");
  PF_TRY(pf_ensure_device(h));
  hipStream_t s = h->stream;
  PF_HIP(h, hipMemcpyAsync(h->d_states, states, static_cast<size_t>(P) * 3 * sizeof(float), hipMemcpyHostToDevice, s));
  PF_HIP(h, hipMemcpyAsync(h->d_aux, scores, static_cast<size_t>(P) * sizeof(float), hipMemcpyHostToDevice, s));
  (void)hipGetLastError();  // a stale error of an earlier call must not be read as this launch's
  launch_estimate(h, false, h->d_states, h->d_aux, P, nullptr, h->d_out, nullptr, s);   // one workgroup at any count
  PF_HIP(h, hipGetLastError());
  double res[5];
  PF_HIP(h, hipMemcpyAsync(res, h->d_out, sizeof res, hipMemcpyDeviceToHost, s));
  PF_HIP(h, hipStreamSynchronize(s));
  for (int c = 0; c < 3; ++c) estimate[c] = res[c];
  if (max_distance != nullptr) *max_distance = res[3];
  if (max_angle != nullptr) *max_angle = res[4];
  return ACMPC_OK;
}

int acmpc_pf_filter_reset(acmpc_pf* h, int32_t n) {
  if (h == nullptr) return ACMPC_EINVAL;
  if (n < 1 || n > h->prm.max_particles) return pf_fail(h, ACMPC_ECAPACITY, "particle count out of range");
  PF_TRY(pf_ensure_filter(h));
  // the resampling kernel's reset branch with nothing valid: n_live = 0, minimum = 1, capacity = n
  hipStream_t s = h->stream;
  const int zero[4] = {0, 0, 0, 0};
  PF_HIP(h, hipMemcpyAsync(h->f_counts, zero, sizeof zero, hipMemcpyHostToDevice, s));
  FilterArgs f = filter_args(h, nullptr);
  f.capacity = n;
  f.minimum_particles = 1;
  (void)hipGetLastError();
  launch_reset(f, s);
  PF_HIP(h, hipGetLastError());
  PF_HIP(h, hipStreamSynchronize(s));
  h->f_cur = 1 - h->f_cur;
  return ACMPC_OK;
}

int acmpc_pf_filter_set(acmpc_pf* h, const float* states, const float* scores, int32_t n) {
  if (h == nullptr) return ACMPC_EINVAL;
  if (states == nullptr || scores == nullptr) return pf_fail(h, ACMPC_EINVAL, "null argument");
  if (n < 1 || n > h->prm.max_particles) return pf_fail(h, ACMPC_ECAPACITY, "particle count out of range");
  PF_TRY(pf_ensure_filter(h));
  hipStream_t s = h->stream;
  const int counts[4] = {n, 0, 0, 0};
  PF_HIP(h, hipMemcpyAsync(h->f_states[h->f_cur], states, static_cast<size_t>(n) * 3 * sizeof(float), hipMemcpyHostToDevice, s));
  PF_HIP(h, hipMemcpyAsync(h->f_scores[h->f_cur], scores, static_cast<size_t>(n) * sizeof(float), hipMemcpyHostToDevice, s));
  PF_HIP(h, hipMemcpyAsync(h->f_counts, counts, sizeof counts, hipMemcpyHostToDevice, s));
  PF_HIP(h, hipStreamSynchronize(s));
  return ACMPC_OK;
}

int acmpc_pf_filter_get(acmpc_pf* h, float* states, float* scores, int32_t capacity, int32_t* n) {
  if (h == nullptr) return ACMPC_EINVAL;
  if (states == nullptr || scores == nullptr || n == nullptr) return pf_fail(h, ACMPC_EINVAL, "null argument");
  if (!h->filter_ready) return pf_fail(h, ACMPC_ESTATE, "no particles on the device yet");
  hipStream_t s = h->stream;
  int counts[4];
  PF_HIP(h, hipMemcpyAsync(counts, h->f_counts, sizeof counts, hipMemcpyDeviceToHost, s));
  PF_HIP(h, hipStreamSynchronize(s));
  if (counts[0] > capacity) return pf_fail(h, ACMPC_ECAPACITY, "output buffers too small");
  PF_HIP(h, hipMemcpyAsync(states, h->f_states[h->f_cur], static_cast<size_t>(counts[0]) * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
  PF_HIP(h, hipMemcpyAsync(scores, h->f_scores[h->f_cur], static_cast<size_t>(counts[0]) * sizeof(float), hipMemcpyDeviceToHost, s));
  PF_HIP(h, hipStreamSynchronize(s));
  *n = counts[0];
  return ACMPC_OK;
}

int acmpc_pf_filter_step(acmpc_pf* h, double tyre_angle, double velocity, double dt, double sigma_yaw,
                         double sigma_velocity, uint64_t seed, uint32_t counter) {
  if (h == nullptr) return ACMPC_EINVAL;
  if (!h->filter_ready) return pf_fail(h, ACMPC_ESTATE, "no particles on the device yet");
  (void)hipGetLastError();
  launch_step(h, static_cast<float>(tyre_angle), static_cast<float>(velocity), static_cast<float>(sigma_yaw),
              static_cast<float>(sigma_velocity), static_cast<float>(dt), seed, counter);
  PF_HIP(h, hipGetLastError());
  return ACMPC_OK;
}

int acmpc_pf_filter_update(acmpc_pf* h, const float* obs_left, int32_t k_left, const float* obs_right,
                           int32_t k_right, const acmpc_pf_resample* rs, double* result) {
  if (h == nullptr) return ACMPC_EINVAL;
  if (rs == nullptr || result == nullptr) return pf_fail(h, ACMPC_EINVAL, "null argument");
  if (rs->struct_size != sizeof(acmpc_pf_resample)) return pf_fail(h, ACMPC_EINVAL, "acmpc_pf_resample size mismatch");
  if (k_left < 0 || k_right < 0 || k_left + k_right < 1) return pf_fail(h, ACMPC_EINVAL, "empty observation");
  if ((k_left > 0 && obs_left == nullptr) || (k_right > 0 && obs_right == nullptr))
    return pf_fail(h, ACMPC_EINVAL, "null observation");
  if (k_left + k_right > h->prm.max_observation_points) return pf_fail(h, ACMPC_ECAPACITY, "too many observation points");
  if (!h->filter_ready) return pf_fail(h, ACMPC_ESTATE, "no particles on the device yet");
  hipStream_t s = h->stream;
  const int capacity = h->prm.max_particles;
  const bool wide = wide_filter(h);
  // 1. the observation up (one pinned block); everything else is already there
  float* up = reinterpret_cast<float*>(h->h_up);
  if (k_left > 0) std::memcpy(up, obs_left, static_cast<size_t>(k_left) * 2 * sizeof(float));
  if (k_right > 0) std::memcpy(up + 2 * static_cast<size_t>(k_left), obs_right, static_cast<size_t>(k_right) * 2 * sizeof(float));
  PF_HIP(h, hipMemcpyAsync(h->f_obs, up, static_cast<size_t>(k_left + k_right) * 2 * sizeof(float), hipMemcpyHostToDevice, s));
  // 2. score: launches over the capacity, whose workgroups beyond the live count (on the device) return at once
  ScoreArgs a = score_args(h, h->f_states[h->f_cur], h->f_obs, k_left, k_right, h->d_down, static_cast<size_t>(capacity));
  a.live = h->f_counts;
  a.publish = h->f_scores[h->f_cur];   // (the scoring kernels write the float32 scores themselves: no launch for that)
  (void)hipGetLastError();
  PF_HIP(h, launch_nearest(h, a, capacity, s));
  launch_score(h, a, capacity, s);
  PF_HIP(h, hipGetLastError());
  // 3. resample into the other pair of buffers
  launch_resample(h, filter_args(h, rs), wide, s);
  PF_HIP(h, hipGetLastError());
  h->f_cur = 1 - h->f_cur;
  // 4. estimate: the last kernel writes it and the counts straight into the page-locked result block (posted writes over
  // the host link): no copy packets behind the update
  double* res = h->h_result;
  launch_estimate(h, wide, h->f_states[h->f_cur], h->f_scores[h->f_cur], -1, h->f_counts, res, reinterpret_cast<int*>(res + 8), s);
  PF_HIP(h, hipGetLastError());
  // 5. wait and hand back
  PF_HIP(h, hipStreamSynchronize(s));
  const int* counts = reinterpret_cast<const int*>(res + 8);
  for (int i = 0; i < 5; ++i) result[i] = res[i];
  result[5] = counts[0];
  result[6] = counts[1];
  result[7] = counts[2];
  return ACMPC_OK;
}

}  // extern "C"
