// Allocate only what is not there yet: after a mid-way failure (out of memory) the buffers already obtained stay
// owned by the handle, a retry on the same handle picks up where the failed call stopped, and the handle's destroy
// frees whatever exists.  Shared by the main handle (acmpc_ctx.h) and the particle filter's (acmpc_pf.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace acmpc {

template <typename T>
hipError_t alloc_once(T** slot, size_t bytes) {
  if (*slot != nullptr) return hipSuccess;
  return hipMalloc(reinterpret_cast<void**>(slot), bytes);
}
template <typename T>
hipError_t host_alloc_once(T** slot, size_t bytes) {
  if (*slot != nullptr) return hipSuccess;
  return hipHostMalloc(reinterpret_cast<void**>(slot), bytes, hipHostMallocDefault);
}

}  // namespace acmpc
