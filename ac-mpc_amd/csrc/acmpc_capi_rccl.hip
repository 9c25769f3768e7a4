// C ABI, reduction across ranks (include/acmpc.h).  This unit owns the RCCL entry points resolved at run time (RCCL is
// never linked) and the calls built on them: acmpc_rccl_* and acmpc_reduce_across_ranks.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enums only: RCCL is resolved at run time, not linked

#include <cstdlib>

#include "acmpc_ctx.h"

using namespace acmpc::capi;

namespace {

using AllReduceFn = ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
using ErrorStringFn = const char* (*)(ncclResult_t);

using UniqueIdFn = ncclResult_t (*)(ncclUniqueId*);
using CommInitRankFn = ncclResult_t (*)(ncclComm_t*, int, ncclUniqueId, int);
using CommDestroyFn = ncclResult_t (*)(ncclComm_t);

struct Rccl {
  AllReduceFn all_reduce = nullptr;
  ErrorStringFn error_string = nullptr;
  UniqueIdFn unique_id = nullptr;
  CommInitRankFn comm_init_rank = nullptr;
  CommDestroyFn comm_destroy = nullptr;
};

// the RCCL that is already in the process owns the caller's communicator; only without one open the system's
const Rccl& rccl() {
  static const Rccl api = [] {
    Rccl r;
    void* sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
    void* handle = nullptr;
    if (sym == nullptr) {
      const char* path = std::getenv("ACMPC_RCCL_LIBRARY");
      handle = dlopen(path != nullptr ? path : "librccl.so.1", RTLD_NOW | RTLD_LOCAL);
      if (handle == nullptr && path == nullptr) handle = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
      if (handle != nullptr) sym = dlsym(handle, "ncclAllReduce");
    }
    r.all_reduce = reinterpret_cast<AllReduceFn>(sym);
    auto also = [handle](const char* name) { return (handle != nullptr) ? dlsym(handle, name) : dlsym(RTLD_DEFAULT, name); };
    r.error_string = reinterpret_cast<ErrorStringFn>(also("ncclGetErrorString"));
    r.unique_id = reinterpret_cast<UniqueIdFn>(also("ncclGetUniqueId"));
    r.comm_init_rank = reinterpret_cast<CommInitRankFn>(also("ncclCommInitRank"));
    r.comm_destroy = reinterpret_cast<CommDestroyFn>(also("ncclCommDestroy"));
    return r;
  }();
  return api;
}

}  // namespace

extern "C" {

// A communicator for acmpc_reduce_across_ranks from the SAME copy of RCCL that call resolves (a process can hold two - the
// system's and the one PyTorch bundles - and a communicator only works with the copy that made it).
int acmpc_rccl_unique_id(void* id_out) {
  if (id_out == nullptr) return ACMPC_EINVAL;
  const Rccl& api = rccl();
  if (api.unique_id == nullptr) return ACMPC_ESTATE;
  static_assert(sizeof(ncclUniqueId) == ACMPC_RCCL_UNIQUE_ID_BYTES, "ncclUniqueId is 128 bytes");
  return api.unique_id(static_cast<ncclUniqueId*>(id_out)) == ncclSuccess ? ACMPC_OK : ACMPC_EHIP;
}

int acmpc_rccl_comm_create(const void* id, int32_t n_ranks, int32_t rank, int32_t device, void** comm_out) {
  if (id == nullptr || comm_out == nullptr || n_ranks < 1 || rank < 0 || rank >= n_ranks) return ACMPC_EINVAL;
  *comm_out = nullptr;
  const Rccl& api = rccl();
  if (api.comm_init_rank == nullptr) return ACMPC_ESTATE;
  if (device >= 0 && hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    return ACMPC_ENODEVICE;
  }
  ncclUniqueId by_value;
  std::memcpy(&by_value, id, sizeof by_value);
  ncclComm_t comm = nullptr;
  if (api.comm_init_rank(&comm, n_ranks, by_value, rank) != ncclSuccess) return ACMPC_EHIP;
  *comm_out = comm;
  return ACMPC_OK;
}

int acmpc_rccl_comm_destroy(void* comm) {
  if (comm == nullptr) return ACMPC_OK;
  const Rccl& api = rccl();
  if (api.comm_destroy == nullptr) return ACMPC_ESTATE;
  return api.comm_destroy(static_cast<ncclComm_t>(comm)) == ncclSuccess ? ACMPC_OK : ACMPC_EHIP;
}

int acmpc_reduce_across_ranks(acmpc_ctx* c, void* rccl_comm, int64_t* d_keys, int32_t P, void* stream) {
  if (c == nullptr) return ACMPC_EINVAL;
  if (rccl_comm == nullptr || d_keys == nullptr) return fail(c, ACMPC_EINVAL, "null communicator or keys");
  if (P < 1 || P > c->prm.max_problems) return fail(c, ACMPC_ECAPACITY, "P exceeds the handle's capacity");
  const Rccl& api = rccl();
  if (api.all_reduce == nullptr) return fail(c, ACMPC_ESTATE, "no RCCL in the process and librccl.so.1 not loadable");
  const ncclResult_t rc = api.all_reduce(d_keys, d_keys, static_cast<size_t>(P), ncclInt64, ncclMin,
                                         static_cast<ncclComm_t>(rccl_comm), static_cast<hipStream_t>(stream));
  if (rc != ncclSuccess) {
    std::string msg = "ncclAllReduce: ";
    msg += (api.error_string != nullptr) ? api.error_string(rc) : "error";
    return fail(c, ACMPC_EHIP, msg.c_str());
  }
  return ACMPC_OK;
}

}  // extern "C"
