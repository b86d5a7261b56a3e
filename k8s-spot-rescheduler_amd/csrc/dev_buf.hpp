// dev_buf.hpp — growing device and pinned host buffers, and HIP_TRY, for the units that call HIP (planner.cpp,
// query.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/sr_planner.h"

namespace sr {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
};

inline hipError_t dev_reserve(DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return hipSuccess;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t cap = std::max<size_t>(bytes + bytes / 4, 4096);
  hipError_t e = hipMalloc(&b.p, cap);
  if (e == hipSuccess) b.cap = cap;
  return e;
}

// Fresh pinned blocks are zeroed: the runtime may hand back memory an earlier
// context freed, and the tagged result words (mapped memory) must never carry
// a stale tag (run sequence numbers also come from one process-wide counter).
inline hipError_t host_reserve(HostBuf& b, size_t bytes) {
  if (bytes <= b.cap) return hipSuccess;
  if (b.p) (void)hipHostFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t cap = std::max<size_t>(bytes + bytes / 4, 4096);
  hipError_t e = hipHostMalloc(&b.p, cap, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) {
    b.cap = cap;
    std::memset(b.p, 0, cap);
  }
  return e;
}

inline sr_status hip_fail(std::string& err, hipError_t e, const char* what) {
  err = std::string(what) + ": " + hipGetErrorString(e);
  return SR_ERR_HIP;
}

}  // namespace sr

// Returns SR_ERR_HIP from the enclosing function, with the failed call and HIP's words for it as the context's
// error string.  `ctx`: whatever the unit's err_string(ctx) gives that string for.
#define HIP_TRY(ctx, expr)                                                      \
  do {                                                                          \
    hipError_t _e = (expr);                                                     \
    if (_e != hipSuccess) return sr::hip_fail(err_string(ctx), _e, #expr);      \
  } while (0)
