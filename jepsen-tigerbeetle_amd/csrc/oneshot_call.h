// oneshot_call.h -- what the one-shot entry points that take op columns (tbc_ledger_check, tbc_ledger_realtime, tbc_perf_series) share
// on the host: the HIP error macro, the device check, and what one call makes on the device, released on every path out.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "tbc_internal.h"

#define TBC_ONESHOT_TRY(expr)                                                                     \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      tbc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
      return e_ == hipErrorOutOfMemory ? TBC_ERR_OOM : TBC_ERR_HIP;                               \
    }                                                                                             \
  } while (0)

namespace tbc {

// what one call makes on the device: released in this order whichever way the call ends
struct OneShotCall {
  int device_before = -1;                                   // the calling thread's current device, put back on the way out
  void* arena = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~OneShotCall() {
    if (stream) (void)hipStreamSynchronize(stream);       // (a call that failed half way may have left a copy or a kernel in flight)
    if (arena) (void)hipFree(arena);
    for (hipEvent_t e : {ev0, ev1}) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (device_before >= 0) (void)hipSetDevice(device_before);
  }
};

inline tbc_status oneshot_check_device(uint32_t device) {
  int ndev = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || (int)device >= ndev) { set_error("no usable HIP device; libtbcheck has no CPU fallback"); return TBC_ERR_NO_DEVICE; }
  if (hipGetDeviceProperties(&prop, (int)device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_error("device %u is not a gfx950 (MI355X) device", device); return TBC_ERR_NO_DEVICE; }
  return TBC_OK;
}

}  // namespace tbc
