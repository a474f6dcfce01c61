// oneshot_launch.h -- the library's launcher (oneshot_plan.h, "the launcher convention"): what ledger.hip, ledger_rt.hip,
// ledger_snap.hip and perf.hip run their kernels' sequences over.  A launch is hipLaunchKernelGGL on the call's stream; a strided
// kernel's grid is capped at the sequence's own cap and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "oneshot_plan.h"

namespace oneshot {

struct DeviceLauncher {
  hipStream_t stream;
  explicit DeviceLauncher(void* s) : stream(static_cast<hipStream_t>(s)) {}
  uint32_t grid(uint64_t blocks, uint32_t cap) const { return capped_grid(blocks, cap); }
  template <class... P, class... A>
  void launch(void (*kernel)(P...), uint32_t grid, uint32_t threads, const A&... args) const {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, stream, static_cast<P>(args)...);
  }
};

}  // namespace oneshot
