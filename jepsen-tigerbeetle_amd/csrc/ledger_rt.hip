// ledger_rt.hip -- the kernels of tbc_ledger_realtime (ledger_rt_kernels.h) and their launches; ledger_rt_host.hip (validation, plan, arena,
// copies) calls lgrt::launch.  A kernel with nothing to do is not launched: a stream without entries, no reads; without accounts only the numbering runs (it counts the sides and the amounts).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "ledger_rt_kernels.h"

namespace lgrt {

template <bool kReads>
static void launch_stream(hipStream_t s, const RtArgs& A, RtStream S, uint32_t count_sides) {
  if (!S.n_entries) return;
  S.grid = std::min<uint32_t>(S.n_chunks, 8192u);
  hipLaunchKernelGGL(rt_number_kernel<kReads>, dim3(S.grid), dim3(64), 0, s, A, S, count_sides);
  if (!A.n_class) return;                                                   // (no account: every side was counted as naming none, and there is no list)
  RtStream C = S;
  C.grid = std::min<uint32_t>(A.n_class, 4096u);
  hipLaunchKernelGGL(rt_carry_kernel<kReads>, dim3(C.grid), dim3(256), 0, s, A, C);
  hipLaunchKernelGGL(rt_offsets_kernel, dim3(1), dim3(256), 0, s, A, S);
  hipLaunchKernelGGL(rt_scan_kernel<kReads>, dim3(S.grid), dim3(64), 0, s, A, S);
}

void launch(void* stream, RtArgs A) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_stream<false>(s, A, A.s[kDefinite], 0u);
  launch_stream<false>(s, A, A.s[kPossible], 1u);
  launch_stream<true>(s, A, A.s[kReads], 0u);
  if (A.n_read_mops) {
    A.grid_query = (uint32_t)std::min<unsigned long long>((A.n_read_mops + 255u) / 256u, 16384u);
    hipLaunchKernelGGL(rt_query_kernel, dim3(A.grid_query), dim3(256), 0, s, A);
  }
  if (A.n_reads) {
    const uint32_t grid = std::min<uint32_t>((A.n_reads + 255u) / 256u, 16384u);
    hipLaunchKernelGGL(rt_count_kernel, dim3(grid), dim3(256), 0, s, A, grid);
    hipLaunchKernelGGL(rt_worst_kernel, dim3(grid), dim3(256), 0, s, A, grid);
  }
  hipLaunchKernelGGL(rt_summary_kernel, dim3(1), dim3(64), 0, s, A);
}

}  // namespace lgrt
