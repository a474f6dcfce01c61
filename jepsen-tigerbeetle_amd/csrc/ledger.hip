// ledger.hip -- the kernels of tbc_ledger_check (ledger_kernels.h) and their launches; ledger_host.hip (validation, plan, arena, copies)
// calls lg::launch.  A kernel with nothing to do is not launched: no reads, no invoked transfers, fewer than two final rows of a kind.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "ledger_kernels.h"

namespace lg {

void launch(void* stream, LgArgs A, unsigned long long fr_mops, unsigned long long fl_mops) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto blocks = [](unsigned long long n, uint32_t cap) { return (uint32_t)std::min<unsigned long long>((n + 255u) / 256u, cap); };
  A.grid_si = std::min<uint32_t>(A.n_runs, 16384u);
  A.grid_lookup = std::min<uint32_t>(A.n_final_lookups, 4096u);
  if (A.n_runs) hipLaunchKernelGGL(lg_si_kernel, dim3(A.grid_si), dim3(256), 0, s, A);
  if (A.n_transfers) hipLaunchKernelGGL(lg_table_build_kernel, dim3((A.n_transfers + 255u) / 256u), dim3(256), 0, s, A);
  if (A.n_transfers && A.n_final_lookups)
    hipLaunchKernelGGL(lg_lookup_kernel<TBC_LEDGER_LOOKUP_WINDOW_WORDS>, dim3(A.grid_lookup), dim3(256), 0, s, A);
  if (A.n_final_reads >= 2u) {
    const LgRows F{A.fr_lo, A.fr_cum, A.n_final_reads, std::max(1u, blocks(fr_mops, 8192u)), A.fr_unlike};
    hipLaunchKernelGGL(lg_rows_equal_kernel, dim3(F.grid), dim3(256), 0, s, A, F);
  }
  if (A.n_final_lookups >= 2u) {
    const LgRows F{A.fl_lo, A.fl_cum, A.n_final_lookups, std::max(1u, blocks(fl_mops, 8192u)), A.fl_unlike};
    hipLaunchKernelGGL(lg_rows_equal_kernel, dim3(F.grid), dim3(256), 0, s, A, F);
  }
  const uint32_t n_threads = std::max(A.n_reads, std::max(A.n_final_reads, A.n_final_lookups));
  if (n_threads) hipLaunchKernelGGL(lg_finish_kernel, dim3((n_threads + 255u) / 256u), dim3(256), 0, s, A, n_threads);
  hipLaunchKernelGGL(lg_summary_kernel, dim3(1), dim3(64), 0, s, A);
}

}  // namespace lg
