// perf.hip -- the kernels of tbc_perf_series (perf_kernels.h) and their launches; perf_host.hip (validation, plan, arena, copies) calls
// pf::launch.  A kernel with nothing to do is not launched: no ops, no f's (no client op: no cells and no classes).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "perf_kernels.h"

namespace pf {

void launch(void* stream, PfArgs A) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto go = [&](void (*kernel)(PfArgs), uint64_t blocks, uint32_t cap, uint32_t threads) {
    if (!blocks) return;
    A.grid = (uint32_t)std::min<uint64_t>(blocks, cap);
    hipLaunchKernelGGL(kernel, dim3(A.grid), dim3(threads), 0, s, A);
  };
  const uint64_t op_blocks = ((uint64_t)A.n_ops + 255u) / 256u;
  go(pf_classify_kernel, op_blocks, 8192u, 256u);
  if (A.n_class) go(pf_open_totals_kernel, A.n_chunks, 4096u, 64u);
  go(pf_open_carry_kernel, A.n_chunks ? A.n_class : 0u, 16384u, 256u);
  go(pf_open_scan_kernel, A.n_chunks, 4096u, 64u);                          // (without a client op it writes the zeros of op_open_after)
  go(pf_cell_sum_kernel, A.n_scan_tiles, 8192u, 256u);
  go(pf_tile_scan_kernel, A.n_scan_tiles ? 1u : 0u, 1u, 256u);
  go(pf_cell_offsets_kernel, A.n_scan_tiles, 8192u, 256u);
  go(pf_gather_kernel, A.n_cells ? op_blocks : 0u, 8192u, 256u);
  go(pf_select_kernel, A.n_cells, 16384u, 256u);
  go(pf_fill_kernel, A.n_class, 16384u, 64u);
  go(pf_summary_kernel, 1u, 1u, 64u);
}

}  // namespace pf
