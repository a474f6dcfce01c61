// ledger_snap.hip -- the kernels of tbc_ledger_snapshots (ledger_snap_kernels.h) and their launches; ledger_snap_host.hip (validation,
// plan, arena, copies) calls lgsn::launch_filter, reads the candidates' number back and calls lgsn::launch_rest.  A kernel with nothing
// to do is not launched: no reads -- only the summary; no accounts -- no counter, so no sort, no scan and no candidate; no candidate
// -- no pair kernel.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "ledger_snap_kernels.h"

namespace lgsn {

static uint32_t grid_of(unsigned long long items, uint32_t per, uint32_t cap) {
  return (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>((items + per - 1u) / per, cap));
}

void launch_filter(void* stream, const SnArgs& A) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!A.n_reads) return;
  const uint32_t grid_layout = grid_of(A.n_reads, 4u, 4096u);                // (a wavefront per read, four to a workgroup)
  hipLaunchKernelGGL(sn_layout_kernel, dim3(grid_layout), dim3(256), 0, s, A, grid_layout);
  if (!A.n_class) return;
  const uint32_t grid_sort = A.sort_chunks;                                 // (kSnSortChunksMax at most)
  for (uint32_t pass = 0; pass < kSnDigits; pass++) {
    hipLaunchKernelGGL(sn_hist_kernel, dim3(grid_sort), dim3(64), 0, s, A, pass, grid_sort);
    hipLaunchKernelGGL(sn_carry_kernel, dim3(1), dim3(256), 0, s, A);
    hipLaunchKernelGGL(sn_scatter_kernel, dim3(grid_sort), dim3(64), 0, s, A, pass, grid_sort);
  }
  const uint32_t grid_scan = grid_of((unsigned long long)A.scan_chunks * A.n_class, 256u, 16384u);
  const uint32_t grid_carry = std::min<uint32_t>(A.n_class, 4096u);
  hipLaunchKernelGGL(sn_extremes_kernel, dim3(grid_scan), dim3(256), 0, s, A, grid_scan);
  hipLaunchKernelGGL(sn_scan_carry_kernel, dim3(grid_carry), dim3(256), 0, s, A, grid_carry);
  hipLaunchKernelGGL(sn_flag_kernel, dim3(grid_scan), dim3(256), 0, s, A, grid_scan);
  const uint32_t grid_reads = grid_of(A.n_reads, 256u, 16384u);
  hipLaunchKernelGGL(sn_compact_kernel, dim3(grid_reads), dim3(256), 0, s, A, grid_reads);
}

void launch_rest(void* stream, const SnArgs& A, uint32_t n_candidates) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A.n_reads) {
    if (n_candidates) {
      // the candidates in blocks of 256, the tiles of reads in as many slices as make about 2,048 workgroups
      const uint32_t n_blocks = (n_candidates + 255u) / 256u, n_tiles = (A.n_reads + kSnTile - 1u) / kSnTile;
      const uint32_t n_slices = std::max<uint32_t>(1u, std::min<uint32_t>(n_tiles, 2048u / std::min<uint32_t>(n_blocks, 2048u)));
      hipLaunchKernelGGL(sn_pair_kernel, dim3(n_blocks * n_slices), dim3(256), 0, s, A, n_candidates, n_blocks, n_slices);
    }
    const uint32_t grid = grid_of(A.n_reads, 256u, 16384u);
    hipLaunchKernelGGL(sn_keys_kernel, dim3(grid), dim3(256), 0, s, A, grid);
    hipLaunchKernelGGL(sn_count_kernel, dim3(grid), dim3(256), 0, s, A, grid);
    hipLaunchKernelGGL(sn_worst_kernel, dim3(grid), dim3(256), 0, s, A, grid);
  }
  hipLaunchKernelGGL(sn_summary_kernel, dim3(1), dim3(64), 0, s, A);
}

}  // namespace lgsn
