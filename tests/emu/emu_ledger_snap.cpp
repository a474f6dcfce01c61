// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger_snap.cpp: tbc_ledger_snapshots on the CPU -- the validation and the host plan of
// csrc/ledger_snap_plan.h, the arena laid out and filled as csrc/ledger_snap_host.hip does it (the one image of the head and the gathered
// columns, the zeroed and the all-ones regions; everything else a pattern, so that what a kernel does not write shows), and the kernels
// of csrc/ledger_snap_kernels.h (the very file hipcc compiles into libtbcheck.so) under the wavefront / workgroup emulator, in the order
// and under the conditions of lgsn::launch_filter and lgsn::launch_rest (csrc/ledger_snap.hip).  Every grid that strides is capped at
// `grid_cap` workgroups, so that the strides run (the pair kernel: as many slices of tiles at most); `sort_chunks_cap` and `scan_rows`
// are the plan's: a few chunks make a sort chunk several wavefronts' worth, a few rows a chunk give the scan's carry several steps.
// Built as a shared object by tests/test_ledger_snapshots_emu.py, which compares what comes back with snapshots_numpy of
// jepsen/ledger.py.  The atomics the kernels use are stated here (between two rendezvous the emulator runs one lane at a time).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "tbcheck.h"
#define TBC_EMU 1
#include "wave_env_emu.h"
#include "wave_env_wg_emu.h"

#define __global__
#define __launch_bounds__(...)
#define __forceinline__ inline
#define __shared__ static
#define __popcll(x) __builtin_popcountll(x)
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p |= v; return o; }
static inline uint32_t atomicMin(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v < o) *p = v; return o; }
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v > o) *p = v; return o; }

#include "ledger_snap_plan.h"
#include "ledger_snap_kernels.h"

namespace {
std::string g_err;
void trampoline(void* arg, uint32_t) { (*static_cast<std::function<void()>*>(arg))(); }
uint64_t g_launches, g_pair_launches;
void launch(std::function<void()> body, uint32_t grid, int waves, uint64_t seed) {
  for (uint32_t b = 0; b < grid; b++) wv::run_workgroup(trampoline, &body, waves, b, seed + 1000u * g_launches + b);
  g_launches++;
}
uint32_t grid_of(unsigned long long items, uint32_t per, uint32_t cap) {
  return (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>((items + per - 1u) / per, cap));
}
}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_snap_error says why)
// sort_chunks_cap, scan_rows: 0 = the library's own
extern "C" int emu_snap_check(const tbc_ledger_in* in, tbc_ledger_snap_out* out, uint32_t grid_cap, uint64_t seed, uint32_t sort_chunks_cap, uint32_t scan_rows) {
  g_err.clear();
  g_launches = g_pair_launches = 0;
  if (!grid_cap) grid_cap = 1;
  if (!lgsn::validate("emu_snap_check", in, g_err)) return TBC_ERR_INVALID_ARG;
  lgsn::Plan P;
  if (!lgsn::plan("emu_snap_check", in, P, g_err, sort_chunks_cap ? sort_chunks_cap : lgsn::kSnSortChunksMax, scan_rows ? scan_rows : lgsn::kSnScanRows)) return TBC_ERR_INVALID_ARG;
  const lgsn::SnArena& L = P.arena;
  std::vector<unsigned char> arena(L.bytes + 256, 0xA5);
  char* const base = reinterpret_cast<char*>(arena.data());
  const auto at = [&](const lg::LgRegion& r) { return base + r.at; };
  const std::vector<unsigned char> img = lgsn::image(in, P);
  std::memcpy(base, img.data(), img.size());
  std::memset(at(L.val), 0, L.zero_bytes());
  std::memset(at(L.skew_first), 0xFF, L.ones_bytes());
  const lgsn::SnArgs A = lgsn::args(in, P, base);
  // ---- lgsn::launch_filter, with every grid capped
  if (A.n_reads) {
    const uint32_t grid_layout = grid_of(A.n_reads, 4u, grid_cap);
    launch([&] { sn_layout_kernel(A, grid_layout); }, grid_layout, 4, seed);
  }
  if (A.n_reads && A.n_class) {
    const uint32_t grid_sort = std::min(A.sort_chunks, grid_cap);
    for (uint32_t pass = 0; pass < lgsn::kSnDigits; pass++) {
      launch([&] { sn_hist_kernel(A, pass, grid_sort); }, grid_sort, 1, seed);
      launch([&] { sn_carry_kernel(A); }, 1, 4, seed);
      launch([&] { sn_scatter_kernel(A, pass, grid_sort); }, grid_sort, 1, seed);
    }
    // the order is sorted by (key, read number), and it is a permutation
    std::vector<uint8_t> seen(A.n_reads, 0);
    for (uint32_t p = 0; p < A.n_reads; p++) {
      const uint32_t r = A.sort_perm[0][p];
      if (r >= A.n_reads || seen[r]) { g_err = "the sorted order is no permutation of the reads"; return -1; }
      seen[r] = 1;
      if (p && (A.sort_key[0][p - 1] > A.sort_key[0][p] || (A.sort_key[0][p - 1] == A.sort_key[0][p] && A.sort_perm[0][p - 1] > r))) { g_err = "the reads are not in the order of (sum, read number)"; return -1; }
    }
    const uint32_t grid_scan = grid_of((unsigned long long)A.scan_chunks * A.n_class, 256u, grid_cap);
    const uint32_t grid_carry = std::min<uint32_t>(A.n_class, grid_cap);
    launch([&] { sn_extremes_kernel(A, grid_scan); }, grid_scan, 4, seed);
    launch([&] { sn_scan_carry_kernel(A, grid_carry); }, grid_carry, 4, seed);
    launch([&] { sn_flag_kernel(A, grid_scan); }, grid_scan, 4, seed);
    const uint32_t grid_reads = grid_of(A.n_reads, 256u, grid_cap);
    launch([&] { sn_compact_kernel(A, grid_reads); }, grid_reads, 4, seed);
  }
  // ---- lgsn::launch_rest
  const uint32_t n_candidates = A.acc->bad_values ? 0u : A.acc->n_candidates;
  if (A.n_reads) {
    if (n_candidates) {
      const uint32_t n_blocks = (n_candidates + 255u) / 256u, n_tiles = (A.n_reads + lgsn::kSnTile - 1u) / lgsn::kSnTile;
      const uint32_t n_slices = std::max<uint32_t>(1u, std::min<uint32_t>(n_tiles, grid_cap));
      launch([&] { sn_pair_kernel(A, n_candidates, n_blocks, n_slices); }, n_blocks * n_slices, 4, seed);
      g_pair_launches++;
    }
    const uint32_t grid = grid_of(A.n_reads, 256u, grid_cap);
    launch([&] { sn_keys_kernel(A, grid); }, grid, 4, seed);
    launch([&] { sn_count_kernel(A, grid); }, grid, 4, seed);
    launch([&] { sn_worst_kernel(A, grid); }, grid, 4, seed);
  }
  launch([&] { sn_summary_kernel(A); }, 1, 1, seed);
  std::memcpy(&out->summary, at(L.summary), sizeof(tbc_ledger_snap_summary));
  out->summary.ns_device = 0; out->summary.bytes_in = img.size();
  if (out->summary.bad_values) { g_err = "emu_snap_check: reads hold counters whose magnitudes add up to 2^63 or more"; return TBC_ERR_UNSUPPORTED; }
  const auto get = [&](void* dst, const lg::LgRegion& r, size_t bytes) { if (dst && bytes) std::memcpy(dst, at(r), bytes); };
  const size_t R = P.n_reads;
  get(out->skew_count, L.skew_count, R * 4); get(out->skew_first, L.skew_first, R * 4); get(out->skew_key, L.skew_key, R * 8); get(out->snap_flags, L.snap_flags, R);
  return 0;
}

extern "C" const char* emu_snap_error() { return g_err.c_str(); }
// how many pair kernels the last call launched (0 or 1)
extern "C" uint64_t emu_snap_pair_launches() { return g_pair_launches; }
// the plan's shape: reads, classes, micro-ops, sort chunks, sort chunk entries, scan rows, scan chunks, image bytes
extern "C" int emu_snap_shape(const tbc_ledger_in* in, uint64_t* out8) {
  lgsn::Plan P;
  if (!lgsn::validate("emu_snap_shape", in, g_err) || !lgsn::plan("emu_snap_shape", in, P, g_err)) return 1;
  out8[0] = P.n_reads; out8[1] = P.n_class; out8[2] = P.n_mops; out8[3] = P.sort_chunks; out8[4] = P.sort_chunk_entries; out8[5] = P.scan_rows; out8[6] = P.scan_chunks;
  out8[7] = P.arena.image_bytes();
  return 0;
}
