// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger.cpp: tbc_ledger_check on the CPU -- the validation and the host plan of
// csrc/ledger_plan.h, the arena laid out and filled as csrc/ledger_host.hip does it (the head image, the caller's columns, the zeroed
// regions; everything else a pattern, so that what a kernel does not write shows), and the kernels of csrc/ledger_kernels.h (the very
// file hipcc compiles into libtbcheck.so) under the wavefront / workgroup emulator, in the order and under the conditions of
// lg::launch (csrc/ledger.hip).  The lookup kernel's window is EMU_W words here (the library's is TBC_LEDGER_LOOKUP_WINDOW_WORDS), so
// that a few hundred transfers span several windows; every grid is capped at `grid_cap` workgroups, so that the grid strides run.
// Built as a shared object by tests/test_ledger_emu.py, which compares what comes back with the host statement of jepsen/ledger.py.
// The emulator headers have ballots, lane reads and the workgroup barrier; the atomics the kernels use are stated here (between two
// rendezvous the emulator runs one lane at a time).
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
#define __popc(x) __builtin_popcount(x)
static inline uint32_t atomicCAS(uint32_t* p, uint32_t expected, uint32_t desired) { const uint32_t o = *p; if (o == expected) *p = desired; return o; }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p |= v; return o; }
static inline uint32_t atomicMin(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v < o) *p = v; return o; }
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v > o) *p = v; return o; }
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; if (v < o) *p = v; return o; }
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; if (v > o) *p = v; return o; }

#include "ledger_plan.h"
#include "ledger_kernels.h"

#ifndef EMU_W
#define EMU_W 8u
#endif

namespace {
std::string g_err;
void trampoline(void* arg, uint32_t) { (*static_cast<std::function<void()>*>(arg))(); }
void launch(std::function<void()> body, uint32_t grid, uint64_t seed) {
  for (uint32_t b = 0; b < grid; b++) wv::run_workgroup(trampoline, &body, 4, b, seed + b);
}
}  // namespace

// 0: checked; 1: refused (emu_lg_error says why)
extern "C" int emu_lg_check(const tbc_ledger_in* in, tbc_ledger_out* out, uint32_t grid_cap, uint64_t seed) {
  g_err.clear();
  if (!lg::validate("emu_lg_check", in, g_err)) return 1;
  lg::Plan P;
  if (!lg::plan("emu_lg_check", in, P, g_err)) return 1;
  const lg::LgArena& L = P.arena;
  std::vector<unsigned char> arena(L.bytes + 256, 0xA5);
  unsigned char* const base = arena.data();
  const auto at = [&](const lg::LgRegion& r) { return base + r.at; };
  const std::vector<unsigned char> img = lg::head_image(P);
  std::memcpy(base, img.data(), img.size());
  const auto put = [&](const lg::LgRegion& r, const void* src) { if (r.bytes) std::memcpy(at(r), src, r.bytes); };
  put(L.mop_id, in->mop_id); put(L.mop_a, in->mop_a); put(L.mop_b, in->mop_b); put(L.mop_c, in->mop_c); put(L.mop_flags, in->mop_flags);
  std::memset(at(L.slots), 0, L.zero_bytes());
  lg::LgArgs A{};
  A.acc = (lg::LgAcc*)at(L.acc); A.summary = (tbc_ledger_summary*)at(L.summary);
  A.mop_id = (const long long*)at(L.mop_id); A.mop_a = (const long long*)at(L.mop_a); A.mop_b = (const long long*)at(L.mop_b);
  A.mop_c = (const long long*)at(L.mop_c); A.mop_flags = (const uint8_t*)at(L.mop_flags);
  A.accounts = (const long long*)at(L.accounts); A.n_accounts = in->n_accounts; A.negative_balances = in->negative_balances;
  A.total_amount = in->total_amount;
  A.read_lo = (const unsigned long long*)at(L.read_lo); A.read_cum = (const unsigned long long*)at(L.read_cum);
  A.run_first = (const uint32_t*)at(L.run_first); A.n_reads = P.n_reads; A.n_runs = P.n_runs;
  A.read_error = (uint8_t*)at(L.read_error); A.read_total = (long long*)at(L.read_total); A.read_badness = (long long*)at(L.read_badness);
  A.transfer = (const long long*)at(L.transfer); A.slots = at(L.slots); A.n_transfers = P.n_transfers; A.tab_mask = P.tab_mask;
  A.fl_lo = (const unsigned long long*)at(L.fl_lo); A.fl_cum = (const unsigned long long*)at(L.fl_cum); A.n_final_lookups = P.n_final_lookups;
  A.missing = (uint32_t*)at(L.missing);
  A.fr_lo = (const unsigned long long*)at(L.fr_lo); A.fr_cum = (const unsigned long long*)at(L.fr_cum); A.n_final_reads = P.n_final_reads;
  A.fr_unlike = (uint32_t*)at(L.fr_unlike); A.fl_unlike = (uint32_t*)at(L.fl_unlike);
  // ---- lg::launch, with every grid capped
  const auto cap = [&](uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, grid_cap ? grid_cap : 1u)); };
  A.grid_si = cap(A.n_runs); A.grid_lookup = cap(A.n_final_lookups);
  if (A.n_runs) launch([&] { lg_si_kernel(A); }, A.grid_si, seed);
  if (A.n_transfers) launch([&] { lg_table_build_kernel(A); }, (A.n_transfers + 255u) / 256u, seed + 1000);
  if (A.n_transfers && A.n_final_lookups) launch([&] { lg_lookup_kernel<EMU_W>(A); }, A.grid_lookup, seed + 2000);
  if (A.n_final_reads >= 2u) {
    const lg::LgRows F{A.fr_lo, A.fr_cum, A.n_final_reads, cap((P.fr_cum.back() + 255u) / 256u), A.fr_unlike};
    launch([&] { lg_rows_equal_kernel(A, F); }, F.grid, seed + 3000);
  }
  if (A.n_final_lookups >= 2u) {
    const lg::LgRows F{A.fl_lo, A.fl_cum, A.n_final_lookups, cap((P.fl_cum.back() + 255u) / 256u), A.fl_unlike};
    launch([&] { lg_rows_equal_kernel(A, F); }, F.grid, seed + 4000);
  }
  const uint32_t n_threads = std::max(A.n_reads, std::max(A.n_final_reads, A.n_final_lookups));
  if (n_threads) launch([&] { lg_finish_kernel(A, n_threads); }, (n_threads + 255u) / 256u, seed + 5000);
  launch([&] { lg_summary_kernel(A); }, 1, seed + 6000);
  // every transfer id sits in the table exactly once
  {
    const SfEncSlot* tab = (const SfEncSlot*)at(L.slots);
    uint64_t used = 0;
    for (uint64_t s = 0; s < P.tab_slots; s++) used += tab[s].col1 != 0u;
    if (used != P.n_transfers) { g_err = "the table does not hold every transfer id once"; return 1; }
  }
  const auto get = [&](void* dst, const lg::LgRegion& r, size_t bytes) { if (dst && bytes) std::memcpy(dst, at(r), bytes); };
  const size_t R = P.n_reads, FR = P.n_final_reads, FL = P.n_final_lookups;
  get(out->read_error, L.read_error, R); get(out->read_total, L.read_total, R * 8); get(out->read_badness, L.read_badness, R * 8);
  get(out->lookup_missing, L.missing, FL * 4); get(out->final_read_unlike, L.fr_unlike, FR); get(out->final_lookup_unlike, L.fl_unlike, FL);
  get(&out->summary, L.summary, sizeof(tbc_ledger_summary));
  out->summary.ns_device = 0; out->summary.bytes_in = 0;
  return 0;
}

extern "C" const char* emu_lg_error() { return g_err.c_str(); }
extern "C" uint32_t emu_lg_window_words() { return EMU_W; }
// the plan's shape: reads, runs, final reads, final lookups, transfers, table slots
extern "C" int emu_lg_shape(const tbc_ledger_in* in, uint64_t* out6) {
  lg::Plan P;
  if (!lg::validate("emu_lg_shape", in, g_err) || !lg::plan("emu_lg_shape", in, P, g_err)) return 1;
  out6[0] = P.n_reads; out6[1] = P.n_runs; out6[2] = P.n_final_reads; out6[3] = P.n_final_lookups; out6[4] = P.n_transfers; out6[5] = P.tab_slots;
  return 0;
}
