// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger_rt.cpp: tbc_ledger_realtime on the CPU -- the validation and the host plan of
// csrc/ledger_rt_plan.h, the arena laid out and filled as csrc/ledger_rt_host.hip does it (the one image of the head and the gathered
// columns, the zeroed regions; everything else a pattern, so that what a kernel does not write shows), and the kernels of csrc/ledger_rt_kernels.h (the
// very file hipcc compiles into libtbcheck.so) under the wavefront / workgroup emulator, in the order and under the conditions of
// lgrt::launch (csrc/ledger_rt.hip).  Every grid is capped at `grid_cap` workgroups, so that the grid strides run; at the sizes of the
// tests a chunk is one wavefront's 64 entries unless `chunks_cap` says otherwise.  Built as a shared object by tests/test_ledger_realtime_emu.py, which compares what comes
// back with realtime_numpy of jepsen/ledger.py.  The atomics the kernels use are stated here (between two rendezvous the emulator runs
// one lane at a time).
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
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; if (v > o) *p = v; return o; }

#include "ledger_rt_plan.h"
#include "ledger_rt_kernels.h"

namespace {
std::string g_err;
void trampoline(void* arg, uint32_t) { (*static_cast<std::function<void()>*>(arg))(); }
uint64_t g_launches;
void launch(std::function<void()> body, uint32_t grid, int waves, uint64_t seed) {
  for (uint32_t b = 0; b < grid; b++) wv::run_workgroup(trampoline, &body, waves, b, seed + 1000u * g_launches + b);
  g_launches++;
}

template <bool kReads>
void launch_stream(const lgrt::RtArgs& A, lgrt::RtStream S, uint32_t count_sides, uint32_t grid_cap, uint64_t seed) {
  if (!S.n_entries) return;
  S.grid = std::min<uint32_t>(S.n_chunks, grid_cap);
  launch([&] { rt_number_kernel<kReads>(A, S, count_sides); }, S.grid, 1, seed);
  if (!A.n_class) return;
  lgrt::RtStream C = S;
  C.grid = std::min<uint32_t>(A.n_class, grid_cap);
  launch([&] { rt_carry_kernel<kReads>(A, C); }, C.grid, 4, seed);
  launch([&] { rt_offsets_kernel(A, S); }, 1, 4, seed);
  launch([&] { rt_scan_kernel<kReads>(A, S); }, S.grid, 1, seed);
}
}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_rt_error says why)
// chunks_cap: 0 = the library's own; otherwise the most chunks per stream (a few: a chunk is then several wavefronts' worth of entries)
extern "C" int emu_rt_check(const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out, uint32_t grid_cap, uint64_t seed, uint32_t chunks_cap) {
  g_err.clear();
  g_launches = 0;
  if (!grid_cap) grid_cap = 1;
  if (!lgrt::validate("emu_rt_check", in, g_err)) return TBC_ERR_INVALID_ARG;
  lgrt::Plan P;
  if (!lgrt::plan("emu_rt_check", in, P, g_err, chunks_cap ? chunks_cap : lgrt::kRtChunksMax)) return TBC_ERR_INVALID_ARG;
  const lgrt::RtArena& L = P.arena;
  std::vector<unsigned char> arena(L.bytes + 256, 0xA5);
  char* const base = reinterpret_cast<char*>(arena.data());
  const auto at = [&](const lg::LgRegion& r) { return base + r.at; };
  const std::vector<unsigned char> img = lgrt::image(in, P);
  std::memcpy(base, img.data(), img.size());
  std::memset(at(L.carry_cnt[0]), 0, L.zero_bytes());
  lgrt::RtArgs A = lgrt::args(in, P, base);
  // ---- lgrt::launch, with every grid capped
  launch_stream<false>(A, A.s[lgrt::kDefinite], 0u, grid_cap, seed);
  launch_stream<false>(A, A.s[lgrt::kPossible], 1u, grid_cap, seed);
  launch_stream<true>(A, A.s[lgrt::kReads], 0u, grid_cap, seed);
  if (A.n_read_mops) {
    A.grid_query = (uint32_t)std::min<unsigned long long>((A.n_read_mops + 255u) / 256u, grid_cap);
    launch([&] { rt_query_kernel(A); }, A.grid_query, 4, seed);
  }
  if (A.n_reads) {
    const uint32_t grid = std::min<uint32_t>((A.n_reads + 255u) / 256u, grid_cap);
    launch([&] { rt_count_kernel(A, grid); }, grid, 4, seed);
    launch([&] { rt_worst_kernel(A, grid); }, grid, 4, seed);
  }
  launch([&] { rt_summary_kernel(A); }, 1, 1, seed);
  // every list is full: each stream's lists hold as many entries as the numbering gave a class, in ascending position order
  for (int k = 0; k < lgrt::kStreams; k++) {
    const lgrt::RtStream& S = A.s[k];
    uint64_t with_class = 0;
    for (uint64_t e = 0; e < S.n_entries; e++) with_class += S.ent_cls[e] != lgrt::kRtNone;
    if (S.n_entries && A.n_class && S.off[A.n_class] != with_class) { g_err = "a stream's lists do not hold every entry that has a class"; return -1; }
    for (uint32_t c = 0; S.n_entries && c < A.n_class; c++)
      for (uint32_t i = S.off[c] + 1u; i < S.off[c + 1u]; i++)
        if (S.list_pos[i] < S.list_pos[i - 1u]) { g_err = "a list is not in position order"; return -1; }
  }
  std::memcpy(&out->summary, at(L.summary), sizeof(tbc_ledger_rt_summary));
  out->summary.ns_device = 0; out->summary.bytes_in = 0;
  if (out->summary.bad_amounts) { g_err = "emu_rt_check: transfer amounts outside [0, 2^31)"; return TBC_ERR_UNSUPPORTED; }
  const auto get = [&](void* dst, const lg::LgRegion& r, size_t bytes) { if (dst && bytes) std::memcpy(dst, at(r), bytes); };
  const size_t R = P.n_reads, Mr = (size_t)P.rows[lgrt::kReads].mops();
  get(out->rt_bits, L.rt_bits, R); get(out->rt_miss, L.rt_miss, R * 24);
  get(out->mop_lo, L.mop_lo, Mr * 16); get(out->mop_hi, L.mop_hi, Mr * 16); get(out->mop_floor, L.mop_floor, Mr * 16);
  return 0;
}

extern "C" const char* emu_rt_error() { return g_err.c_str(); }
// the plan's shape: per stream rows, micro-ops, chunks, chunk_entries (12 words), then reads, classes
extern "C" int emu_rt_shape(const tbc_ledger_rt_in* in, uint64_t* out14) {
  lgrt::Plan P;
  if (!lgrt::validate("emu_rt_shape", in, g_err) || !lgrt::plan("emu_rt_shape", in, P, g_err)) return 1;
  for (int k = 0; k < lgrt::kStreams; k++) {
    out14[4 * k] = P.rows[k].lo.size(); out14[4 * k + 1] = P.rows[k].mops(); out14[4 * k + 2] = P.rows[k].n_chunks; out14[4 * k + 3] = P.rows[k].chunk_entries;
  }
  out14[12] = P.n_reads; out14[13] = P.n_class;
  return 0;
}
