// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_perf.cpp: tbc_perf_series on the CPU -- the validation and the host plan of
// csrc/perf_plan.h, the arena laid out and filled as csrc/perf_host.hip does it (the zeroed head, the partner column, the caller's
// columns; everything else a pattern, so that what a kernel does not write shows), and the kernels of csrc/perf_kernels.h (the very file
// hipcc compiles into libtbcheck.so) under the wavefront / workgroup emulator, in the order and under the conditions of pf::launch
// (csrc/perf.hip).  The select's LDS tile is PF_SELECT_TILE = 32 latencies here (the library's is TBC_PERF_SELECT_TILE), so that a cell
// of a few dozen takes the radix select; every grid is capped at `grid_cap` workgroups, so that the grid strides run.
// Built as a shared object by tests/test_perf_emu.py, which compares what comes back with the host statement of jepsen/perf.py.
// The emulator headers have ballots, lane reads and the workgroup barrier; the atomics and the lane shuffle the kernels use are stated
// here (between two rendezvous the emulator runs one lane at a time).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#ifndef PF_SELECT_TILE
#define PF_SELECT_TILE 32u
#endif
#include "tbcheck.h"
#define TBC_EMU 1
#include "wave_env_emu.h"
#include "wave_env_wg_emu.h"

#define __global__
#define __launch_bounds__(...)
#define __forceinline__ inline
#define __shared__ static
#define __popcll(x) __builtin_popcountll(x)
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
// a lane shuffle is a rendezvous: every lane deposits, each reads its partner's deposit
static inline uint64_t emu_shfl(uint64_t v, int src_of_me, int site) {
  const int me = (int)wv::lane_id();
  const uint64_t* s = wv::gather(v, site);
  return src_of_me >= 0 && src_of_me < 64 ? s[src_of_me] : s[me];
}
#define __shfl_up(v, d) ((decltype(v))emu_shfl((uint64_t)(uint32_t)(v), (int)wv::lane_id() - (d), 300000 + __LINE__))
#define __shfl(v, src) ((decltype(v))emu_shfl((uint64_t)(uint32_t)(v), (int)(src), 400000 + __LINE__))
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v > o) *p = v; return o; }
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; if (v > o) *p = v; return o; }

#include "perf_plan.h"
#include "perf_kernels.h"

namespace {
std::string g_err;
void trampoline(void* arg, uint32_t) { (*static_cast<std::function<void()>*>(arg))(); }
}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_pf_error says why)
extern "C" int emu_pf_series(const tbc_perf_in* in, tbc_perf_out* out, uint32_t grid_cap, uint64_t seed) {
  g_err.clear();
  tbc_status st = pf::validate("emu_pf_series", in, g_err);
  if (st != TBC_OK) return st;
  pf::Plan P;
  st = pf::plan("emu_pf_series", in, P, g_err);
  if (st != TBC_OK) return st;
  const pf::PfArena& L = P.arena;
  std::vector<unsigned char> arena(L.bytes + 256, 0xA5);
  char* const base = reinterpret_cast<char*>(arena.data());
  const auto at = [&](const pf::PfRegion& r) { return base + r.at; };
  std::memset(base, 0, L.zero_bytes());
  const auto put = [&](const pf::PfRegion& r, const void* src) { if (r.bytes) std::memcpy(at(r), src, r.bytes); };
  put(L.partner, P.partner.data()); put(L.time, in->time); put(L.process, in->process); put(L.type, in->type); put(L.f, in->f);
  pf::PfArgs A = pf::args(P, base);
  // ---- pf::launch, with every grid capped
  uint64_t launches = 0;
  const auto go = [&](void (*kernel)(pf::PfArgs), uint64_t blocks, bool capped, int waves) {
    if (!blocks) return;
    A.grid = (uint32_t)(capped ? std::min<uint64_t>(blocks, grid_cap ? grid_cap : 1u) : blocks);
    std::function<void()> body = [&] { kernel(A); };
    for (uint32_t b = 0; b < A.grid; b++) wv::run_workgroup(trampoline, &body, waves, b, seed + 1000u * launches + b);
    launches++;
  };
  const uint64_t op_blocks = ((uint64_t)A.n_ops + 255u) / 256u;
  go(pf_classify_kernel, op_blocks, true, 4);
  if (A.n_class) go(pf_open_totals_kernel, A.n_chunks, true, 1);
  go(pf_open_carry_kernel, A.n_chunks ? A.n_class : 0u, true, 4);
  go(pf_open_scan_kernel, A.n_chunks, true, 1);
  go(pf_cell_sum_kernel, A.n_scan_tiles, true, 4);
  go(pf_tile_scan_kernel, A.n_scan_tiles ? 1u : 0u, true, 4);
  go(pf_cell_offsets_kernel, A.n_scan_tiles, true, 4);
  go(pf_gather_kernel, A.n_cells ? op_blocks : 0u, true, 4);
  go(pf_select_kernel, A.n_cells, true, 4);
  go(pf_fill_kernel, A.n_class, true, 1);
  go(pf_summary_kernel, 1u, true, 1);
  // every cell's cursor has come to the end of the cell
  {
    const uint32_t *off = A.q_off, *cur = A.q_cur, *cnt = A.q_count;
    for (uint32_t c = 0; c < A.n_cells; c++)
      if (cur[c] != off[c] + cnt[c]) { g_err = "a cell's cursor is not at the cell's end"; return -1; }
  }
  const auto get = [&](void* dst, const pf::PfRegion& r) { if (dst && r.bytes) std::memcpy(dst, at(r), r.bytes); };
  get(out->op_latency, L.op_latency); get(out->op_outcome, L.op_outcome); get(out->op_open_after, L.op_open_after);
  get(out->q_count, L.q_count); get(out->q_value, L.q_value); get(out->rate_count, L.rate_count);
  get(out->open_last, L.open_last); get(out->open_fill, L.open_fill); get(&out->summary, L.summary);
  out->summary.ns_device = 0; out->summary.bytes_in = 0;
  return 0;
}

extern "C" int emu_pf_plan_sizes(const tbc_perf_in* in, tbc_perf_sizes* sizes) {
  g_err.clear();
  tbc_status st = pf::validate("emu_pf_plan_sizes", in, g_err);
  if (st == TBC_OK) st = pf::sizes("emu_pf_plan_sizes", in, *sizes, g_err);
  return st;
}
extern "C" const char* emu_pf_error() { return g_err.c_str(); }
extern "C" uint32_t emu_pf_tile() { return pf::kPfTile; }
// the plan's shape: chunk_ops, n_chunks, n_scan_tiles, n_matched, n_cells, n_class
extern "C" int emu_pf_shape(const tbc_perf_in* in, uint64_t* out6) {
  pf::Plan P;
  if (pf::validate("emu_pf_shape", in, g_err) != TBC_OK || pf::plan("emu_pf_shape", in, P, g_err) != TBC_OK) return 1;
  out6[0] = P.chunk_ops; out6[1] = P.n_chunks; out6[2] = P.n_scan_tiles; out6[3] = P.n_matched; out6[4] = P.n_cells; out6[5] = P.n_class;
  return 0;
}
