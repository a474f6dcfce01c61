// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_perf.cpp: tbc_perf_series on the CPU -- the validation and the host plan of
// csrc/perf_plan.h, the steps of the call as pf::steps of that header states them -- the list csrc/perf_host.hip runs -- over the
// emulator's call frame, and the kernels of csrc/perf_kernels.h (the very file hipcc compiles into libtbcheck.so) under the wavefront /
// workgroup emulator, launched by pf::sequence of that file -- the library's own statement -- over the emulator's launcher (oneshot_emu.h).  The
// select's LDS tile is PF_SELECT_TILE = 32 latencies here (the library's is TBC_PERF_SELECT_TILE), so that a cell of a few dozen takes
// the radix select; every grid that strides is capped at `grid_cap` workgroups, so that the strides run.
// Built as a shared object by tests/test_perf_emu.py, which compares what comes back with the host statement of jepsen/perf.py.
// The lane shuffle the kernels use is stated here.
#ifndef PF_SELECT_TILE
#define PF_SELECT_TILE 32u
#endif
#include "oneshot_emu.h"

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

#include "perf_plan.h"
#include "perf_kernels.h"

namespace {
std::string g_err;
}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_pf_error says why)
extern "C" int emu_pf_series(const tbc_perf_in* in, tbc_perf_out* out, uint32_t grid_cap, uint64_t seed) {
  g_err.clear();
  tbc_status st = pf::validate("emu_pf_series", in, g_err);
  if (st != TBC_OK) return st;
  pf::Plan P;
  st = pf::plan("emu_pf_series", in, P, g_err);
  if (st != TBC_OK) return st;
  struct Run { emu::Launcher go; void sequence(const pf::PfArgs& A) { pf::sequence(go, A); } };
  emu::Arena C(g_err);
  C.open(in->device, P.arena.bytes);
  pf::steps(C, Run{emu::Launcher(grid_cap, seed)}, in, P, out);
  if (C.close() != TBC_OK) return C.status;
  // every cell's cursor has come to the end of the cell
  const pf::PfArgs A = pf::args(P, C.base());
  for (uint32_t c = 0; c < A.n_cells; c++)
    if (A.q_cur[c] != A.q_off[c] + A.q_count[c]) { g_err = "a cell's cursor is not at the cell's end"; return -1; }
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
