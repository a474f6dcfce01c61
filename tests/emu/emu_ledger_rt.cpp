// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger_rt.cpp: tbc_ledger_realtime on the CPU -- the validation and the host plan of
// csrc/ledger_rt_plan.h, the steps of the call as lgrt::steps of that header states them -- the list csrc/ledger_rt_host.hip runs --
// over the emulator's call frame, and the kernels of csrc/ledger_rt_kernels.h (the very file hipcc compiles into libtbcheck.so)
// under the wavefront / workgroup emulator, launched by lgrt::sequence of that file -- the library's own statement -- over the
// emulator's launcher (oneshot_emu.h).  Every grid that strides is capped at `grid_cap` workgroups, so that the strides run; at the
// sizes of the tests a chunk is one wavefront's 64 entries unless `chunks_cap` says otherwise.  Built as a shared object by
// tests/test_ledger_realtime_emu.py, which compares what comes back with realtime_numpy of jepsen/ledger.py.
#include "oneshot_emu.h"
#include "ledger_rt_plan.h"
#include "ledger_rt_kernels.h"

namespace {
std::string g_err;
}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_rt_error says why)
// chunks_cap: 0 = the library's own; otherwise the most chunks per stream (a few: a chunk is then several wavefronts' worth of entries)
extern "C" int emu_rt_check(const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out, uint32_t grid_cap, uint64_t seed, uint32_t chunks_cap) {
  g_err.clear();
  if (!lgrt::validate("emu_rt_check", in, g_err)) return TBC_ERR_INVALID_ARG;
  lgrt::Plan P;
  if (!lgrt::plan("emu_rt_check", in, P, g_err, chunks_cap ? chunks_cap : lgrt::kRtChunksMax)) return TBC_ERR_INVALID_ARG;
  struct Run { emu::Launcher go; void sequence(const lgrt::RtArgs& A) { lgrt::sequence(go, A); } };
  emu::Arena C(g_err);
  C.open(in->ledger.device, P.arena.bytes);
  lgrt::steps("emu_rt_check", C, Run{emu::Launcher(grid_cap, seed)}, in, P, out);
  if (C.close() != TBC_OK && C.status != TBC_ERR_UNSUPPORTED) return C.status;
  // every list is full: each stream's lists hold as many entries as the numbering gave a class, in ascending position order
  const lgrt::RtArgs A = lgrt::args(in, P, C.base());
  for (int k = 0; k < lgrt::kStreams; k++) {
    const lgrt::RtStream& S = A.s[k];
    uint64_t with_class = 0;
    for (uint64_t e = 0; e < S.n_entries; e++) with_class += S.ent_cls[e] != lgrt::kRtNone;
    if (S.n_entries && A.n_class && S.off[A.n_class] != with_class) { g_err = "a stream's lists do not hold every entry that has a class"; return -1; }
    for (uint32_t c = 0; S.n_entries && c < A.n_class; c++)
      for (uint32_t i = S.off[c] + 1u; i < S.off[c + 1u]; i++)
        if (S.list_pos[i] < S.list_pos[i - 1u]) { g_err = "a list is not in position order"; return -1; }
  }
  return C.status;
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
