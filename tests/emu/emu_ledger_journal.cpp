// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger_journal.cpp: tbc_ledger_journal on the CPU -- the validation and the host plan of
// csrc/ledger_journal_plan.h, the steps of the call as lgjn::steps of that header states them -- the list csrc/ledger_journal_host.hip
// runs -- over the emulator's call frame, and the kernels of csrc/ledger_journal_kernels.h (the very file hipcc compiles into
// libtbcheck.so) under the wavefront / workgroup emulator, launched by lgjn::sequence of that file -- the library's own statement -- over
// the emulator's launcher (oneshot_emu.h).  Every grid that strides is capped at `grid_cap` workgroups, so that the strides run;
// `slice_entries` and `chunk` are the plan's: a few entries a slice cut a lookup over several workgroups, whose rows of the bitmap are
// OR-ed; 64 micro-ops a chunk give the members kernel several chunks, and with a chunk given its tiles are 3 lookups; the LDS window is kEmuWindowWords words, so that records past it
// take the global path.  Built as a shared object by tests/test_ledger_journal_emu.py, which compares what comes back with journal_numpy
// of jepsen/ledger.py.
#include "oneshot_emu.h"
#include "ledger_journal_plan.h"
#include "ledger_journal_kernels.h"

namespace {
std::string g_err;
constexpr uint32_t kEmuWindowWords = 3;
constexpr uint32_t kEmuTile = 3;
}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_journal_error says why)
// slice_entries, chunk: 0 = the library's own
extern "C" int emu_journal_check(const tbc_ledger_rt_in* in, tbc_ledger_journal_out* out, uint32_t grid_cap, uint64_t seed, uint32_t slice_entries, uint32_t chunk) {
  g_err.clear();
  if (!lgjn::validate("emu_journal_check", in, g_err)) return TBC_ERR_INVALID_ARG;
  lgjn::Plan P;
  if (!lgjn::plan("emu_journal_check", in, P, g_err, slice_entries ? slice_entries : lgjn::kJnSliceEntries, chunk ? chunk : lgjn::kJnChunk, chunk ? kEmuTile : lgjn::kJnTile)) return TBC_ERR_INVALID_ARG;
  struct Run { emu::Launcher go; void sequence(const lgjn::JnArgs& A) { lgjn::sequence<kEmuWindowWords>(go, A); } };
  emu::Arena C(g_err);
  C.open(in->ledger.device, P.arena.bytes);
  lgjn::steps("emu_journal_check", C, Run{emu::Launcher(grid_cap, seed)}, in, P, out);
  return C.close();
}

extern "C" const char* emu_journal_error() { return g_err.c_str(); }
// the plan's shape: transfer micro-ops, words, entries, lookups, slices, slice entries, chunk, reads, read micro-ops, image bytes, head bytes
extern "C" int emu_journal_shape(const tbc_ledger_rt_in* in, uint32_t slice_entries, uint32_t chunk, uint64_t* out11) {
  lgjn::Plan P;
  if (!lgjn::validate("emu_journal_shape", in, g_err) || !lgjn::plan("emu_journal_shape", in, P, g_err, slice_entries ? slice_entries : lgjn::kJnSliceEntries, chunk ? chunk : lgjn::kJnChunk)) return 1;
  out11[0] = P.xf.n_mops; out11[1] = P.n_words; out11[2] = P.lk.n_mops; out11[3] = P.n_lookups; out11[4] = P.n_slices; out11[5] = P.slice_entries; out11[6] = P.chunk;
  out11[7] = P.n_reads; out11[8] = P.rd.n_mops; out11[9] = P.arena.image_bytes(); out11[10] = P.arena.head_bytes();
  return 0;
}
