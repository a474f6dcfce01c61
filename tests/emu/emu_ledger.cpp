// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger.cpp: tbc_ledger_check on the CPU -- the validation and the host plan of
// csrc/ledger_plan.h, the steps of the call as lg::steps of that header states them -- the list csrc/ledger_host.hip runs -- over the
// emulator's call frame, and the kernels of csrc/ledger_kernels.h (the very file hipcc compiles into libtbcheck.so) under the
// wavefront / workgroup emulator, launched by lg::sequence of that file -- the library's own statement -- over the emulator's launcher
// (oneshot_emu.h).  The lookup kernel's window is EMU_W words here (the library's is TBC_LEDGER_LOOKUP_WINDOW_WORDS), so that a few
// hundred transfers span several windows; every grid that strides is capped at `grid_cap` workgroups, so that the strides run.
// Built as a shared object by tests/test_ledger_emu.py, which compares what comes back with the host statement of jepsen/ledger.py.
#include "oneshot_emu.h"
#include "ledger_plan.h"
#include "ledger_kernels.h"

#ifndef EMU_W
#define EMU_W 8u
#endif

namespace {
std::string g_err;
}  // namespace

// 0: checked; 1: refused (emu_lg_error says why)
extern "C" int emu_lg_check(const tbc_ledger_in* in, tbc_ledger_out* out, uint32_t grid_cap, uint64_t seed) {
  g_err.clear();
  if (!lg::validate("emu_lg_check", in, g_err)) return 1;
  lg::Plan P;
  if (!lg::plan("emu_lg_check", in, P, g_err)) return 1;
  struct Run { emu::Launcher go; void sequence(const lg::LgArgs& A, unsigned long long fr_mops, unsigned long long fl_mops) { lg::sequence<EMU_W>(go, A, fr_mops, fl_mops); } };
  emu::Arena C(g_err);
  C.open(in->device, P.arena.bytes);
  lg::steps(C, Run{emu::Launcher(grid_cap, seed)}, in, P, out);
  if (C.close() != TBC_OK) return C.status;
  // every transfer id sits in the table exactly once
  const SfEncSlot* tab = (const SfEncSlot*)C.at(P.arena.slots);
  uint64_t used = 0;
  for (uint64_t s = 0; s < P.tab_slots; s++) used += tab[s].col1 != 0u;
  if (used != P.n_transfers) { g_err = "the table does not hold every transfer id once"; return 1; }
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
