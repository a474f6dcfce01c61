// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger.cpp: tbc_ledger_check on the CPU -- the validation and the host plan of
// csrc/ledger_plan.h, the arena laid out and filled in the steps of csrc/ledger_host.hip (the head image, the caller's columns, the
// zeroed regions), and the kernels of csrc/ledger_kernels.h (the very file hipcc compiles into libtbcheck.so) under the wavefront /
// workgroup emulator, launched by lg::sequence of that file -- the library's own statement -- over the emulator's launcher
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
  const lg::LgArena& L = P.arena;
  emu::Arena C(L.bytes);
  C.image(lg::head_image(P));
  C.put(L.mop_id, in->mop_id); C.put(L.mop_a, in->mop_a); C.put(L.mop_b, in->mop_b); C.put(L.mop_c, in->mop_c); C.put(L.mop_flags, in->mop_flags);
  C.fill(L.slots, 0, L.zero_bytes());
  emu::Launcher go(grid_cap, seed);
  lg::sequence<EMU_W>(go, lg::args(in, P, C.base()), P.fr_cum.back(), P.fl_cum.back());
  // every transfer id sits in the table exactly once
  {
    const SfEncSlot* tab = (const SfEncSlot*)C.at(L.slots);
    uint64_t used = 0;
    for (uint64_t s = 0; s < P.tab_slots; s++) used += tab[s].col1 != 0u;
    if (used != P.n_transfers) { g_err = "the table does not hold every transfer id once"; return 1; }
  }
  const size_t R = P.n_reads, FR = P.n_final_reads, FL = P.n_final_lookups;
  C.get(out->read_error, L.read_error, R); C.get(out->read_total, L.read_total, R * 8); C.get(out->read_badness, L.read_badness, R * 8);
  C.get(out->lookup_missing, L.missing, FL * 4); C.get(out->final_read_unlike, L.fr_unlike, FR); C.get(out->final_lookup_unlike, L.fl_unlike, FL);
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_summary));
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
