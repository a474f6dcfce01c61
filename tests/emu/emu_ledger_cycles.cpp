// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger_cycles.cpp: tbc_ledger_cycles on the CPU -- the validation and the host plan of
// csrc/ledger_cycles_plan.h, the steps of the call as lgcy::steps of that header states them -- the list csrc/ledger_cycles_host.hip
// runs: the core's size and the changed flag of every round read in between, the two matrices made once the core is counted -- over
// the emulator's call frame, and the kernels of csrc/ledger_cycles_kernels.h (the very file hipcc compiles into libtbcheck.so, the
// snapshot filter's kernels with it) under the wavefront / workgroup emulator, launched by the four sequences of that file -- the
// library's own statement -- over the emulator's launcher (oneshot_emu.h).  Every grid that strides is capped at `grid_cap`
// workgroups, so that the strides run; `sort_chunks_cap` and `scan_rows` are the snapshot plan's knobs; `max_core` (0: the library's
// TBC_LEDGER_CYCLES_MAX_CORE) is the step list's, and lets a small history meet the cap.  Built as a shared object by
// tests/test_ledger_cycles_emu.py, which compares what comes back with cycles_numpy of jepsen/ledger.py.
#include "oneshot_emu.h"
#include "ledger_cycles_plan.h"
#include "ledger_cycles_kernels.h"

namespace {
std::string g_err;
uint64_t g_launches[4];                  // of the last call: closure kernels, matrix kernels, member kernels, all kernels
}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_cycles_error says why)
extern "C" int emu_cycles_check(const tbc_ledger_rt_in* in, tbc_ledger_cycles_out* out, uint32_t grid_cap, uint64_t seed, uint32_t sort_chunks_cap, uint32_t scan_rows,
                                uint32_t max_core) {
  g_err.clear();
  for (uint64_t& n : g_launches) n = 0;
  if (!lgcy::validate("emu_cycles_check", in, g_err)) return TBC_ERR_INVALID_ARG;
  lgcy::Plan P;
  if (!lgcy::plan("emu_cycles_check", in, P, g_err, sort_chunks_cap ? sort_chunks_cap : lgsn::kSnSortChunksMax, scan_rows ? scan_rows : lgsn::kSnScanRows)) return TBC_ERR_INVALID_ARG;
  struct Run {
    emu::Launcher go;
    bool core_listed = true;
    void prepare(const lgcy::CyArgs& A) { lgcy::prepare_sequence(go, A); }
    // (before it: the core is listed ascending, and it is the reads whose state says so; if not, nothing more is launched)
    void describe(const lgcy::CyArgs& A) {
      for (uint32_t i = 0; i < A.n_core; i++) {
        const uint32_t r = A.core_list[i];
        core_listed = core_listed && r < A.n_reads && (A.state[r] & TBC_LEDGER_CYC_CORE) && A.core_pos[r] == i && !(i && A.core_list[i - 1] >= r);
      }
      if (core_listed) lgcy::describe_sequence(go, A);
    }
    void round(const lgcy::CyArgs& A, uint32_t round) { if (core_listed) lgcy::round_sequence(go, A, round); }
    void finish(const lgcy::CyArgs& A, uint32_t final_side, uint32_t rounds) { if (core_listed) lgcy::finish_sequence(go, A, final_side, rounds); }
  } run{emu::Launcher(grid_cap, seed)};
  emu::Arena C(g_err);
  C.open(in->ledger.device, P.arena.bytes);
  lgcy::steps("emu_cycles_check", C, run, in, P, out, max_core ? max_core : TBC_LEDGER_CYCLES_MAX_CORE);
  if (!run.core_listed) { g_err = "the core's list is not the core reads ascending"; return -1; }
  for (const emu::Recorder::Launch& l : run.go.ran.launches) {
    g_launches[0] += l.kernel == emu::Recorder::of(cy_closure_kernel);
    g_launches[1] += l.kernel == emu::Recorder::of(cy_matrix_kernel);
    g_launches[2] += l.kernel == emu::Recorder::of(cy_member_kernel);
    g_launches[3]++;
  }
  return C.close();
}

extern "C" const char* emu_cycles_error() { return g_err.c_str(); }
// of the last call: how many closure, matrix and member kernels it launched, and how many kernels in all
extern "C" uint64_t emu_cycles_launches(uint32_t which) { return which < 4 ? g_launches[which] : 0; }
