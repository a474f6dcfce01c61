// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger_cycles.cpp: tbc_ledger_cycles on the CPU -- the validation and the host plan of
// csrc/ledger_cycles_plan.h, the arena laid out and filled in the steps of csrc/ledger_cycles_host.hip (the snapshot plan's image, this
// checker's head, the zeroed region; the two matrices made once the core is counted), and the kernels of csrc/ledger_cycles_kernels.h
// (the very file hipcc compiles into libtbcheck.so, the snapshot filter's kernels with it) under the wavefront / workgroup emulator,
// launched by the four sequences of that file -- the library's own statement -- over the emulator's launcher (oneshot_emu.h), the
// core's size and the changed flag of every round read in between as the host does.  Every grid that strides is capped at `grid_cap`
// workgroups, so that the strides run; `sort_chunks_cap` and `scan_rows` are the snapshot plan's knobs; `max_core` (0: the library's
// TBC_LEDGER_CYCLES_MAX_CORE) lets a small history meet the cap.  Built as a shared object by tests/test_ledger_cycles_emu.py, which
// compares what comes back with cycles_numpy of jepsen/ledger.py.
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
  const lgsn::SnArena& S = P.sn.arena;
  const lgcy::CyArena& L = P.arena;
  emu::Arena C(L.bytes);
  const std::vector<unsigned char> img = lgsn::image(&in->ledger, P.sn), head = lgcy::head_image(P);
  C.image(img);
  C.put(oneshot::Region{L.head_at(), L.head_bytes()}, head.data());
  C.fill(S.val, 0, S.zero_bytes());
  lgcy::CyArgs A = lgcy::args(in, P, C.base());
  emu::Launcher go(grid_cap, seed);
  lgcy::prepare_sequence(go, A);
  tbc_ledger_cycles_summary& s = out->summary;
  s = tbc_ledger_cycles_summary{};
  s.read_count = P.sn.n_reads; s.n_partial = A.sn.acc->n_partial; s.n_core = A.acc->n_core; s.bad_values = A.sn.acc->bad_values; s.n_checked = A.sn.acc->n_checked;
  s.first = s.largest = lgcy::kCyNone;
  s.bytes_in = img.size() + head.size();
  if (s.bad_values) { g_err = "emu_cycles_check: reads hold counters whose magnitudes add up to 2^63 or more"; return TBC_ERR_UNSUPPORTED; }
  if (s.n_core > (max_core ? max_core : TBC_LEDGER_CYCLES_MAX_CORE)) { g_err = "emu_cycles_check: the core is above the cap"; return TBC_ERR_UNSUPPORTED; }
  // the core is listed ascending, and it is the reads whose state says so
  for (uint32_t i = 0; i < s.n_core; i++) {
    const uint32_t r = A.core_list[i];
    if (r >= A.n_reads || !(A.state[r] & TBC_LEDGER_CYC_CORE) || A.core_pos[r] != i || (i && A.core_list[i - 1] >= r)) { g_err = "the core's list is not the core reads ascending"; return -1; }
  }
  uint32_t rounds = 0, final_side = 0;
  std::vector<unsigned char> matrices(2 * lgcy::matrix_bytes(s.n_core) + 256, 0xA5);
  if (s.n_core) {
    A = lgcy::with_matrix(A, s.n_core, reinterpret_cast<char*>(matrices.data()));
    lgcy::describe_sequence(go, A);
    for (;;) {
      lgcy::round_sequence(go, A, rounds);
      final_side = (rounds & 1u) ^ 1u;
      if (!A.acc->changed[rounds++]) break;
      if (rounds == lgcy::kCyMaxRounds) { g_err = "the closure did not settle"; return -1; }
    }
  }
  lgcy::finish_sequence(go, A, final_side, rounds);
  for (size_t k = 2 * lgcy::matrix_bytes(s.n_core); k < matrices.size(); k++)
    if (matrices[k] != 0xA5) { g_err = "a kernel wrote past the matrices"; return -1; }
  for (const emu::Recorder::Launch& l : go.ran.launches) {
    g_launches[0] += l.kernel == emu::Recorder::of(cy_closure_kernel);
    g_launches[1] += l.kernel == emu::Recorder::of(cy_matrix_kernel);
    g_launches[2] += l.kernel == emu::Recorder::of(cy_member_kernel);
    g_launches[3]++;
  }
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_cycles_summary));
  out->summary.ns_device = 0; out->summary.bytes_in = img.size() + head.size();
  const size_t R = P.sn.n_reads;
  C.get(out->scc, L.scc, R * 4); C.get(out->cyc_flags, L.cyc_flags, R);
  return 0;
}

extern "C" const char* emu_cycles_error() { return g_err.c_str(); }
// of the last call: how many closure, matrix and member kernels it launched, and how many kernels in all
extern "C" uint64_t emu_cycles_launches(uint32_t which) { return which < 4 ? g_launches[which] : 0; }
