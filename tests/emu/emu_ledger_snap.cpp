// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger_snap.cpp: tbc_ledger_snapshots on the CPU -- the validation and the host plan of
// csrc/ledger_snap_plan.h, the steps of the call as lgsn::steps of that header states them -- the list csrc/ledger_snap_host.hip runs,
// the candidates' number read between the two runs of kernels -- over the emulator's call frame, and the kernels of
// csrc/ledger_snap_kernels.h (the very file hipcc compiles into libtbcheck.so) under the wavefront / workgroup emulator, launched by
// lgsn::filter_sequence and lgsn::rest_sequence of that file -- the library's own statement -- over the emulator's launcher
// (oneshot_emu.h).  Every grid that strides is capped at `grid_cap` workgroups, so that the strides run (the pair kernel: as many slices of tiles
// at most); `sort_chunks_cap` and `scan_rows` are the plan's: a few chunks make a sort chunk several wavefronts' worth, a few rows a
// chunk give the scan's carry several steps.  Built as a shared object by tests/test_ledger_snapshots_emu.py, which compares what comes
// back with snapshots_numpy of jepsen/ledger.py.
#include "oneshot_emu.h"
#include "ledger_snap_plan.h"
#include "ledger_snap_kernels.h"

namespace {
std::string g_err;
uint64_t g_pair_launches;
}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_snap_error says why)
// sort_chunks_cap, scan_rows: 0 = the library's own
extern "C" int emu_snap_check(const tbc_ledger_in* in, tbc_ledger_snap_out* out, uint32_t grid_cap, uint64_t seed, uint32_t sort_chunks_cap, uint32_t scan_rows) {
  g_err.clear();
  g_pair_launches = 0;
  if (!lgsn::validate("emu_snap_check", in, g_err)) return TBC_ERR_INVALID_ARG;
  lgsn::Plan P;
  if (!lgsn::plan("emu_snap_check", in, P, g_err, sort_chunks_cap ? sort_chunks_cap : lgsn::kSnSortChunksMax, scan_rows ? scan_rows : lgsn::kSnScanRows)) return TBC_ERR_INVALID_ARG;
  struct Run {
    emu::Launcher go;
    void filter(const lgsn::SnArgs& A) { lgsn::filter_sequence(go, A); }
    void rest(const lgsn::SnArgs& A, uint32_t n_candidates) { lgsn::rest_sequence(go, A, n_candidates); }
  } run{emu::Launcher(grid_cap, seed)};
  emu::Arena C(g_err);
  C.open(in->device, P.arena.bytes);
  lgsn::steps("emu_snap_check", C, run, in, P, out);
  if (C.close() != TBC_OK && C.status != TBC_ERR_UNSUPPORTED) return C.status;
  for (const emu::Recorder::Launch& l : run.go.ran.launches) g_pair_launches += l.kernel == emu::Recorder::of(sn_pair_kernel);
  // the order is sorted by (key, read number), and it is a permutation (nothing after the sort writes the order)
  const lgsn::SnArgs A = lgsn::args(in, P, C.base());
  if (A.n_reads && A.n_class) {
    std::vector<uint8_t> seen(A.n_reads, 0);
    for (uint32_t p = 0; p < A.n_reads; p++) {
      const uint32_t r = A.sort_perm[0][p];
      if (r >= A.n_reads || seen[r]) { g_err = "the sorted order is no permutation of the reads"; return -1; }
      seen[r] = 1;
      if (p && (A.sort_key[0][p - 1] > A.sort_key[0][p] || (A.sort_key[0][p - 1] == A.sort_key[0][p] && A.sort_perm[0][p - 1] > r))) { g_err = "the reads are not in the order of (sum, read number)"; return -1; }
    }
  }
  return C.status;
}

extern "C" const char* emu_snap_error() { return g_err.c_str(); }
// how many pair kernels the last call launched (0 or 1)
extern "C" uint64_t emu_snap_pair_launches() { return g_pair_launches; }
// the plan's shape: reads, classes, micro-ops, sort chunks, sort chunk entries, scan rows, scan chunks, image bytes
extern "C" int emu_snap_shape(const tbc_ledger_in* in, uint64_t* out8) {
  lgsn::Plan P;
  if (!lgsn::validate("emu_snap_shape", in, g_err) || !lgsn::plan("emu_snap_shape", in, P, g_err)) return 1;
  out8[0] = P.n_reads; out8[1] = P.n_class; out8[2] = P.n_mops; out8[3] = P.sort_chunks; out8[4] = P.sort_chunk_entries; out8[5] = P.scan_rows; out8[6] = P.scan_chunks;
  out8[7] = P.arena.image_bytes();
  return 0;
}
