// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_ledger_journal.cpp: tbc_ledger_journal on the CPU -- the validation and the host plan of
// csrc/ledger_journal_plan.h, the arena laid out and filled in the steps of csrc/ledger_journal_host.hip (the one image of the head and
// the gathered columns, the zeroed regions), and the kernels of csrc/ledger_journal_kernels.h (the very file hipcc compiles into
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
  const lgjn::JnArena& L = P.arena;
  emu::Arena C(L.bytes);
  const std::vector<unsigned char> img = lgjn::image(in, P);
  C.image(img);
  C.fill(L.slots, 0, L.zero_bytes());
  const lgjn::JnArgs A = lgjn::args(in, P, C.base());
  emu::Launcher go(grid_cap, seed);
  lgjn::sequence<kEmuWindowWords>(go, A);
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_journal_summary));
  out->summary.ns_device = 0; out->summary.bytes_in = img.size();
  if (out->summary.bad_amounts) { g_err = "emu_journal_check: amounts of journalled transfers are outside [0, 2^31)"; return TBC_ERR_UNSUPPORTED; }
  const size_t M = (size_t)P.xf.n_mops, R = P.n_reads;
  C.get(out->entry_bits, L.entry_bits); C.get(out->lk_counts, L.lk_counts); C.get(out->lk_present, L.lk_present); C.get(out->lk_vector, L.lk_vector);
  C.get(out->rd_bits, L.rd_bits, R); C.get(out->rd_first, L.rd_first, R * 8);
  C.get(out->xfer_present, L.xfer_present, M * 4); C.get(out->xfer_early, L.xfer_early, M * 4); C.get(out->xfer_lost, L.xfer_lost, M * 4);
  C.get(out->xfer_vanished, L.xfer_vanished, M * 4); C.get(out->xfer_flags, L.xfer_flags, M);
  return 0;
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
