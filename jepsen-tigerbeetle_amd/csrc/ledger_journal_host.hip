// ledger_journal_host.hip -- tbc_ledger_journal, the entry point of the journal audit of a ledger's lookups (include/tbcheck.h), over
// the call frame of oneshot_call.h: every rule of the input on the host, the plan (ledger_journal_plan.h), the head and the three groups
// of micro-op columns as one image in one copy, the kernels (ledger_journal.hip), the summary back -- an amount out of range, which only
// the device has looked at, ends the call there -- and then one copy per array the caller asked for.
#include <string>
#include <vector>
#include "oneshot_call.h"
#include "ledger_journal_plan.h"

using namespace tbc;

namespace {

tbc_status journal_check(const char* fn, const tbc_ledger_rt_in* in, tbc_ledger_journal_out* out) {
  std::string err;
  lgjn::Plan P;
  if (!lgjn::validate(fn, in, err) || !lgjn::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  const lgjn::JnArena& L = P.arena;
  const std::vector<unsigned char> img = lgjn::image(in, P);
  OneShotCall C;
  if (C.open(in->ledger.device, L.bytes) != TBC_OK) return C.status;
  C.image(img);
  C.fill(L.slots, 0, L.zero_bytes());
  C.timed([&] { lgjn::launch(C.stream, lgjn::args(in, P, C.base())); });
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_journal_summary));
  if (C.sync() != TBC_OK) return C.status;
  out->summary.ns_device = C.ns_device();
  out->summary.bytes_in = C.bytes_in;
  if (out->summary.bad_amounts) {
    set_error("%s: %u amounts of journalled transfers are outside [0, 2^31)", fn, out->summary.bad_amounts);
    return TBC_ERR_UNSUPPORTED;
  }
  const size_t M = (size_t)P.xf.n_mops, R = P.n_reads;
  C.get(out->entry_bits, L.entry_bits); C.get(out->lk_counts, L.lk_counts); C.get(out->lk_present, L.lk_present); C.get(out->lk_vector, L.lk_vector);
  C.get(out->rd_bits, L.rd_bits, R); C.get(out->rd_first, L.rd_first, R * 8);
  C.get(out->xfer_present, L.xfer_present, M * 4); C.get(out->xfer_early, L.xfer_early, M * 4); C.get(out->xfer_lost, L.xfer_lost, M * 4);
  C.get(out->xfer_vanished, L.xfer_vanished, M * 4); C.get(out->xfer_flags, L.xfer_flags, M);
  return C.sync();
}

}  // namespace

extern "C" tbc_status tbc_ledger_journal(const tbc_ledger_rt_in* in, tbc_ledger_journal_out* out) { return oneshot_entry("tbc_ledger_journal", in, out, journal_check); }
