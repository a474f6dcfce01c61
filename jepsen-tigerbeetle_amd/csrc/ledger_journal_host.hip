// ledger_journal_host.hip -- tbc_ledger_journal, the entry point of the journal audit of a ledger's lookups (include/tbcheck.h), over
// the call frame of oneshot_call.h: every rule of the input on the host, the plan, the frame, and the steps of the call as lgjn::steps
// states them (ledger_journal_plan.h), the kernels those of ledger_journal.hip on the frame's stream.
#include <string>
#include "oneshot_call.h"
#include "ledger_journal_plan.h"

using namespace tbc;

namespace {

tbc_status journal_check(const char* fn, const tbc_ledger_rt_in* in, tbc_ledger_journal_out* out) {
  std::string err;
  lgjn::Plan P;
  if (!lgjn::validate(fn, in, err) || !lgjn::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  struct Run { void* stream; void sequence(const lgjn::JnArgs& A) { lgjn::launch(stream, A); } };
  OneShotCall C;
  if (C.open(in->ledger.device, P.arena.bytes) != TBC_OK) return C.status;
  return lgjn::steps(fn, C, Run{C.stream}, in, P, out);
}

}  // namespace

extern "C" tbc_status tbc_ledger_journal(const tbc_ledger_rt_in* in, tbc_ledger_journal_out* out) { return oneshot_entry("tbc_ledger_journal", in, out, journal_check); }
