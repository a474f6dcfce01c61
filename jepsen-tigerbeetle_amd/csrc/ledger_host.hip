// ledger_host.hip -- tbc_ledger_check, the entry point of the ledger workload's checkers (include/tbcheck.h), over the call frame of
// oneshot_call.h: every rule of the input on the host, the plan, the frame, and the steps of the call as lg::steps states them
// (ledger_plan.h), the kernels those of ledger.hip on the frame's stream.
#include <string>
#include "oneshot_call.h"
#include "ledger_plan.h"

using namespace tbc;

namespace {

tbc_status lg_check(const char* fn, const tbc_ledger_in* in, tbc_ledger_out* out) {
  std::string err;
  lg::Plan P;
  if (!lg::validate(fn, in, err) || !lg::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  struct Run { void* stream; void sequence(const lg::LgArgs& A, unsigned long long fr_mops, unsigned long long fl_mops) { lg::launch(stream, A, fr_mops, fl_mops); } };
  OneShotCall C;
  if (C.open(in->device, P.arena.bytes) != TBC_OK) return C.status;
  return lg::steps(C, Run{C.stream}, in, P, out);
}

}  // namespace

extern "C" tbc_status tbc_ledger_check(const tbc_ledger_in* in, tbc_ledger_out* out) { return oneshot_entry("tbc_ledger_check", in, out, lg_check); }
