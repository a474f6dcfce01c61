// ledger_rt_host.hip -- tbc_ledger_realtime, the entry point of the realtime bounds on the ledger's posted counters (include/tbcheck.h),
// over the call frame of oneshot_call.h: every rule of the input on the host, the plan, the frame, and the steps of the call as
// lgrt::steps states them (ledger_rt_plan.h), the kernels those of ledger_rt.hip on the frame's stream.
#include <string>
#include "oneshot_call.h"
#include "ledger_rt_plan.h"

using namespace tbc;

namespace {

tbc_status rt_check(const char* fn, const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out) {
  std::string err;
  lgrt::Plan P;
  if (!lgrt::validate(fn, in, err) || !lgrt::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  struct Run { void* stream; void sequence(const lgrt::RtArgs& A) { lgrt::launch(stream, A); } };
  OneShotCall C;
  if (C.open(in->ledger.device, P.arena.bytes) != TBC_OK) return C.status;
  return lgrt::steps(fn, C, Run{C.stream}, in, P, out);
}

}  // namespace

extern "C" tbc_status tbc_ledger_realtime(const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out) { return oneshot_entry("tbc_ledger_realtime", in, out, rt_check); }
