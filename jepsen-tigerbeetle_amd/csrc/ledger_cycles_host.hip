// ledger_cycles_host.hip -- tbc_ledger_cycles, the entry point of the cycle search over a ledger's reads (include/tbcheck.h), over the
// call frame of oneshot_call.h: every rule of the input on the host, the plan, the frame, and the steps of the call as lgcy::steps
// states them (ledger_cycles_plan.h), the four runs of kernels those of ledger_cycles.hip on the frame's stream.
#include <string>
#include "oneshot_call.h"
#include "ledger_cycles_plan.h"

using namespace tbc;

namespace {

tbc_status cycles_check(const char* fn, const tbc_ledger_rt_in* in, tbc_ledger_cycles_out* out) {
  std::string err;
  lgcy::Plan P;
  if (!lgcy::validate(fn, in, err) || !lgcy::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  struct Run {
    void* stream;
    void prepare(const lgcy::CyArgs& A) { lgcy::launch_prepare(stream, A); }
    void describe(const lgcy::CyArgs& A) { lgcy::launch_describe(stream, A); }
    void round(const lgcy::CyArgs& A, uint32_t round) { lgcy::launch_round(stream, A, round); }
    void finish(const lgcy::CyArgs& A, uint32_t final_side, uint32_t rounds) { lgcy::launch_finish(stream, A, final_side, rounds); }
  };
  OneShotCall C;
  if (C.open(in->ledger.device, P.arena.bytes) != TBC_OK) return C.status;
  return lgcy::steps(fn, C, Run{C.stream}, in, P, out);
}

}  // namespace

extern "C" tbc_status tbc_ledger_cycles(const tbc_ledger_rt_in* in, tbc_ledger_cycles_out* out) { return oneshot_entry("tbc_ledger_cycles", in, out, cycles_check); }
