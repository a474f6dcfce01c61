// ledger_snap_host.hip -- tbc_ledger_snapshots, the entry point of the snapshot order of a ledger's reads (include/tbcheck.h), over the
// call frame of oneshot_call.h: every rule of the input on the host, the plan, the frame, and the steps of the call as lgsn::steps
// states them (ledger_snap_plan.h), the two runs of kernels those of ledger_snap.hip on the frame's stream.
#include <string>
#include "oneshot_call.h"
#include "ledger_snap_plan.h"

using namespace tbc;

namespace {

tbc_status snap_check(const char* fn, const tbc_ledger_in* in, tbc_ledger_snap_out* out) {
  std::string err;
  lgsn::Plan P;
  if (!lgsn::validate(fn, in, err) || !lgsn::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  struct Run {
    void* stream;
    void filter(const lgsn::SnArgs& A) { lgsn::launch_filter(stream, A); }
    void rest(const lgsn::SnArgs& A, uint32_t n_candidates) { lgsn::launch_rest(stream, A, n_candidates); }
  };
  OneShotCall C;
  if (C.open(in->device, P.arena.bytes) != TBC_OK) return C.status;
  return lgsn::steps(fn, C, Run{C.stream}, in, P, out);
}

}  // namespace

extern "C" tbc_status tbc_ledger_snapshots(const tbc_ledger_in* in, tbc_ledger_snap_out* out) { return oneshot_entry("tbc_ledger_snapshots", in, out, snap_check); }
