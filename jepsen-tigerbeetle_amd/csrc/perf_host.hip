// perf_host.hip -- tbc_perf_series and tbc_perf_plan_sizes, the entry points of the perf series (include/tbcheck.h), the former over the
// call frame of oneshot_call.h: every rule of the input on the host, the plan, the frame, and the steps of the call as pf::steps states
// them (perf_plan.h), the kernels those of perf.hip on the frame's stream.
#include <string>
#include "oneshot_call.h"
#include "perf_plan.h"

using namespace tbc;

namespace {

tbc_status pf_series(const char* fn, const tbc_perf_in* in, tbc_perf_out* out) {
  std::string err;
  pf::Plan P;
  tbc_status st = pf::validate(fn, in, err);
  if (st == TBC_OK) st = pf::plan(fn, in, P, err);
  if (st != TBC_OK) { set_error("%s", err.c_str()); return st; }
  struct Run { void* stream; void sequence(const pf::PfArgs& A) { pf::launch(stream, A); } };
  OneShotCall C;
  if (C.open(in->device, P.arena.bytes) != TBC_OK) return C.status;
  return pf::steps(C, Run{C.stream}, in, P, out);
}

}  // namespace

extern "C" tbc_status tbc_perf_plan_sizes(const tbc_perf_in* in, tbc_perf_sizes* sizes) {
  const char* fn = "tbc_perf_plan_sizes";
  if (!in || !sizes) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  std::string err;
  tbc_status st = pf::validate(fn, in, err);
  if (st == TBC_OK) st = pf::sizes(fn, in, *sizes, err);
  if (st != TBC_OK) set_error("%s", err.c_str());
  return st;
}

extern "C" tbc_status tbc_perf_series(const tbc_perf_in* in, tbc_perf_out* out) { return oneshot_entry("tbc_perf_series", in, out, pf_series); }
