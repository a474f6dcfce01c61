// perf_host.hip -- tbc_perf_series and tbc_perf_plan_sizes, the entry points of the perf series (include/tbcheck.h), the former over the
// call frame of oneshot_call.h: every rule of the input on the host, the plan (perf_plan.h), the zeroed head, the plan's partner column
// and the caller's columns straight to their regions, the kernels (perf.hip), and the results back in one copy per array the caller
// asked for.
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
  const pf::PfArena& L = P.arena;
  OneShotCall C;
  if (C.open(in->device, L.bytes) != TBC_OK) return C.status;
  C.fill(L.acc, 0, L.zero_bytes());
  C.put(L.partner, P.partner.data());
  C.put(L.time, in->time); C.put(L.process, in->process); C.put(L.type, in->type); C.put(L.f, in->f);
  C.timed([&] { pf::launch(C.stream, pf::args(P, C.base())); });
  C.get(out->op_latency, L.op_latency); C.get(out->op_outcome, L.op_outcome); C.get(out->op_open_after, L.op_open_after);
  C.get(out->q_count, L.q_count); C.get(out->q_value, L.q_value); C.get(out->rate_count, L.rate_count);
  C.get(out->open_last, L.open_last); C.get(out->open_fill, L.open_fill);
  C.get(&out->summary, L.summary);
  if (C.sync() != TBC_OK) return C.status;
  out->summary.ns_device = C.ns_device();
  out->summary.bytes_in = C.bytes_in;
  return TBC_OK;
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
