// ledger_rt_host.hip -- tbc_ledger_realtime, the entry point of the realtime bounds on the ledger's posted counters (include/tbcheck.h),
// over the call frame of oneshot_call.h: every rule of the input on the host, the plan (ledger_rt_plan.h), the head and the micro-op
// columns of the ops the kernels look at as one image in one copy, the kernels (ledger_rt.hip), the summary back -- an amount out of
// range, which only the device has looked at, ends the call there -- and then one copy per array the caller asked for.
#include <string>
#include <vector>
#include "oneshot_call.h"
#include "ledger_rt_plan.h"

using namespace tbc;

namespace {

tbc_status rt_check(const char* fn, const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out) {
  std::string err;
  lgrt::Plan P;
  if (!lgrt::validate(fn, in, err) || !lgrt::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  const lgrt::RtArena& L = P.arena;
  const std::vector<unsigned char> img = lgrt::image(in, P);
  OneShotCall C;
  if (C.open(in->ledger.device, L.bytes) != TBC_OK) return C.status;
  C.image(img);
  C.fill(L.carry_cnt[0], 0, L.zero_bytes());
  C.timed([&] { lgrt::launch(C.stream, lgrt::args(in, P, C.base())); });
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_rt_summary));
  if (C.sync() != TBC_OK) return C.status;
  out->summary.ns_device = C.ns_device();
  out->summary.bytes_in = C.bytes_in;
  if (out->summary.bad_amounts) {
    set_error("%s: %u transfer amounts are outside [0, 2^31)", fn, out->summary.bad_amounts);
    return TBC_ERR_UNSUPPORTED;
  }
  const size_t R = P.n_reads, Mr = (size_t)P.rows[lgrt::kReads].mops();
  C.get(out->rt_bits, L.rt_bits, R); C.get(out->rt_miss, L.rt_miss, R * 24);
  C.get(out->mop_lo, L.mop_lo, Mr * 16); C.get(out->mop_hi, L.mop_hi, Mr * 16); C.get(out->mop_floor, L.mop_floor, Mr * 16);
  return C.sync();
}

}  // namespace

extern "C" tbc_status tbc_ledger_realtime(const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out) { return oneshot_entry("tbc_ledger_realtime", in, out, rt_check); }
