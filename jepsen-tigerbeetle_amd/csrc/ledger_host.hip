// ledger_host.hip -- tbc_ledger_check, the entry point of the ledger workload's checkers (include/tbcheck.h), over the call frame of
// oneshot_call.h: every rule of the input on the host, the plan (ledger_plan.h), the head as one image and the caller's micro-op columns
// straight to their regions, the kernels (ledger.hip), and the results back in one copy per array the caller asked for.
#include <string>
#include <vector>
#include "oneshot_call.h"
#include "ledger_plan.h"

using namespace tbc;

namespace {

tbc_status lg_check(const char* fn, const tbc_ledger_in* in, tbc_ledger_out* out) {
  std::string err;
  lg::Plan P;
  if (!lg::validate(fn, in, err) || !lg::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  const lg::LgArena& L = P.arena;
  const std::vector<unsigned char> img = lg::head_image(P);
  OneShotCall C;
  if (C.open(in->device, L.bytes) != TBC_OK) return C.status;
  C.image(img);
  C.put(L.mop_id, in->mop_id); C.put(L.mop_a, in->mop_a); C.put(L.mop_b, in->mop_b); C.put(L.mop_c, in->mop_c); C.put(L.mop_flags, in->mop_flags);
  C.fill(L.slots, 0, L.zero_bytes());
  C.timed([&] { lg::launch(C.stream, lg::args(in, P, C.base()), P.fr_cum.back(), P.fl_cum.back()); });
  const size_t R = P.n_reads, FR = P.n_final_reads, FL = P.n_final_lookups;
  C.get(out->read_error, L.read_error, R); C.get(out->read_total, L.read_total, R * 8); C.get(out->read_badness, L.read_badness, R * 8);
  C.get(out->lookup_missing, L.missing, FL * 4);
  C.get(out->final_read_unlike, L.fr_unlike, FR); C.get(out->final_lookup_unlike, L.fl_unlike, FL);
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_summary));
  if (C.sync() != TBC_OK) return C.status;
  out->summary.ns_device = C.ns_device();
  out->summary.bytes_in = C.bytes_in;
  return TBC_OK;
}

}  // namespace

extern "C" tbc_status tbc_ledger_check(const tbc_ledger_in* in, tbc_ledger_out* out) { return oneshot_entry("tbc_ledger_check", in, out, lg_check); }
