// ledger_snap_host.hip -- tbc_ledger_snapshots, the entry point of the snapshot order of a ledger's reads (include/tbcheck.h), over the
// call frame of oneshot_call.h: every rule of the input on the host, the plan (ledger_snap_plan.h), the head and the reads' micro-op
// columns as one image in one copy, the filter's kernels (ledger_snap.hip), the accumulators back -- the number of candidates decides
// whether a pair kernel is launched at all --, the rest of the kernels, the summary back -- a read out of range, which only the device
// has looked at, ends the call there -- and then one copy per array the caller asked for.  The two runs of kernels are timed sections of
// their own; ns_device is their sum.
#include <string>
#include <vector>
#include "oneshot_call.h"
#include "ledger_snap_plan.h"

using namespace tbc;

namespace {

tbc_status snap_check(const char* fn, const tbc_ledger_in* in, tbc_ledger_snap_out* out) {
  std::string err;
  lgsn::Plan P;
  if (!lgsn::validate(fn, in, err) || !lgsn::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  const lgsn::SnArena& L = P.arena;
  const std::vector<unsigned char> img = lgsn::image(in, P);
  lgsn::SnAcc acc{};
  OneShotCall C;
  if (C.open(in->device, L.bytes) != TBC_OK) return C.status;
  C.image(img);
  C.fill(L.val, 0, L.zero_bytes());
  C.fill(L.skew_first, 0xFF, L.ones_bytes());
  const lgsn::SnArgs A = lgsn::args(in, P, C.base());
  C.timed([&] { lgsn::launch_filter(C.stream, A); });
  C.get(&acc, L.acc, sizeof acc);
  if (C.sync() != TBC_OK) return C.status;
  C.timed([&] { lgsn::launch_rest(C.stream, A, acc.bad_values ? 0u : acc.n_candidates); });    // (bad values: only the summary is wanted)
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_snap_summary));
  if (C.sync() != TBC_OK) return C.status;
  out->summary.ns_device = C.ns_device();
  out->summary.bytes_in = C.bytes_in;
  if (out->summary.bad_values) {
    set_error("%s: %u reads hold counters whose magnitudes add up to 2^63 or more", fn, out->summary.bad_values);
    return TBC_ERR_UNSUPPORTED;
  }
  const size_t R = P.n_reads;
  C.get(out->skew_count, L.skew_count, R * 4); C.get(out->skew_first, L.skew_first, R * 4);
  C.get(out->skew_key, L.skew_key, R * 8); C.get(out->snap_flags, L.snap_flags, R);
  return C.sync();
}

}  // namespace

extern "C" tbc_status tbc_ledger_snapshots(const tbc_ledger_in* in, tbc_ledger_snap_out* out) { return oneshot_entry("tbc_ledger_snapshots", in, out, snap_check); }
