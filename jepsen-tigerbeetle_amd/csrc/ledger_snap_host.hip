// ledger_snap_host.hip -- tbc_ledger_snapshots, the entry point of the snapshot order of a ledger's reads (include/tbcheck.h): every
// rule of the input on the host, the plan (ledger_snap_plan.h), ONE device allocation laid out by it, the head and the reads' micro-op
// columns as one image in one copy, the filter's kernels (ledger_snap.hip), the accumulators back -- a read out of range, which only the
// device has looked at, ends the call there; the number of candidates decides whether a pair kernel is launched at all --, the rest of
// the kernels, the summary back and then one copy per array the caller asked for.  The two runs of kernels lie between events of their
// own; ns_device is their sum.  One-shot and re-entrant through oneshot_call.h, as tbc_ledger_check is.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <new>
#include <string>
#include <vector>
#include "oneshot_call.h"
#include "ledger_snap_plan.h"

using namespace tbc;

namespace {

tbc_status snap_check(const char* fn, const tbc_ledger_in* in, tbc_ledger_snap_out* out) {
  std::string err;
  if (!lgsn::validate(fn, in, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  lgsn::Plan P;
  if (!lgsn::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  const tbc_status dev = oneshot_check_device(in->device);
  if (dev != TBC_OK) return dev;
  const lgsn::SnArena& L = P.arena;
  const std::vector<unsigned char> img = lgsn::image(in, P);
  OneShotCall C;
  TBC_ONESHOT_TRY(hipGetDevice(&C.device_before));
  TBC_ONESHOT_TRY(hipSetDevice((int)in->device));
  TBC_ONESHOT_TRY(hipMalloc(&C.arena, std::max<size_t>(L.bytes, 256)));
  TBC_ONESHOT_TRY(hipStreamCreateWithFlags(&C.stream, hipStreamNonBlocking));
  TBC_ONESHOT_TRY(hipEventCreate(&C.ev0)); TBC_ONESHOT_TRY(hipEventCreate(&C.ev1));
  char* const base = static_cast<char*>(C.arena);
  const auto at = [&](const lg::LgRegion& r) { return base + r.at; };
  // (one copy out of the image, which lives until the synchronise below)
  if (!img.empty()) TBC_ONESHOT_TRY(hipMemcpyAsync(base, img.data(), img.size(), hipMemcpyHostToDevice, C.stream));
  if (L.zero_bytes()) TBC_ONESHOT_TRY(hipMemsetAsync(at(L.val), 0, L.zero_bytes(), C.stream));
  if (L.ones_bytes()) TBC_ONESHOT_TRY(hipMemsetAsync(at(L.skew_first), 0xFF, L.ones_bytes(), C.stream));
  const lgsn::SnArgs A = lgsn::args(in, P, base);
  lgsn::SnAcc acc{};
  TBC_ONESHOT_TRY(hipEventRecord(C.ev0, C.stream));
  lgsn::launch_filter(C.stream, A);
  TBC_ONESHOT_TRY(hipGetLastError());
  TBC_ONESHOT_TRY(hipEventRecord(C.ev1, C.stream));
  TBC_ONESHOT_TRY(hipMemcpyAsync(&acc, at(L.acc), sizeof acc, hipMemcpyDeviceToHost, C.stream));
  TBC_ONESHOT_TRY(hipStreamSynchronize(C.stream));
  float ms_filter = 0, ms_rest = 0;
  TBC_ONESHOT_TRY(hipEventElapsedTime(&ms_filter, C.ev0, C.ev1));
  TBC_ONESHOT_TRY(hipEventRecord(C.ev0, C.stream));
  lgsn::launch_rest(C.stream, A, acc.bad_values ? 0u : acc.n_candidates);    // (bad values: only the summary is wanted)
  TBC_ONESHOT_TRY(hipGetLastError());
  TBC_ONESHOT_TRY(hipEventRecord(C.ev1, C.stream));
  TBC_ONESHOT_TRY(hipMemcpyAsync(&out->summary, at(L.summary), sizeof(tbc_ledger_snap_summary), hipMemcpyDeviceToHost, C.stream));
  TBC_ONESHOT_TRY(hipStreamSynchronize(C.stream));
  TBC_ONESHOT_TRY(hipEventElapsedTime(&ms_rest, C.ev0, C.ev1));
  out->summary.ns_device = (uint64_t)(((double)ms_filter + (double)ms_rest) * 1e6);
  out->summary.bytes_in = img.size();
  if (out->summary.bad_values) {
    set_error("%s: %u reads hold counters whose magnitudes add up to 2^63 or more", fn, out->summary.bad_values);
    return TBC_ERR_UNSUPPORTED;
  }
  const auto get = [&](void* dst, const lg::LgRegion& r, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, at(r), bytes, hipMemcpyDeviceToHost, C.stream) : hipSuccess;
  };
  const size_t R = P.n_reads;
  TBC_ONESHOT_TRY(get(out->skew_count, L.skew_count, R * 4)); TBC_ONESHOT_TRY(get(out->skew_first, L.skew_first, R * 4));
  TBC_ONESHOT_TRY(get(out->skew_key, L.skew_key, R * 8)); TBC_ONESHOT_TRY(get(out->snap_flags, L.snap_flags, R));
  TBC_ONESHOT_TRY(hipStreamSynchronize(C.stream));
  return TBC_OK;
}

}  // namespace

extern "C" tbc_status tbc_ledger_snapshots(const tbc_ledger_in* in, tbc_ledger_snap_out* out) {
  const char* fn = "tbc_ledger_snapshots";
  if (!in || !out) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  try {
    return snap_check(fn, in, out);
  } catch (const std::bad_alloc&) {
    set_error("%s: host memory", fn);
    return TBC_ERR_OOM;
  }
}
