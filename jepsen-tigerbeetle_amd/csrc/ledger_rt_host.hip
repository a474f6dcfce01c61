// ledger_rt_host.hip -- tbc_ledger_realtime, the entry point of the realtime bounds on the ledger's posted counters (include/tbcheck.h):
// every rule of the input on the host, the plan (ledger_rt_plan.h), ONE device allocation laid out by it, the head and the micro-op
// columns of the ops the kernels look at as one image in one copy, the kernels (ledger_rt.hip) between two events, the summary back -- an amount out of
// range, which only the device has looked at, ends the call there -- and then one copy per array the caller asked for.  One-shot and
// re-entrant through oneshot_call.h, as tbc_ledger_check is.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <new>
#include <string>
#include <vector>
#include "oneshot_call.h"
#include "ledger_rt_plan.h"

using namespace tbc;

namespace {

tbc_status rt_check(const char* fn, const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out) {
  std::string err;
  if (!lgrt::validate(fn, in, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  lgrt::Plan P;
  if (!lgrt::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  const tbc_status dev = oneshot_check_device(in->ledger.device);
  if (dev != TBC_OK) return dev;
  const lgrt::RtArena& L = P.arena;
  const std::vector<unsigned char> img = lgrt::image(in, P);
  OneShotCall C;
  TBC_ONESHOT_TRY(hipGetDevice(&C.device_before));
  TBC_ONESHOT_TRY(hipSetDevice((int)in->ledger.device));
  TBC_ONESHOT_TRY(hipMalloc(&C.arena, std::max<size_t>(L.bytes, 256)));
  TBC_ONESHOT_TRY(hipStreamCreateWithFlags(&C.stream, hipStreamNonBlocking));
  TBC_ONESHOT_TRY(hipEventCreate(&C.ev0)); TBC_ONESHOT_TRY(hipEventCreate(&C.ev1));
  char* const base = static_cast<char*>(C.arena);
  const auto at = [&](const lg::LgRegion& r) { return base + r.at; };
  // (one copy out of the image, which lives until the synchronise below)
  if (!img.empty()) TBC_ONESHOT_TRY(hipMemcpyAsync(base, img.data(), img.size(), hipMemcpyHostToDevice, C.stream));
  if (L.zero_bytes()) TBC_ONESHOT_TRY(hipMemsetAsync(at(L.carry_cnt[0]), 0, L.zero_bytes(), C.stream));
  const lgrt::RtArgs A = lgrt::args(in, P, base);
  TBC_ONESHOT_TRY(hipEventRecord(C.ev0, C.stream));
  lgrt::launch(C.stream, A);
  TBC_ONESHOT_TRY(hipGetLastError());
  TBC_ONESHOT_TRY(hipEventRecord(C.ev1, C.stream));
  TBC_ONESHOT_TRY(hipMemcpyAsync(&out->summary, at(L.summary), sizeof(tbc_ledger_rt_summary), hipMemcpyDeviceToHost, C.stream));
  TBC_ONESHOT_TRY(hipStreamSynchronize(C.stream));
  float ms = 0;
  TBC_ONESHOT_TRY(hipEventElapsedTime(&ms, C.ev0, C.ev1));
  out->summary.ns_device = (uint64_t)(ms * 1e6);
  out->summary.bytes_in = img.size();
  if (out->summary.bad_amounts) {
    set_error("%s: %u transfer amounts are outside [0, 2^31)", fn, out->summary.bad_amounts);
    return TBC_ERR_UNSUPPORTED;
  }
  const auto get = [&](void* dst, const lg::LgRegion& r, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, at(r), bytes, hipMemcpyDeviceToHost, C.stream) : hipSuccess;
  };
  const size_t R = P.n_reads, Mr = (size_t)P.rows[lgrt::kReads].mops();
  TBC_ONESHOT_TRY(get(out->rt_bits, L.rt_bits, R)); TBC_ONESHOT_TRY(get(out->rt_miss, L.rt_miss, R * 24));
  TBC_ONESHOT_TRY(get(out->mop_lo, L.mop_lo, Mr * 16)); TBC_ONESHOT_TRY(get(out->mop_hi, L.mop_hi, Mr * 16)); TBC_ONESHOT_TRY(get(out->mop_floor, L.mop_floor, Mr * 16));
  TBC_ONESHOT_TRY(hipStreamSynchronize(C.stream));
  return TBC_OK;
}

}  // namespace

extern "C" tbc_status tbc_ledger_realtime(const tbc_ledger_rt_in* in, tbc_ledger_rt_out* out) {
  const char* fn = "tbc_ledger_realtime";
  if (!in || !out) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  try {
    return rt_check(fn, in, out);
  } catch (const std::bad_alloc&) {
    set_error("%s: host memory", fn);
    return TBC_ERR_OOM;
  }
}
