// perf_host.hip -- tbc_perf_series and tbc_perf_plan_sizes, the entry points of the perf series (include/tbcheck.h): every rule of the
// input on the host, the plan (perf_plan.h), ONE device allocation laid out by it, the zeroed head, the plan's partner column and the
// caller's columns straight to their regions, the kernels (perf.hip) between two events, and the results back in one copy per array the
// caller asked for.  One-shot and re-entrant: the stream, the events and the arena are the call's own and are gone on every path out.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <new>
#include <string>
#include "oneshot_call.h"
#include "perf_plan.h"

using namespace tbc;

namespace {

tbc_status pf_series(const char* fn, const tbc_perf_in* in, tbc_perf_out* out) {
  std::string err;
  tbc_status st = pf::validate(fn, in, err);
  if (st != TBC_OK) { set_error("%s", err.c_str()); return st; }
  pf::Plan P;
  st = pf::plan(fn, in, P, err);
  if (st != TBC_OK) { set_error("%s", err.c_str()); return st; }
  st = oneshot_check_device(in->device);
  if (st != TBC_OK) return st;
  const pf::PfArena& L = P.arena;
  OneShotCall C;
  TBC_ONESHOT_TRY(hipGetDevice(&C.device_before));
  TBC_ONESHOT_TRY(hipSetDevice((int)in->device));
  TBC_ONESHOT_TRY(hipMalloc(&C.arena, std::max<size_t>(L.bytes, 256)));
  TBC_ONESHOT_TRY(hipStreamCreateWithFlags(&C.stream, hipStreamNonBlocking));
  TBC_ONESHOT_TRY(hipEventCreate(&C.ev0)); TBC_ONESHOT_TRY(hipEventCreate(&C.ev1));
  char* const base = static_cast<char*>(C.arena);
  const auto at = [&](const pf::PfRegion& r) { return base + r.at; };
  uint64_t bytes_in = 0;
  const auto put = [&](const pf::PfRegion& r, const void* src) {
    bytes_in += r.bytes;
    return r.bytes ? hipMemcpyAsync(at(r), src, r.bytes, hipMemcpyHostToDevice, C.stream) : hipSuccess;
  };
  // (the copies read pageable memory of the caller's and the plan's: the synchronise below ends them before the call returns)
  TBC_ONESHOT_TRY(hipMemsetAsync(base, 0, L.zero_bytes(), C.stream));
  TBC_ONESHOT_TRY(put(L.partner, P.partner.data()));
  TBC_ONESHOT_TRY(put(L.time, in->time)); TBC_ONESHOT_TRY(put(L.process, in->process)); TBC_ONESHOT_TRY(put(L.type, in->type));
  TBC_ONESHOT_TRY(put(L.f, in->f));
  const pf::PfArgs A = pf::args(P, base);
  TBC_ONESHOT_TRY(hipEventRecord(C.ev0, C.stream));
  pf::launch(C.stream, A);
  TBC_ONESHOT_TRY(hipGetLastError());
  TBC_ONESHOT_TRY(hipEventRecord(C.ev1, C.stream));
  const auto get = [&](void* dst, const pf::PfRegion& r) {
    return dst && r.bytes ? hipMemcpyAsync(dst, at(r), r.bytes, hipMemcpyDeviceToHost, C.stream) : hipSuccess;
  };
  TBC_ONESHOT_TRY(get(out->op_latency, L.op_latency)); TBC_ONESHOT_TRY(get(out->op_outcome, L.op_outcome));
  TBC_ONESHOT_TRY(get(out->op_open_after, L.op_open_after));
  TBC_ONESHOT_TRY(get(out->q_count, L.q_count)); TBC_ONESHOT_TRY(get(out->q_value, L.q_value));
  TBC_ONESHOT_TRY(get(out->rate_count, L.rate_count));
  TBC_ONESHOT_TRY(get(out->open_last, L.open_last)); TBC_ONESHOT_TRY(get(out->open_fill, L.open_fill));
  TBC_ONESHOT_TRY(get(&out->summary, L.summary));
  TBC_ONESHOT_TRY(hipStreamSynchronize(C.stream));
  float ms = 0;
  TBC_ONESHOT_TRY(hipEventElapsedTime(&ms, C.ev0, C.ev1));
  out->summary.ns_device = (uint64_t)(ms * 1e6);
  out->summary.bytes_in = bytes_in;
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

extern "C" tbc_status tbc_perf_series(const tbc_perf_in* in, tbc_perf_out* out) {
  const char* fn = "tbc_perf_series";
  if (!in || !out) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  try {
    return pf_series(fn, in, out);
  } catch (const std::bad_alloc&) {
    set_error("%s: host memory", fn);
    return TBC_ERR_OOM;
  }
}
