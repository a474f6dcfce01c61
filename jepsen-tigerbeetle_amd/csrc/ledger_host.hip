// ledger_host.hip -- tbc_ledger_check, the entry point of the ledger workload's checkers (include/tbcheck.h): every rule of the input on
// the host, the plan (ledger_plan.h), ONE device allocation laid out by it, the head as one image and the caller's micro-op columns
// straight to their regions, the kernels (ledger.hip) between two events, and the results back in one copy per array the caller asked
// for.  One-shot and re-entrant: the stream, the events and the arena are the call's own and are gone on every path out.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include "oneshot_call.h"
#include "ledger_plan.h"

using namespace tbc;

#define LG_TRY TBC_ONESHOT_TRY

namespace {

using LgCall = OneShotCall;

tbc_status lg_check(const char* fn, const tbc_ledger_in* in, tbc_ledger_out* out) {
  std::string err;
  if (!lg::validate(fn, in, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  lg::Plan P;
  if (!lg::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  const tbc_status dev = oneshot_check_device(in->device);
  if (dev != TBC_OK) return dev;
  const lg::LgArena& L = P.arena;
  const std::vector<unsigned char> img = lg::head_image(P);
  LgCall C;
  LG_TRY(hipGetDevice(&C.device_before));
  LG_TRY(hipSetDevice((int)in->device));
  LG_TRY(hipMalloc(&C.arena, std::max<size_t>(L.bytes, 256)));
  LG_TRY(hipStreamCreateWithFlags(&C.stream, hipStreamNonBlocking));
  LG_TRY(hipEventCreate(&C.ev0)); LG_TRY(hipEventCreate(&C.ev1));
  char* const base = static_cast<char*>(C.arena);
  const auto at = [&](const lg::LgRegion& r) { return base + r.at; };
  uint64_t bytes_in = img.size();
  const auto put = [&](const lg::LgRegion& r, const void* src) {
    bytes_in += r.bytes;
    return r.bytes ? hipMemcpyAsync(at(r), src, r.bytes, hipMemcpyHostToDevice, C.stream) : hipSuccess;
  };
  // (the copies read pageable memory of the caller's: the synchronise below ends them before the call returns)
  LG_TRY(hipMemcpyAsync(base, img.data(), img.size(), hipMemcpyHostToDevice, C.stream));
  LG_TRY(put(L.mop_id, in->mop_id)); LG_TRY(put(L.mop_a, in->mop_a)); LG_TRY(put(L.mop_b, in->mop_b)); LG_TRY(put(L.mop_c, in->mop_c));
  LG_TRY(put(L.mop_flags, in->mop_flags));
  if (L.zero_bytes()) LG_TRY(hipMemsetAsync(at(L.slots), 0, L.zero_bytes(), C.stream));
  lg::LgArgs A{};
  A.acc = (lg::LgAcc*)at(L.acc); A.summary = (tbc_ledger_summary*)at(L.summary);
  A.mop_id = (const long long*)at(L.mop_id); A.mop_a = (const long long*)at(L.mop_a); A.mop_b = (const long long*)at(L.mop_b);
  A.mop_c = (const long long*)at(L.mop_c); A.mop_flags = (const uint8_t*)at(L.mop_flags);
  A.accounts = (const long long*)at(L.accounts); A.n_accounts = in->n_accounts; A.negative_balances = in->negative_balances;
  A.total_amount = in->total_amount;
  A.read_lo = (const unsigned long long*)at(L.read_lo); A.read_cum = (const unsigned long long*)at(L.read_cum);
  A.run_first = (const uint32_t*)at(L.run_first); A.n_reads = P.n_reads; A.n_runs = P.n_runs;
  A.read_error = (uint8_t*)at(L.read_error); A.read_total = (long long*)at(L.read_total); A.read_badness = (long long*)at(L.read_badness);
  A.transfer = (const long long*)at(L.transfer); A.slots = at(L.slots); A.n_transfers = P.n_transfers; A.tab_mask = P.tab_mask;
  A.fl_lo = (const unsigned long long*)at(L.fl_lo); A.fl_cum = (const unsigned long long*)at(L.fl_cum); A.n_final_lookups = P.n_final_lookups;
  A.missing = (uint32_t*)at(L.missing);
  A.fr_lo = (const unsigned long long*)at(L.fr_lo); A.fr_cum = (const unsigned long long*)at(L.fr_cum); A.n_final_reads = P.n_final_reads;
  A.fr_unlike = (uint32_t*)at(L.fr_unlike); A.fl_unlike = (uint32_t*)at(L.fl_unlike);
  LG_TRY(hipEventRecord(C.ev0, C.stream));
  lg::launch(C.stream, A, P.fr_cum.back(), P.fl_cum.back());
  LG_TRY(hipGetLastError());
  LG_TRY(hipEventRecord(C.ev1, C.stream));
  const auto get = [&](void* dst, const lg::LgRegion& r, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, at(r), bytes, hipMemcpyDeviceToHost, C.stream) : hipSuccess;
  };
  const size_t R = P.n_reads, FR = P.n_final_reads, FL = P.n_final_lookups;
  LG_TRY(get(out->read_error, L.read_error, R)); LG_TRY(get(out->read_total, L.read_total, R * 8)); LG_TRY(get(out->read_badness, L.read_badness, R * 8));
  LG_TRY(get(out->lookup_missing, L.missing, FL * 4));
  LG_TRY(get(out->final_read_unlike, L.fr_unlike, FR)); LG_TRY(get(out->final_lookup_unlike, L.fl_unlike, FL));
  LG_TRY(get(&out->summary, L.summary, sizeof(tbc_ledger_summary)));
  LG_TRY(hipStreamSynchronize(C.stream));
  float ms = 0;
  LG_TRY(hipEventElapsedTime(&ms, C.ev0, C.ev1));
  out->summary.ns_device = (uint64_t)(ms * 1e6);
  out->summary.bytes_in = bytes_in;
  return TBC_OK;
}

}  // namespace

extern "C" tbc_status tbc_ledger_check(const tbc_ledger_in* in, tbc_ledger_out* out) {
  const char* fn = "tbc_ledger_check";
  if (!in || !out) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  try {
    return lg_check(fn, in, out);
  } catch (const std::bad_alloc&) {
    set_error("%s: host memory", fn);
    return TBC_ERR_OOM;
  }
}
