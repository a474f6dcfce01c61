// ledger_search.h -- the small device functions the ledger's kernel sets share (ledger_kernels.h: tbc_ledger_check; ledger_rt_kernels.h:
// tbc_ledger_realtime): signed order as unsigned order, a lane's row by a binary search of running lengths, an id among the sorted accounts.
#pragma once
#include <cstdint>

namespace {

// signed order as unsigned order, and back
__device__ __forceinline__ unsigned long long lg_key(long long v) { return (unsigned long long)v ^ 0x8000000000000000ull; }
__device__ __forceinline__ long long lg_unkey(unsigned long long k) { return (long long)(k ^ 0x8000000000000000ull); }

// the last row whose running sum is <= g (rows of no micro-ops share their successor's and are never picked)
template <class T>
__device__ __forceinline__ uint32_t lg_row_of(const T* __restrict__ cum, uint32_t n, unsigned long long g) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (cum[mid] <= g) lo = mid; else hi = mid; }
  return lo;
}

__device__ __forceinline__ bool lg_is_account(const long long* __restrict__ acct, uint32_t n, long long id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (acct[mid] < id) lo = mid + 1u; else hi = mid; }
  return lo < n && acct[lo] == id;
}

// the id's number among the sorted accounts, 0xFFFFFFFF if it is none
__device__ __forceinline__ uint32_t lg_account_no(const long long* __restrict__ acct, uint32_t n, long long id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (acct[mid] < id) lo = mid + 1u; else hi = mid; }
  return lo < n && acct[lo] == id ? lo : 0xFFFFFFFFu;
}

}  // namespace
