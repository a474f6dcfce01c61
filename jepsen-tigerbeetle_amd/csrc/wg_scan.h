// wg_scan.h -- an exclusive scan over a workgroup's 256 threads in LDS, for any associative `op` with identity `ident`: what the carried
// totals of a chunked scan are made with (perf_kernels.h: the open scan's per-class counts; ledger_rt_kernels.h: per-account counts, sums
// and maxima).  s: 256 words of LDS; `total`: op over all 256.  Called by the whole workgroup.
#pragma once
#include "wave_env_wg.h"

namespace {

template <class T, class Op>
__device__ __forceinline__ T wg_scan_excl(T v, T* s, uint32_t t, T ident, T& total, Op op) {
  s[t] = v;
  wv::wg_barrier();
  for (uint32_t d = 1; d < 256u; d <<= 1) {
    const T o = t >= d ? s[t - d] : ident;
    wv::wg_barrier();
    s[t] = op(o, s[t]);
    wv::wg_barrier();
  }
  const T ex = t ? s[t - 1u] : ident;
  total = s[255];
  wv::wg_barrier();                                                         // (s is written again only when everybody has read it)
  return ex;
}

}  // namespace
