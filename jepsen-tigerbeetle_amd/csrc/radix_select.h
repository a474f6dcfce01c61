// radix_select.h -- what the exact order statistics of set_full_results.h (latency quantiles of set-full, a key split across
// workgroups, histograms in memory) and of perf_kernels.h (latency quantiles per (f, second), a cell per workgroup, histograms in LDS)
// have in common: the rank of a quantile, and one level of the most-significant-digit-first radix select over 64-bit values, eight
// bits a level -- a wavefront finds, in a histogram of 256 bins, the bin that holds rank k.  The callers keep the histograms, the
// prefixes and the order of the levels; the lane shuffles are plain HIP, which the emulator programs of both callers state.
#pragma once
#include "wave_env_wg.h"

namespace {

constexpr uint32_t kSelBins = 256;

__device__ __forceinline__ uint32_t sf_rank(uint32_t n, double p) {          // Python's min(n - 1, int(n * p))
  const unsigned long long r = (unsigned long long)((double)n * p);
  return r < (unsigned long long)(n - 1u) ? (uint32_t)r : n - 1u;
}
__device__ __forceinline__ bool sf_level_used(unsigned long long maxv, uint32_t level) { return (maxv >> (8u * level)) != 0ull; }

// One wavefront, lane l holding bins 4l .. 4l + 3 of a level's histogram in `h`: the bin that holds rank k (k below the histogram's
// sum) and the rank left inside that bin.  True in exactly one lane -- the one whose bins hold it, which gets `bin` and `left`.
__device__ __forceinline__ bool rs_pick(const uint4 h, uint32_t lane, uint32_t k, uint32_t& bin, uint32_t& left) {
  const uint32_t mine = h.x + h.y + h.z + h.w;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d); if (lane >= (uint32_t)d) incl += o; }
  const uint64_t at = wv::ballot(k < incl);
  if (lane != (at ? (uint32_t)__builtin_ctzll(at) : 63u)) return false;  // (the rank is below the count: some lane holds it)
  uint32_t b = 0u;
  left = k - (incl - mine);
  if (left >= h.x) { left -= h.x; b = 1u; if (left >= h.y) { left -= h.y; b = 2u; if (left >= h.z) { left -= h.z; b = 3u; } } }
  bin = 4u * lane + b;
  return true;
}

}  // namespace
