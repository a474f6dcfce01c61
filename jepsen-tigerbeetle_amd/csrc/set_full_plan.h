// set_full_plan.h -- the plan table of a set-full object: what every kernel of set_full.hip and set_full_results.h finds its key with.
#pragma once
#include <cstdint>

namespace {

constexpr uint32_t kNoneU = 0xFFFFFFFFu;

// ---- the plan: every object holds n_keys keys (tbc_setfull_create / _create_rows: one) in ONE arena, and each pass is ONE launch over
// the tiles of all keys.  The plan table (built on the host at create) gives each key its arrays' offsets, its chunking and the first tile
// of each grid; a workgroup finds its key by a binary search over those first tiles (uniform across the workgroup: scalar loads) and
// then works on that key alone.  Each key's pitch is a multiple of four words, so every 16 B load and store of the scan is aligned; the
// bits at or above a key's E never count (the kernels mask them, and the padding words of a row are zeros).
struct SfKeyPlan {                 // one key (device table; offsets in 32-bit words)
  uint32_t E, R, WPR, PITCH, rows_per_chunk, chunks, elem_base, row_base;
  uint32_t pmax_off, any_gy;
  unsigned long long m_off, sum_off;
};
enum { kFirstRows = 0, kFirstPrefix, kFirstAny, kFirstResolve, kFirstSelect, kFirsts };   // first[g * (n_keys + 1) + k]: key k's first tile in grid g
                                                                                         // (kFirstSelect: the results' passes, set_full_results.h)

// the last key whose first tile (row) is <= b: keys with no tile share their successor's first and are never picked for a tile of theirs
__device__ __forceinline__ uint32_t sf_find_key(const uint32_t* __restrict__ first, uint32_t n_keys, uint32_t b) {
  uint32_t lo = 0, hi = n_keys;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (first[mid] <= b) lo = mid; else hi = mid; }
  return lo;
}

}  // namespace
