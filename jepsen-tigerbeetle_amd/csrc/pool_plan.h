// pool_plan.h -- what a pass zeroes of a batch's GROWTH POOL (batch_run.hip first_pass), for the host and the device.
//
// A history whose visited set fills up moves to a 4x larger one carved from the batch's pool (wgl_narrow_impl.h grow_group, wgl_beam.hip
// grow_visited_set): the wavefront adds what it needs to the pool's cursor, a word in device memory, and claims entries of the new set
// by compare-and-swap from zero -- so the words it is handed must be zero.  Until now every pass zeroed the whole pool, a tenth of the
// visited-set arena (1.7 GB at the bench's shape), although the headline's sets almost never grow.  But the pool is handed out from
// word 0 upwards, and a grant that does not fit is not written (the cursor still moves: it may end past the pool): after any number of
// searches the words that may be non-zero are [0, min(cursor, pool_words)).  The cursor never leaves the device -- the pass that zeroes
// reads it there (pool_zero_written_kernel), whichever phase of the last run moved it last.
//
// That leaves the host ONE thing to know: whether the pool is CLEAN, i.e. whether every word at or past the device's cursor is zero and
// the cursor counts grants of THIS memory.  It is not after the pool's memory was allocated or replaced (contents undefined, and so is
// the cursor's before the first pass); it is from the first pass's zeroing on.  Where the visited-set arena starts over -- the first
// pass, a fresh input that outgrew the arenas, the pass number's wrap: B->epoch back at 1 -- the whole pool is zeroed with it.
//
// tests/emu/pool_plan.cpp runs these functions through the events of a batch's life against a model of the device's memory.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TBC_POOL_HD __host__ __device__
#else
#define TBC_POOL_HD
#endif

namespace tbc {

struct PoolState {
  bool clean = false;          // every word at or past the device's cursor is zero; false: new memory, zero all of it
  void replaced() { clean = false; }          // the pool's memory was allocated or regrown
};

// the words a pass must zero when the pool is clean: what the searches since the last zeroing may have written
TBC_POOL_HD inline uint64_t pool_written(uint64_t cursor, uint64_t pool_words) { return cursor < pool_words ? cursor : pool_words; }

// does this pass zero the whole pool?  (use_epoch: the batch's visited sets are tagged with the pass number, `epoch` is this pass's)
inline bool pool_zero_whole(PoolState& st, bool use_epoch, uint32_t epoch) {
  const bool whole = !st.clean || (use_epoch && epoch == 1u);
  st.clean = true;             // (the zeroing is queued in front of the pass's search, on its stream)
  return whole;
}

}  // namespace tbc
