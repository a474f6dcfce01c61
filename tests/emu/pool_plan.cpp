// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  pool_plan.cpp: what a pass zeroes of a batch's growth pool (csrc/pool_plan.h -- the very
// functions batch_run.hip's first_pass and its pool_zero_written_kernel go through) against a model of the device's memory, in a program
// of its own, the one to build with -fsanitize=address,undefined (tests/test_pool_plan_host.py does):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I jepsen-tigerbeetle_amd/csrc tests/emu/pool_plan.cpp -o pool_plan && ./pool_plan
// The model: a pool of exactly pool_words words and a cursor, both garbage when the memory is new; a search hands out grants as the
// kernels do (the cursor moves by what is asked, a grant that does not fit is not written) and fills what it was handed.  A batch goes
// through seeded sequences of the events of its life -- passes whose searches grow nothing, a little, past the end of the pool; a
// second search in the same run (the race's resumed default order); a fresh input that outgrows the arenas (new memory, the pass number
// starts over); 255 passes and the wrap -- and before every search EVERY word of the pool must be zero, with no more zeroed than the
// plan says.  The pool is exactly as long as pool_words, so a store past its end is the sanitizer's to see.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pool_plan.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

namespace {

uint64_t rng_state = 1;
uint64_t rnd(uint64_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state % n; }

struct Device {          // the pool's memory and its cursor, as the kernels see them
  std::vector<uint64_t> pool;
  unsigned long long cursor = 0;
  void fresh(uint64_t words) {          // hipMalloc: contents undefined
    pool.assign(words, 0);
    for (uint64_t& w : pool) w = rnd(3) ? rnd(~0ull) | 1ull : 0ull;
    cursor = rnd(2) ? rnd(4 * words + 1) : ~0ull - rnd(1000);
  }
  // grow_group / grow_visited_set: returns whether the grant fitted
  bool grant(uint64_t need) {
    const unsigned long long base = cursor;
    cursor += need;
    if (base + need > pool.size()) return false;
    for (uint64_t i = 0; i < need; i++) { CHECK(pool[base + i] == 0ull); pool[base + i] = rnd(~0ull) | 1ull; }      // (claimed by compare-and-swap from zero)
    return true;
  }
};

struct Batch {
  tbc::PoolState pool_state;
  uint32_t epoch = 0;
  bool use_epoch = true;
  Device dev;
  uint64_t zeroed_words = 0, whole = 0, passes = 0;

  void create(uint64_t words, bool lanes) { dev.fresh(words); pool_state = tbc::PoolState{}; epoch = 0; use_epoch = lanes; }
  void regrow(uint64_t words) { pool_state.replaced(); dev.fresh(words); epoch = 0; }          // batch_stream.hip: a fresh input outgrew the arenas
  void new_tab_only() { epoch = 0; }                                                             // ... the visited-set arena alone

  // first_pass up to the search: the zeroing, then the memset of the cursor
  void zero() {
    if (use_epoch) epoch = epoch % 255u + 1u;
    if (tbc::pool_zero_whole(pool_state, use_epoch, epoch)) {
      for (uint64_t& w : dev.pool) w = 0ull;
      zeroed_words += dev.pool.size(); whole++;
    } else {
      // pool_zero_written_kernel: a grid of threads, two words each, striding
      const uint64_t n = tbc::pool_written(dev.cursor, dev.pool.size());
      const uint64_t threads = 6, stride = threads * 2u;
      for (uint64_t t = 0; t < threads; t++)
        for (uint64_t i = t * 2u; i < n; i += stride) {
          if (i + 1u < n) { dev.pool[i] = 0ull; dev.pool[i + 1u] = 0ull; }
          else dev.pool[i] = 0ull;
        }
      zeroed_words += n;
    }
    dev.cursor = 0;
    passes++;
    for (uint64_t w : dev.pool) CHECK(w == 0ull);
  }
  // a search: `grants` requests of up to `max_need` words
  void search(uint32_t grants, uint64_t max_need) {
    bool fitted = true;
    for (uint32_t g = 0; g < grants; g++) {
      const bool ok = dev.grant(1 + rnd(max_need));
      CHECK(fitted || !ok);              // once a grant has not fitted, none does: nothing is written past the cursor's first overshoot
      fitted = ok;
    }
  }
};

}  // namespace

int main() {
  CHECK(tbc::pool_written(0, 10) == 0 && tbc::pool_written(9, 10) == 9 && tbc::pool_written(10, 10) == 10 && tbc::pool_written(~0ull, 10) == 10 &&
        tbc::pool_written(5, 0) == 0);
  uint64_t total_passes = 0, total_whole = 0;
  for (uint64_t seed = 1; seed <= 40; seed++) {
    rng_state = 0x9E3779B97F4A7C15ull * seed;
    Batch B;
    const uint64_t words = seed % 7 == 0 ? 1 : 1 + rnd(700);
    B.create(words, seed % 4 != 0);
    // the first pass zeroes everything, whatever the memory held
    B.zero();
    CHECK(B.whole == 1);
    B.search(0, 1);
    // a pass after one that grew nothing zeroes nothing
    { const uint64_t z = B.zeroed_words; B.zero(); CHECK(B.zeroed_words == z); }
    for (int ev = 0; ev < 600; ev++) {
      const uint64_t before = B.zeroed_words, wh = B.whole;
      const uint64_t dirty = tbc::pool_written(B.dev.cursor, B.dev.pool.size());
      const uint64_t what = rnd(100);
      if (what < 2) { B.regrow(B.dev.pool.size() + 1 + rnd(300)); B.zero(); CHECK(B.whole == wh + 1); }
      else if (what < 4) { B.new_tab_only(); B.zero(); CHECK(B.whole == wh + (B.use_epoch ? 1 : 0)); }
      else {
        const uint32_t was = B.epoch;
        B.zero();
        const bool wrapped = B.use_epoch && was == 255u;
        CHECK(B.whole == wh + (wrapped ? 1 : 0));
        if (!wrapped) CHECK(B.zeroed_words == before + dirty);          // exactly what the searches were handed, no more
      }
      // the searches of this run: nothing, a few small sets, or more than the pool holds; sometimes a second search goes on
      const uint64_t kind = rnd(10);
      if (kind >= 6) B.search(1 + (uint32_t)rnd(5), kind == 9 ? B.dev.pool.size() : 1 + B.dev.pool.size() / 8);
      if (rnd(8) == 0) B.search(1 + (uint32_t)rnd(3), 1 + B.dev.pool.size() / 4);
    }
    total_passes += B.passes; total_whole += B.whole;
  }
  std::printf("%llu passes checked, %llu of them zeroed the whole pool\n", (unsigned long long)total_passes, (unsigned long long)total_whole);
  return 0;
}
