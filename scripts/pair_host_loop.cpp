// pair_host_loop.cpp -- what scripts/gpu_pair_events.py times as "the host loop": tbc_pair_events, a history a call, over the histories
// of a tbc_event_batch on `threads` std::threads (contiguous shares of the histories), history h's ops written at ev_off[h] of
// preallocated op arrays.  The entry point is passed in as a pointer, so this unit links against nothing; the script compiles it with
// the host compiler into a temporary shared object.  No Python runs inside the timed region.  Returns the seconds the loop took, or -1
// if a history was refused.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>
#include "tbcheck.h"

using pair_fn = tbc_status (*)(const tbc_events*, uint8_t*, int32_t*, int32_t*, int32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*);

extern "C" double pair_host_loop(void* fn, const tbc_event_batch* in, uint8_t* f, int32_t* a, int32_t* b, int32_t* process,
                                 uint32_t* inv_pos, uint32_t* ret_pos, uint32_t* n_ops, uint32_t* n_process, uint32_t threads) {
  const pair_fn pair = reinterpret_cast<pair_fn>(fn);
  std::atomic<int> bad{0};
  const auto work = [&](uint32_t lo, uint32_t hi) {
    for (uint32_t h = lo; h < hi; h++) {
      const uint64_t e0 = in->ev_off[h];
      const tbc_events ev{(uint32_t)(in->ev_off[h + 1] - e0), in->type + e0, in->process + e0, in->f + e0, in->a + e0, in->b + e0};
      if (pair(&ev, f + e0, a + e0, b + e0, process + e0, inv_pos + e0, ret_pos + e0, n_ops + h, n_process + h) != TBC_OK) bad++;
    }
  };
  const auto t0 = std::chrono::steady_clock::now();
  if (threads <= 1) work(0, in->n_hist);
  else {
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < threads; t++)
      th.emplace_back(work, (uint32_t)((uint64_t)in->n_hist * t / threads), (uint32_t)((uint64_t)in->n_hist * (t + 1) / threads));
    for (auto& x : th) x.join();
  }
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return bad ? -1.0 : s;
}
