// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_setfull_results.cpp: the kernels of csrc/set_full_results.h (the very file hipcc
// compiles into libtbcheck.so) under the wavefront / workgroup emulator, launched in the order tbc_setfull_results launches them.
// Built as a shared object by tests/test_set_full_results_emu.py and fed the three indices per element; what it returns is compared
// with numpy there.  The emulator headers have ballots, lane reads, the workgroup barrier and LDS adds; the few other things the
// kernels use -- lane shuffles, 64-bit atomics on global memory, an atomic load -- are stated here on top of the emulator's rendezvous.
#include <cstdint>
#include <vector>
#include "tbcheck.h"
#define TBC_EMU 1
#include "wave_env_emu.h"
#include "wave_env_wg_emu.h"

#define __global__
#define __launch_bounds__(...)
#define __forceinline__ inline
#define __shared__ static
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))
#define __popcll(x) __builtin_popcountll(x)
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
// a lane shuffle is a rendezvous: every lane deposits, each reads its partner's deposit (a lane that has ended reads as 0)
static inline uint64_t emu_shfl(uint64_t v, int src_of_me, int site) {
  const int me = (int)wv::lane_id();
  const uint64_t* s = wv::gather(v, site);
  return src_of_me >= 0 && src_of_me < 64 ? s[src_of_me] : s[me];
}
#define __shfl_xor(v, d) ((decltype(v))emu_shfl((uint64_t)(v), (int)wv::lane_id() ^ (d), 200000 + __LINE__))
#define __shfl_up(v, d) ((decltype(v))emu_shfl((uint64_t)(uint32_t)(v), (int)wv::lane_id() - (d), 300000 + __LINE__))
template <class T> static inline T atomicMin(T* p, T v) { const T o = *p; if (v < o) *p = v; return o; }
template <class T> static inline T atomicMax(T* p, T v) { const T o = *p; if (v > o) *p = v; return o; }

#include "set_full_results.h"

namespace {
struct Call { void (*k0)(SfResArgs); void (*k1)(SfResArgs, uint32_t); SfResArgs A; uint32_t level; };
void trampoline(void* arg, uint32_t) { Call* c = (Call*)arg; if (c->k0) c->k0(c->A); else c->k1(c->A, c->level); }
void launch(Call c, uint32_t grid, int waves, uint64_t seed) {
  for (uint32_t b = 0; b < grid; b++) wv::run_workgroup(trampoline, &c, waves, b, seed + b);
}
}  // namespace

// n_keys keys of E[k] elements, the three indices key after key -> what tbc_setfull_keys_results returns
extern "C" int emu_setfull_results(uint32_t n_keys, const uint32_t* E, const uint32_t* known, const uint32_t* lp, const uint32_t* la,
                                   const int64_t* op_time, const uint64_t* time_off, uint64_t unit, uint32_t flags, uint8_t* outcome,
                                   int64_t* slat, int64_t* llat, tbc_setfull_key_summary* summary, uint64_t seed) {
  // the library's own plan (csrc/set_full_plan.h) of these keys -- without reads: the results' passes look at the elements only
  const std::vector<uint32_t> no_reads(n_keys, 0u);
  const SfLayout L = sf_make_layout(n_keys, E, no_reads.data(), SfSource::Rows, 0u, 0u);
  const std::vector<SfKeyPlan>& plan = L.plan;
  const std::vector<uint32_t>& first = L.first;
  const uint32_t tiles = (uint32_t)L.tiles[kFirstSelect];
  std::vector<SfKeyAcc> acc(n_keys);
  std::vector<SfSel> sel((size_t)n_keys * kSelTargets, SfSel{0ull, 0u, 0u});
  std::vector<uint32_t> hist((size_t)n_keys * kSelTargets * kSelBins, 0u);
  SfResArgs A;
  A.plan = plan.data(); A.first = first.data(); A.n_keys = n_keys; A.flags = flags;
  A.known = known; A.lp = lp; A.la = la;
  A.op_time = (const long long*)op_time; A.time_off = (const unsigned long long*)time_off; A.unit = op_time ? unit : 1ull;
  A.outcome = outcome; A.slat = (long long*)slat; A.llat = (long long*)llat;
  A.acc = acc.data(); A.sel = sel.data(); A.hist = hist.data(); A.summary = summary;
  const uint32_t key_blocks = (n_keys + 255u) / 256u;
  launch(Call{sf_results_init_kernel, nullptr, A, 0u}, key_blocks, 4, seed);
  if (tiles) {
    launch(Call{sf_decide_kernel, nullptr, A, 0u}, tiles, 4, seed + 1000);
    for (uint32_t level = 8; level-- > 0;) {
      launch(Call{nullptr, sf_select_hist_kernel, A, level}, tiles, 4, seed + 2000 + level);
      launch(Call{nullptr, sf_select_pick_kernel, A, level}, n_keys, (int)kSelTargets, seed + 3000 + level);
    }
    launch(Call{sf_worst_collect_kernel, nullptr, A, 0u}, tiles, 4, seed + 4000);
  }
  launch(Call{sf_results_final_kernel, nullptr, A, 0u}, key_blocks, 4, seed + 5000);
  for (uint32_t i = 0; i < hist.size(); i++) if (hist[i]) return 1;        // every pick leaves its histogram zeroed
  return 0;
}
