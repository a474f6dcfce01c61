// set_full_results.h -- jepsen.checker/set-full's verdict from the scan's three indices, on the MI355X (gfx950).  Included by
// set_full_host.hip; tbc_setfull_results / tbc_setfull_keys_results run these kernels behind the scan.  (kSelTile, the elements a
// workgroup takes, is the plan's: set_full_plan.h.)
//
// The scan leaves known / last_present / last_absent per element on the device.  What follows is a fixed sequence of launches over
// the elements of ALL keys (the key of a workgroup found through the plan table, as in the scan), whatever n_keys is:
//   sf_results_init_kernel     a thread per key: the key's accumulators to their start values
//   sf_decide_kernel           a pass over the elements: gather the three times, classify, both latencies, the per-element arrays;
//                              per key the counts (ballot + popcount per wavefront, ONE atomic per wavefront and counter, and none
//                              where the wavefront has nothing to add) and the least / greatest latency of each kind (quantile
//                              points 0 and 1)
//   8 x (sf_select_hist_kernel, sf_select_pick_kernel)
//                              the exact order statistics: a most-significant-digit-first radix select over the 64-bit latencies, eight
//                              bits a level, SEVEN targets a key at once -- ranks .5 / .95 / .99 of the stable latencies, the eighth
//                              greatest stable latency (the threshold of worst-stale), ranks .5 / .95 / .99 of the lost latencies.  A
//                              level counts, per target, the digit of every value that still matches the target's prefix (histograms
//                              in LDS, their non-zero bins added to the key's histogram in memory); the pick (a wavefront per key and
//                              target) finds the bin that holds the rank, extends the prefix and leaves the histogram zeroed for the
//                              next level.  A key of any size is split across workgroups of kSelTile elements; the kernel boundary
//                              between count and pick is the only ordering needed (no fence wider than the workgroup's barrier).  A
//                              level above the highest digit the key's greatest latency uses is skipped by every workgroup of the key:
//                              latencies in milliseconds use two or three levels.
//   sf_worst_collect_kernel    the stale elements above the threshold (at most seven) and the lowest-numbered ones AT it
//   sf_results_final_kernel    a thread per key: the summary
// Cross-lane work goes through wave_env.h / wave_env_wg.h where they have the primitive (ballots, the workgroup barrier, LDS adds, the
// workgroup's index and thread); the lane shuffles of the 64-bit wavefront min / max and of the pick's prefix sum and the atomics on
// global memory are plain HIP, which tests/emu/emu_setfull_results.cpp states for the host emulator on top of its rendezvous -- these
// very kernels run there, lane by lane, against numpy (tests/test_set_full_results_emu.py).
#pragma once
#include "wave_env_wg.h"
#include "set_full_plan.h"
#include "radix_select.h"                    // sf_rank, sf_level_used, rs_pick: shared with perf_kernels.h

namespace {

constexpr uint32_t kSelTargets = 7;          // 0-2: stable .5 .95 .99; 3: the 8th greatest stable latency; 4-6: lost .5 .95 .99
constexpr uint32_t kWorst = TBC_SETFULL_WORST;

struct SfKeyAcc {                            // per key; reset by sf_results_init_kernel
  uint32_t n_lost, n_never, n_stale, n_gt;
  unsigned long long min_s, max_s, min_l, max_l;
  uint32_t eq[kWorst], gt[kWorst];           // worst-stale candidates: element numbers at / above the threshold
};
struct SfSel { unsigned long long prefix; uint32_t k, pad; };       // per (key, target): the value's bits decided so far (in place), the rank left

struct SfResArgs {
  const SfKeyPlan* plan; const uint32_t* first; uint32_t n_keys, flags;
  const uint32_t *known, *lp, *la;           // the scan's results, key after key
  const long long* op_time;                  // nullptr: time = the op index
  const unsigned long long* time_off;
  unsigned long long unit;
  uint8_t* outcome; long long *slat, *llat;
  SfKeyAcc* acc; SfSel* sel; uint32_t* hist; tbc_setfull_key_summary* summary;
};

// how many values target t selects among and the rank it wants (n = 0: the target is off)
__device__ __forceinline__ void sf_target(const SfKeyAcc& a, uint32_t E, uint32_t t, uint32_t& n, uint32_t& rank) {
  const uint32_t n_stable = E - a.n_lost - a.n_never;
  const double p = (t % 4u) == 0u ? 0.5 : ((t % 4u) == 1u ? 0.95 : 0.99);
  if (t == 3u) { n = a.n_stale > kWorst ? n_stable : 0u; rank = n ? n_stable - kWorst : 0u; return; }
  n = t < 3u ? n_stable : a.n_lost;
  rank = n ? sf_rank(n, p) : 0u;
}

__global__ __launch_bounds__(256) void sf_results_init_kernel(SfResArgs A) {
  const uint32_t k = wv::wg_index() * 256u + wv::wg_thread();
  if (k >= A.n_keys) return;
  SfKeyAcc a;
  a.n_lost = a.n_never = a.n_stale = a.n_gt = 0u;
  a.min_s = a.min_l = ~0ull; a.max_s = a.max_l = 0ull;
  for (uint32_t i = 0; i < kWorst; i++) { a.eq[i] = 0xFFFFFFFFu; a.gt[i] = 0xFFFFFFFFu; }
  A.acc[k] = a;
}

__device__ __forceinline__ unsigned long long sf_wave_min64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned long long sf_wave_max64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o > v ? o : v; }
  return v;
}
// The extremes only ever move one way, so a value the key's word already covers needs no atomic -- and a STALE copy of the word errs on
// the safe side (it covers less than the word does now).  Of the 512 wavefronts of a key of 262,144 elements a handful get through.
__device__ __forceinline__ void sf_offer_min(unsigned long long* p, unsigned long long v) {
  if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, v);
}
__device__ __forceinline__ void sf_offer_max(unsigned long long* p, unsigned long long v) {
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}

// the workgroup's key and the first element of this wavefront's 512; false: nothing to do
__device__ __forceinline__ bool sf_tile(const SfResArgs& A, uint32_t& key, uint32_t& e0) {
  const uint32_t* f = A.first + kFirstSelect * (A.n_keys + 1u);
  key = sf_find_key(f, A.n_keys, wv::wg_index());
  const uint32_t tile = wv::wg_index() - f[key];
  e0 = tile * kSelTile + (wv::wg_thread() >> 6) * (kSelTile / 4u);
  return (uint64_t)tile * kSelTile < A.plan[key].E;
}

__global__ __launch_bounds__(256) void sf_decide_kernel(SfResArgs A) {
  uint32_t key, e0;
  if (!sf_tile(A, key, e0)) return;
  const SfKeyPlan& p = A.plan[key];
  const uint32_t E = p.E, lane = wv::wg_thread() & 63u;
  const uint32_t* __restrict__ known = A.known + p.elem_base;
  const uint32_t* __restrict__ lp = A.lp + p.elem_base;
  const uint32_t* __restrict__ la = A.la + p.elem_base;
  const long long* __restrict__ T = A.op_time ? A.op_time + A.time_off[key] : nullptr;
  const unsigned long long unit = T ? A.unit : 1ull;
  const auto time_of = [&](uint32_t i) -> long long { return T ? T[i] : (long long)i; };
  uint32_t c_lost = 0, c_never = 0, c_stale = 0;
  unsigned long long mn_s = ~0ull, mx_s = 0ull, mn_l = ~0ull, mx_l = 0ull;
  for (uint32_t it = 0; it < kSelTile / 256u; it++) {
    const uint32_t e = e0 + it * 64u + lane;
    const bool in = e < E;
    bool stable = false, lost = false, stale = false;
    if (in) {
      const uint32_t k = known[e], a = la[e], b = lp[e];
      const long long ai = a == kNoneU ? -1ll : (long long)a, bi = b == kNoneU ? -1ll : (long long)b;
      stable = b != kNoneU && ai < bi;
      lost = k != kNoneU && a != kNoneU && bi < ai && (long long)k < ai;
      long long sl = -1ll, ll = -1ll;
      if (stable || lost) {
        const long long tk = k != kNoneU ? time_of(k) : 0ll;
        const uint32_t other = stable ? a : b;
        const long long dt = (other != kNoneU ? time_of(other) + 1ll : 0ll) - tk;
        const unsigned long long lat = dt > 0ll ? (unit == 1ull ? (unsigned long long)dt : (unsigned long long)dt / unit) : 0ull;
        if (stable) {
          sl = (long long)lat; stale = lat > 0ull;
          mn_s = lat < mn_s ? lat : mn_s; mx_s = lat > mx_s ? lat : mx_s;
        } else {
          ll = (long long)lat;
          mn_l = lat < mn_l ? lat : mn_l; mx_l = lat > mx_l ? lat : mx_l;
        }
      }
      A.outcome[p.elem_base + e] = stable ? (uint8_t)TBC_SETFULL_STABLE : (lost ? (uint8_t)TBC_SETFULL_LOST : (uint8_t)TBC_SETFULL_NEVER_READ);
      A.slat[p.elem_base + e] = sl;
      A.llat[p.elem_base + e] = ll;
    }
    c_lost += (uint32_t)__popcll(wv::ballot(lost));
    c_never += (uint32_t)__popcll(wv::ballot(in && !stable && !lost));
    c_stale += (uint32_t)__popcll(wv::ballot(stale));
  }
  mn_s = sf_wave_min64(mn_s); mx_s = sf_wave_max64(mx_s); mn_l = sf_wave_min64(mn_l); mx_l = sf_wave_max64(mx_l);
  if (lane == 0u) {
    SfKeyAcc& a = A.acc[key];
    if (c_lost) atomicAdd(&a.n_lost, c_lost);
    if (c_never) atomicAdd(&a.n_never, c_never);
    if (c_stale) atomicAdd(&a.n_stale, c_stale);
    if (mn_s != ~0ull) { sf_offer_min(&a.min_s, mn_s); sf_offer_max(&a.max_s, mx_s); }
    if (mn_l != ~0ull) { sf_offer_min(&a.min_l, mn_l); sf_offer_max(&a.max_l, mx_l); }
  }
}

// one level of the select, counting: LDS histograms of the workgroup's 2,048 elements, the non-zero bins added to the key's
__global__ __launch_bounds__(256) void sf_select_hist_kernel(SfResArgs A, uint32_t level) {
  uint32_t key, e0;
  if (!sf_tile(A, key, e0)) return;
  const SfKeyPlan& p = A.plan[key];
  const SfKeyAcc& a = A.acc[key];
  const uint32_t E = p.E, lane = wv::wg_thread() & 63u;
  const bool use_s = sf_level_used(a.max_s, level), use_l = sf_level_used(a.max_l, level);
  bool on[kSelTargets];
  unsigned long long hi[kSelTargets];                      // the bits above this level's digit that a value must share with the target
  bool any = false;
#pragma unroll
  for (uint32_t t = 0; t < kSelTargets; t++) {
    uint32_t n, rank;
    sf_target(a, E, t, n, rank);
    on[t] = n != 0u && (t < 4u ? use_s : use_l);
    hi[t] = level < 7u ? A.sel[key * kSelTargets + t].prefix >> (8u * (level + 1u)) : 0ull;
    any = any || on[t];
  }
  if (!any) return;                                        // (uniform: the whole workgroup)
  __shared__ uint32_t s_hist[kSelTargets * kSelBins];
  for (uint32_t i = wv::wg_thread(); i < kSelTargets * kSelBins; i += 256u) s_hist[i] = 0u;
  wv::wg_barrier();
  for (uint32_t it = 0; it < kSelTile / 256u; it++) {
    const uint32_t e = e0 + it * 64u + lane;
    if (e >= E) continue;
    const uint32_t oc = A.outcome[p.elem_base + e];
    if (oc == TBC_SETFULL_NEVER_READ) continue;
    const bool st = oc == TBC_SETFULL_STABLE;
    if (!(st ? use_s : use_l)) continue;
    const unsigned long long v = (unsigned long long)(st ? A.slat : A.llat)[p.elem_base + e];
    const unsigned long long above = level < 7u ? v >> (8u * (level + 1u)) : 0ull;
    const uint32_t digit = (uint32_t)(v >> (8u * level)) & 255u;
#pragma unroll
    for (uint32_t t = 0; t < kSelTargets; t++)
      if (on[t] && (t < 4u) == st && above == hi[t]) wv::lds_add32_wg(&s_hist[t * kSelBins + digit], 1u);
  }
  wv::wg_barrier();
  uint32_t* __restrict__ g = A.hist + (uint64_t)key * (kSelTargets * kSelBins);
  for (uint32_t i = wv::wg_thread(); i < kSelTargets * kSelBins; i += 256u) {
    const uint32_t c = s_hist[i];
    if (c) atomicAdd(&g[i], c);
  }
}

// ... and picking: a workgroup per key, a wavefront per target; lane l holds bins 4l .. 4l + 3
__global__ __launch_bounds__(kSelTargets * 64) void sf_select_pick_kernel(SfResArgs A, uint32_t level) {
  const uint32_t key = wv::wg_index(), t = wv::wg_thread() >> 6, lane = wv::wg_thread() & 63u;
  const SfKeyAcc& a = A.acc[key];
  uint32_t n, rank;
  sf_target(a, A.plan[key].E, t, n, rank);
  SfSel* const s = &A.sel[key * kSelTargets + t];
  // level 7 runs first: the state starts there.  A level none of the key's values reaches (every digit 0) counted nothing and adds nothing.
  if (n == 0u || !sf_level_used(t < 4u ? a.max_s : a.max_l, level)) {
    if (level == 7u && lane == 0u) { s->prefix = 0ull; s->k = rank; s->pad = 0u; }
    return;
  }
  const uint32_t k = level == 7u ? rank : s->k;
  uint4* const g = reinterpret_cast<uint4*>(A.hist + ((uint64_t)key * kSelTargets + t) * kSelBins) + lane;
  const uint4 h = *g;
  *g = make_uint4(0u, 0u, 0u, 0u);
  uint32_t bin = 0u, left = 0u;
  if (!rs_pick(h, lane, k, bin, left)) return;                          // (one lane goes on: the one whose bins hold the rank)
  const unsigned long long prefix = level == 7u ? 0ull : s->prefix;
  s->prefix = prefix | ((unsigned long long)bin << (8u * level));
  s->k = left;
}

// worst-stale: the stale elements above the key's threshold (at most seven where there are more than eight stale, else all of them) are
// appended; those AT the threshold compete for the places left with their element numbers, lowest first: eq[] is kept as the eight
// least numbers offered so far by an exchange per slot (atomicMin leaves the lesser in the slot, the greater is carried on: a number
// is dropped only past eight slots that each held a lesser one).  A wavefront's elements come in ascending order, so it offers its
// first eight at most.
__global__ __launch_bounds__(256) void sf_worst_collect_kernel(SfResArgs A) {
  uint32_t key, e0;
  if (!sf_tile(A, key, e0)) return;
  const SfKeyPlan& p = A.plan[key];
  SfKeyAcc& a = A.acc[key];
  const uint32_t E = p.E, lane = wv::wg_thread() & 63u, n_stale = a.n_stale;
  if (n_stale == 0u) return;
  const bool ties = n_stale > kWorst;
  const unsigned long long thr = ties ? A.sel[key * kSelTargets + 3u].prefix : 0ull;
  uint32_t taken = 0u;
  for (uint32_t it = 0; it < kSelTile / 256u; it++) {
    const uint32_t e = e0 + it * 64u + lane;
    unsigned long long v = 0ull;
    if (e < E && A.outcome[p.elem_base + e] == TBC_SETFULL_STABLE) v = (unsigned long long)A.slat[p.elem_base + e];
    if (v > thr) {
      const uint32_t slot = atomicAdd(&a.n_gt, 1u);
      if (slot < kWorst) a.gt[slot] = e;
    }
    const bool tie = ties && v == thr && v != 0ull;
    const uint64_t who = wv::ballot(tie);
    const uint32_t before = taken + (uint32_t)__popcll(who & ((1ull << lane) - 1ull));
    taken += (uint32_t)__popcll(who);
    if (tie && before < kWorst) {
      uint32_t c = e;
      for (uint32_t j = 0; j < kWorst && c != 0xFFFFFFFFu; j++) { const uint32_t old = atomicMin(&a.eq[j], c); c = old > c ? old : c; }
    }
  }
}

__global__ __launch_bounds__(256) void sf_results_final_kernel(SfResArgs A) {
  const uint32_t key = wv::wg_index() * 256u + wv::wg_thread();
  if (key >= A.n_keys) return;
  const SfKeyPlan& p = A.plan[key];
  const SfKeyAcc& a = A.acc[key];
  const SfSel* s = A.sel + key * kSelTargets;
  tbc_setfull_key_summary o;
  const uint32_t n_stable = p.E - a.n_lost - a.n_never;
  o.attempt_count = p.E; o.stable_count = n_stable; o.lost_count = a.n_lost; o.never_read_count = a.n_never; o.stale_count = a.n_stale;
  o.valid = a.n_lost ? TBC_SETFULL_VALID_FALSE
                     : (n_stable == 0u ? TBC_SETFULL_VALID_UNKNOWN
                                       : (((A.flags & TBC_SETFULL_F_LINEARIZABLE) && a.n_stale) ? TBC_SETFULL_VALID_FALSE : TBC_SETFULL_VALID_TRUE));
  o.stable_q_present = n_stable != 0u; o.lost_q_present = a.n_lost != 0u;
  for (int i = 0; i < 5; i++) { o.stable_q[i] = 0; o.lost_q[i] = 0; }
  if (n_stable) {
    o.stable_q[0] = (int64_t)a.min_s; o.stable_q[1] = (int64_t)s[0].prefix; o.stable_q[2] = (int64_t)s[1].prefix; o.stable_q[3] = (int64_t)s[2].prefix;
    o.stable_q[4] = (int64_t)a.max_s;
  }
  if (a.n_lost) {
    o.lost_q[0] = (int64_t)a.min_l; o.lost_q[1] = (int64_t)s[4].prefix; o.lost_q[2] = (int64_t)s[5].prefix; o.lost_q[3] = (int64_t)s[6].prefix;
    o.lost_q[4] = (int64_t)a.max_l;
  }
  // the worst stale: those above the threshold by (latency descending, element ascending), then the lowest-numbered ones at it
  const uint32_t n_worst = a.n_stale < kWorst ? a.n_stale : kWorst;
  const uint32_t n_gt = a.n_gt < n_worst ? a.n_gt : n_worst;
  uint32_t el[kWorst]; long long lat[kWorst];
  for (uint32_t i = 0; i < kWorst; i++) { el[i] = 0u; lat[i] = 0; }
  for (uint32_t i = 0; i < n_gt; i++) {
    const uint32_t e = a.gt[i];
    const long long v = A.slat[p.elem_base + e];
    uint32_t j = i;
    while (j > 0u && (lat[j - 1u] < v || (lat[j - 1u] == v && el[j - 1u] > e))) { el[j] = el[j - 1u]; lat[j] = lat[j - 1u]; j--; }
    el[j] = e; lat[j] = v;
  }
  if (n_gt < n_worst) {
    uint32_t q[kWorst];
    for (uint32_t i = 0; i < kWorst; i++) {
      const uint32_t e = a.eq[i];
      uint32_t j = i;
      while (j > 0u && q[j - 1u] > e) { q[j] = q[j - 1u]; j--; }
      q[j] = e;
    }
    for (uint32_t i = n_gt; i < n_worst; i++) { el[i] = q[i - n_gt]; lat[i] = (long long)s[3].prefix; }
  }
  o.n_worst = (uint8_t)n_worst;
  for (uint32_t i = 0; i < kWorst; i++) {
    const bool in = i < n_worst && el[i] < p.E;
    o.worst_element[i] = in ? el[i] : 0u;
    o.worst_latency[i] = in ? lat[i] : 0;
    o.worst_known[i] = in ? A.known[p.elem_base + el[i]] : kNoneU;
    o.worst_last_absent[i] = in ? A.la[p.elem_base + el[i]] : kNoneU;
  }
  A.summary[key] = o;
}

}  // namespace
