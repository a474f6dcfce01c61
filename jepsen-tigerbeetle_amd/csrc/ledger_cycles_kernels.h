// ledger_cycles_kernels.h -- tbc_ledger_cycles on the MI355X (gfx950): the kernel bodies.  ledger_cycles.hip compiles them into
// libtbcheck.so; their launches are the four sequences at the end of this file; the host plan is ledger_cycles_plan.h; the rules and
// the reduction are stated in jepsen/ledger.py ("Cycle search", cycles_dense_numpy).  The layout, the sort by (sum, read number) and the
// prefix-maximum / suffix-minimum flag are tbc_ledger_snapshots' own kernels (ledger_snap_kernels.h, lgsn::filter_sequence), run
// first and unchanged; the sort by inv reuses its three sort kernels over other buffers.  Then, in launch order; no kernel holds an
// agent-scope fence, none uses scratch, every grid strides (a kernel of ONE workgroup walks its array in steps of 256):
//
//   cy_sums_kernel        thread = position of the order: the read's sum key stored by read number; the inv sort's keys laid down
//   cy_pmax_kernel        ONE workgroup: the inclusive prefix maximum, over read numbers (= the order of ret), of the sums of U
//   cy_clean_kernel       thread = read: how many reads returned before it was invoked (a binary search of ret), rt-flagged if the
//                         maximum over those is above its own sum; its state bits: partial, core
//   cy_core_scan_kernel   ONE workgroup: the core reads listed ascending (an exclusive sum of the core bits), counted
//   cy_class_scan_kernel  ONE workgroup, along the order: the last clean key before each position (a scan that keeps the later one),
//                         a class starts where that differs; classes numbered by an exclusive sum; per class a read that holds its vector
//   the sort by inv1, 4 passes of 8 bits: sn_hist_kernel, sn_carry_kernel, sn_scatter_kernel
//   cy_rt_scan_kernel     ONE workgroup: prefix maximum of class over read numbers; suffix minimum of class along the inv order
//   cy_desc_kernel        thread = core read: per checked counter an upper-bound and a lower-bound search along the classes' vectors (the
//                         chain is monotone in every counter), the two realtime lookups; s_out and s_in with their monotonic bits as codes:
//                         out_code = 2 (s_out + 1) - mono_out, in_code = 2 (s_in + 1) + mono_in, so that "mediated" is out_code < in_code
//   cy_matrix_kernel      a workgroup per row, lanes over the columns: direct realtime, mediated, direct monotonic (the common
//                         checked counters word by word); a wavefront's 64 bits by one ballot, stored as two words
//   cy_closure_kernel     a workgroup per row, the row in LDS, lanes over the row's words: the OR of the rows the row names; one
//                         changed flag per round
//   cy_comp_kernel        a workgroup per core read: the reads it shares a component with (both bits of the closure), the least of them
//                         its representative; a representative folds its component's lo and hi descriptors and lists itself
//   cy_member_kernel      thread = clean read, the components through LDS in tiles of 64: the one that encloses it
//   cy_labels_kernel      lane = read: scc, cyc_flags; the counts, the first read on a cycle, the greatest size
//   cy_largest_kernel, cy_summary_kernel   the EARLIEST label of the greatest size; the summary (as sn_worst / sn_summary)
#pragma once
#include "wave_env_wg.h"
#include "wg_scan.h"
#include "ledger_cycles_plan.h"
#include "ledger_search.h"
#include "ledger_snap_kernels.h"

namespace {

using lgcy::CyArgs;
using lgcy::kCyNone;

// how many of the ascending a[0 .. n) are below x; how many are at or below x
template <class T>
__device__ __forceinline__ uint32_t cy_count_below(const T* __restrict__ a, uint32_t n, T x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1u; else hi = mid; }
  return lo;
}
template <class T>
__device__ __forceinline__ uint32_t cy_count_upto(const T* __restrict__ a, uint32_t n, T x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a[mid] <= x) lo = mid + 1u; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(256) void cy_sums_kernel(CyArgs A, uint32_t grid) {
  for (uint32_t p = wv::wg_index() * 256u + wv::wg_thread(); p < A.n_reads; p += grid * 256u) {
    A.sumkey[A.sn.sort_perm[0][p]] = A.sn.sort_key[0][p];
    A.ikey[0][p] = A.inv1[p]; A.iperm[0][p] = p;                              // (p as a read number)
  }
}

__global__ __launch_bounds__(256) void cy_pmax_kernel(CyArgs A) {       // (ONE workgroup)
  __shared__ unsigned long long s_val[256];
  const uint32_t t = wv::wg_thread();
  unsigned long long run = 0ull;
  for (uint32_t base = 0; base < A.n_reads; base += 256u) {
    const uint32_t r = base + t;
    const bool in = r < A.n_reads;
    const unsigned long long v = in && A.sn.cand_flag[r] == 0u ? A.sumkey[r] : 0ull;     // (a sum's key is 1 at least: 0 is "none")
    unsigned long long total;
    const unsigned long long ex = wg_scan_excl(v, s_val, t, 0ull, total, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; });
    const unsigned long long upto = ex > v ? ex : v;
    if (in) A.pmax[r] = upto > run ? upto : run;
    run = run > total ? run : total;
  }
}

__global__ __launch_bounds__(256) void cy_clean_kernel(CyArgs A, uint32_t grid) {
  for (uint32_t r = wv::wg_index() * 256u + wv::wg_thread(); r < A.n_reads; r += grid * 256u) {
    const uint32_t flag = A.sn.cand_flag[r], inv1 = A.inv1[r];
    const uint32_t before = inv1 ? cy_count_below(A.ret1, A.n_reads, inv1) : 0u;        // the reads that returned before this one was invoked
    const unsigned long long best = before ? A.pmax[before - 1u] : 0ull;
    const bool clean = flag == 0u && !(best > A.sumkey[r]);
    A.state[r] = ((flag & lgsn::kSnPartial) ? TBC_LEDGER_CYC_PARTIAL : 0u) | (clean ? 0u : TBC_LEDGER_CYC_CORE);
  }
}

__global__ __launch_bounds__(256) void cy_core_scan_kernel(CyArgs A) {  // (ONE workgroup)
  __shared__ uint32_t s_val[256];
  const uint32_t t = wv::wg_thread();
  uint32_t run = 0u;
  for (uint32_t base = 0; base < A.n_reads; base += 256u) {
    const uint32_t r = base + t;
    const bool core = r < A.n_reads && (A.state[r] & TBC_LEDGER_CYC_CORE);
    uint32_t total;
    const uint32_t ex = wg_scan_excl(core ? 1u : 0u, s_val, t, 0u, total, [](uint32_t a, uint32_t b) { return a + b; });
    if (core) { A.core_list[run + ex] = r; A.core_pos[r] = run + ex; }
    run += total;
  }
  if (t == 0u) A.acc->n_core = run;
}

__global__ __launch_bounds__(256) void cy_class_scan_kernel(CyArgs A) { // (ONE workgroup)
  __shared__ unsigned long long s_key[256];
  __shared__ uint32_t s_cnt[256];
  const uint32_t t = wv::wg_thread();
  unsigned long long run_key = 0ull;                                        // the last clean key so far, 0 = none
  uint32_t run = 0u;
  for (uint32_t base = 0; base < A.n_reads; base += 256u) {
    const uint32_t p = base + t;
    const bool in = p < A.n_reads;
    const uint32_t r = in ? A.sn.sort_perm[0][p] : 0u;
    const bool clean = in && !(A.state[r] & TBC_LEDGER_CYC_CORE);
    const unsigned long long key = clean ? A.sn.sort_key[0][p] : 0ull;
    unsigned long long total_key;
    const unsigned long long ex_key = wg_scan_excl(key, s_key, t, 0ull, total_key, [](unsigned long long a, unsigned long long b) { return b ? b : a; });
    const bool head = clean && (ex_key ? ex_key : run_key) != key;
    uint32_t total;
    const uint32_t ex = wg_scan_excl(head ? 1u : 0u, s_cnt, t, 0u, total, [](uint32_t a, uint32_t b) { return a + b; });
    if (in) A.cls1[r] = clean ? run + ex + (head ? 1u : 0u) : 0u;
    if (head) A.cls_rep[run + ex] = r;
    run += total;
    run_key = total_key ? total_key : run_key;
  }
  if (t == 0u) A.acc->n_cls = run;
}

__global__ __launch_bounds__(256) void cy_rt_scan_kernel(CyArgs A) {    // (ONE workgroup)
  __shared__ uint32_t s_val[256];
  const uint32_t t = wv::wg_thread(), R = A.n_reads;
  uint32_t run_max = 0u, run_min = kCyNone;
  for (uint32_t base = 0; base < R; base += 256u) {
    const uint32_t r = base + t;
    const bool in = r < R;
    const uint32_t up = in ? A.cls1[r] : 0u;                                // read numbers ascending: the prefix maximum
    const uint32_t q = in ? R - 1u - r : 0u;                                // the inv order descending: the suffix minimum
    const uint32_t c = in ? A.cls1[A.iperm[0][q]] : 0u;
    const uint32_t down = c ? c : kCyNone;
    uint32_t total_max, total_min;
    const uint32_t ex_max = wg_scan_excl(up, s_val, t, 0u, total_max, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
    const uint32_t ex_min = wg_scan_excl(down, s_val, t, kCyNone, total_min, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
    if (in) {
      const uint32_t mx = ex_max > up ? ex_max : up, mn = ex_min < down ? ex_min : down;
      A.pcls[r] = mx > run_max ? mx : run_max;
      A.scls[q] = mn < run_min ? mn : run_min;
    }
    run_max = run_max > total_max ? run_max : total_max; run_min = run_min < total_min ? run_min : total_min;
  }
}

__global__ __launch_bounds__(256) void cy_desc_kernel(CyArgs A, uint32_t grid) {
  const uint32_t n_cls = A.acc->n_cls, C = A.sn.n_class, R = A.n_reads;
  for (uint32_t i = wv::wg_index() * 256u + wv::wg_thread(); i < A.n_core; i += grid * 256u) {
    const uint32_t P = A.core_list[i];
    const unsigned long long* const row = A.sn.val + (unsigned long long)P * C;
    const uint32_t* const chk = A.sn.chk + (unsigned long long)P * A.sn.n_words;
    uint32_t mono_out = n_cls, mono_in1 = 0u;                               // the least class above P somewhere; the classes below P somewhere
    for (uint32_t c = 0; c < C; c++) {
      if (!sn_bit(chk, c)) continue;
      const unsigned long long v = row[c];
      uint32_t lo = 0u, hi = n_cls;
      while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (A.sn.val[(unsigned long long)A.cls_rep[mid] * C + c] <= v) lo = mid + 1u; else hi = mid; }
      mono_out = lo < mono_out ? lo : mono_out;
      lo = 0u; hi = n_cls;
      while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (A.sn.val[(unsigned long long)A.cls_rep[mid] * C + c] < v) lo = mid + 1u; else hi = mid; }
      mono_in1 = lo > mono_in1 ? lo : mono_in1;
    }
    const uint32_t inf = n_cls + 1u, mono_out1 = mono_out + 1u;
    const uint32_t inv1 = A.inv1[P], ret1 = A.ret1[P];
    const uint32_t q = cy_count_upto(A.ikey[0], R, (unsigned long long)ret1);            // the first read invoked after P returned
    uint32_t rt_out1 = q < R ? A.scls[q] : kCyNone;
    rt_out1 = rt_out1 == kCyNone ? inf : rt_out1;
    const uint32_t before = inv1 ? cy_count_below(A.ret1, R, inv1) : 0u;
    const uint32_t rt_in1 = before ? A.pcls[before - 1u] : 0u;
    const uint32_t s_out1 = mono_out1 < rt_out1 ? mono_out1 : rt_out1, s_in1 = mono_in1 > rt_in1 ? mono_in1 : rt_in1;
    const uint32_t m_out = mono_out1 == s_out1 && s_out1 < inf, m_in = mono_in1 == s_in1 && s_in1 > 0u;
    A.out_code[i] = 2u * s_out1 - m_out; A.in_code[i] = 2u * s_in1 + m_in;
    A.cinv[i] = inv1; A.cret[i] = ret1;
  }
}

__global__ __launch_bounds__(256) void cy_matrix_kernel(CyArgs A, uint32_t grid) {
  const uint32_t t = wv::wg_thread(), lane = t & 63u, m = A.n_core, W = A.n_words, C = A.sn.n_class, CW = A.sn.n_words;
  const uint32_t m64 = (m + 63u) & ~63u;
  for (uint32_t i = wv::wg_index(); i < m; i += grid) {
    const uint32_t Pi = A.core_list[i], ret_i = A.cret[i], out_i = A.out_code[i];
    const unsigned long long* const row_i = A.sn.val + (unsigned long long)Pi * C;
    const uint32_t* const chk_i = A.sn.chk + (unsigned long long)Pi * CW;
    // (whole wavefronts: every lane of one makes the same trips, the ballot is wavefront-uniform)
    for (uint32_t j0 = t & ~63u; j0 < m64; j0 += 256u) {
      const uint32_t j = j0 + lane;
      bool edge = false;
      if (j < m) {
        edge = ret_i < A.cinv[j] || out_i < A.in_code[j];
        if (!edge) {
          const uint32_t Pj = A.core_list[j];
          const unsigned long long* const row_j = A.sn.val + (unsigned long long)Pj * C;
          const uint32_t* const chk_j = A.sn.chk + (unsigned long long)Pj * CW;
          for (uint32_t w = 0; w < CW && !edge; w++)
            for (uint32_t both = chk_i[w] & chk_j[w]; both && !edge; both &= both - 1u) {
              const uint32_t c = 32u * w + (uint32_t)__builtin_ctz(both);
              edge = row_i[c] < row_j[c];
            }
        }
      }
      const unsigned long long b = wv::ballot(edge);
      if (lane == 0u) {
        const uint32_t w = j0 >> 5;
        if (w < W) A.mat[0][(size_t)i * W + w] = (uint32_t)b;
        if (w + 1u < W) A.mat[0][(size_t)i * W + w + 1u] = (uint32_t)(b >> 32);
      }
    }
  }
}

__global__ __launch_bounds__(256) void cy_closure_kernel(CyArgs A, uint32_t round, uint32_t grid) {
  __shared__ uint32_t s_row[TBC_LEDGER_CYCLES_MAX_CORE / 32u];
  const uint32_t t = wv::wg_thread(), m = A.n_core, W = A.n_words;
  const uint32_t* __restrict__ src = A.mat[round & 1u];
  uint32_t* __restrict__ dst = A.mat[(round & 1u) ^ 1u];
  bool changed = false;
  for (uint32_t i = wv::wg_index(); i < m; i += grid) {
    for (uint32_t w = t; w < W; w += 256u) s_row[w] = src[(size_t)i * W + w];
    wv::wg_barrier();
    for (uint32_t w = t; w < W; w += 256u) {
      uint32_t acc = s_row[w];
      for (uint32_t kw = 0; kw < W; kw++)
        for (uint32_t bits = s_row[kw]; bits; bits &= bits - 1u) acc |= src[(size_t)(32u * kw + (uint32_t)__builtin_ctz(bits)) * W + w];
      dst[(size_t)i * W + w] = acc;
      changed = changed || acc != s_row[w];
    }
    wv::wg_barrier();                                                       // (the row has been read before the next one replaces it)
  }
  if (changed) atomicOr(&A.acc->changed[round], 1u);
}

__device__ __forceinline__ bool cy_mat_bit(const uint32_t* __restrict__ M, uint32_t W, uint32_t i, uint32_t j) { return (M[(size_t)i * W + (j >> 5)] >> (j & 31u)) & 1u; }

__global__ __launch_bounds__(256) void cy_comp_kernel(CyArgs A, uint32_t side, uint32_t grid) {
  __shared__ uint32_t s_rep, s_cnt, s_lo, s_hi, s_lo_ret, s_hi_inv;
  const uint32_t t = wv::wg_thread(), m = A.n_core, W = A.n_words;
  const uint32_t* __restrict__ M = A.mat[side];
  for (uint32_t i = wv::wg_index(); i < m; i += grid) {
    if (t == 0u) { s_rep = kCyNone; s_cnt = 0u; s_lo = kCyNone; s_hi = 0u; s_lo_ret = kCyNone; s_hi_inv = 0u; }
    wv::wg_barrier();
    uint32_t rep = kCyNone, cnt = 0u, lo = kCyNone, hi = 0u;
    for (uint32_t j = t; j < m; j += 256u) {
      if (j != i && !(cy_mat_bit(M, W, i, j) && cy_mat_bit(M, W, j, i))) continue;
      rep = j < rep ? j : rep; cnt++;
      const uint32_t o = A.out_code[j], n = A.in_code[j];
      lo = o < lo ? o : lo; hi = n > hi ? n : hi;
    }
    if (cnt) { atomicMin(&s_rep, rep); atomicAdd(&s_cnt, cnt); atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    wv::wg_barrier();
    const uint32_t rep_i = s_rep;                                           // (i itself is a member: never none)
    if (rep_i == i) {                                                       // (uniform) the representative folds the component's descriptors
      const uint32_t lo_s = (s_lo + 1u) >> 1, hi_s = s_hi >> 1;
      uint32_t lo_ret = kCyNone, hi_inv = 0u;
      for (uint32_t j = t; j < m; j += 256u) {
        if (j != i && !(cy_mat_bit(M, W, i, j) && cy_mat_bit(M, W, j, i))) continue;
        if (((A.out_code[j] + 1u) >> 1) == lo_s) lo_ret = A.cret[j] < lo_ret ? A.cret[j] : lo_ret;
        if ((A.in_code[j] >> 1) == hi_s) hi_inv = A.cinv[j] > hi_inv ? A.cinv[j] : hi_inv;
      }
      if (lo_ret != kCyNone) atomicMin(&s_lo_ret, lo_ret);
      if (hi_inv) atomicMax(&s_hi_inv, hi_inv);
      wv::wg_barrier();
      if (t == 0u) {
        A.k_lo_code[i] = s_lo; A.k_lo_ret[i] = s_lo_ret; A.k_hi_code[i] = s_hi; A.k_hi_inv[i] = s_hi_inv;
        A.k_size[i] = s_cnt; A.k_label[i] = A.core_list[i];
        A.rep_list[atomicAdd(&A.acc->n_reps, 1u)] = i;
      }
    }
    if (t == 0u) A.rep[i] = rep_i;
    wv::wg_barrier();                                                       // (the folds have been read before the next row resets them)
  }
}

__global__ __launch_bounds__(256) void cy_member_kernel(CyArgs A, uint32_t grid) {
  constexpr uint32_t T = lgcy::kCyTile;
  __shared__ uint32_t s_lo[T], s_lo_ret[T], s_hi[T], s_hi_inv[T], s_k[T];
  const uint32_t t = wv::wg_thread(), R = A.n_reads, n_reps = A.acc->n_reps;
  // (whole workgroups: every thread of one makes the same trips, the barriers are uniform)
  for (uint32_t base = wv::wg_index() * 256u; base < R; base += grid * 256u) {
    const uint32_t r = base + t;
    const uint32_t c1 = r < R ? A.cls1[r] : 0u;                             // (0: no clean read)
    const uint32_t inv1 = r < R ? A.inv1[r] : 0u, ret1 = r < R ? A.ret1[r] : 0u;
    uint32_t found = kCyNone;
    for (uint32_t e0 = 0; e0 < n_reps; e0 += T) {
      wv::wg_barrier();                                                     // (the tile before has been read)
      if (t < T && e0 + t < n_reps) {
        const uint32_t k = A.rep_list[e0 + t];
        s_k[t] = k; s_lo[t] = A.k_lo_code[k]; s_lo_ret[t] = A.k_lo_ret[k]; s_hi[t] = A.k_hi_code[k]; s_hi_inv[t] = A.k_hi_inv[k];
      }
      wv::wg_barrier();
      const uint32_t n = n_reps - e0 < T ? n_reps - e0 : T;
      for (uint32_t e = 0; c1 && e < n; e++) {
        const uint32_t lo_s = (s_lo[e] + 1u) >> 1, hi_s = s_hi[e] >> 1;
        const bool above = c1 > lo_s || (c1 == lo_s && ((s_lo[e] & 1u) || inv1 > s_lo_ret[e]));
        const bool below = c1 < hi_s || (c1 == hi_s && ((s_hi[e] & 1u) || ret1 < s_hi_inv[e]));
        if (above && below) found = s_k[e];
      }
    }
    if (r < R) {
      A.member_of[r] = found;
      if (found != kCyNone) { atomicMin(&A.k_label[found], r); atomicAdd(&A.k_size[found], 1u); }
    }
  }
}

// the component of read r as its representative's place in the core's list, none if r is on no cycle
__device__ __forceinline__ uint32_t cy_comp_of(const CyArgs& A, uint32_t r) {
  if (!A.n_core) return kCyNone;
  if (A.state[r] & TBC_LEDGER_CYC_CORE) {
    const uint32_t k = A.rep[A.core_pos[r]];
    return A.k_size[k] >= 2u ? k : kCyNone;
  }
  return A.member_of[r];
}

__global__ __launch_bounds__(256) void cy_labels_kernel(CyArgs A, uint32_t grid) {
  const uint32_t lane = wv::wg_thread() & 63u;
  // (whole wavefronts: every lane of one makes the same trips, the ballots are wavefront-uniform)
  for (uint32_t wave_r0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_r0 < A.n_reads; wave_r0 += grid * 256u) {
    const uint32_t r = wave_r0 + lane;
    const bool in = r < A.n_reads;
    const uint32_t k = in ? cy_comp_of(A, r) : kCyNone;
    const bool on = k != kCyNone;
    const uint32_t label = on ? A.k_label[k] : kCyNone;
    if (in) { A.scc[r] = label; A.cyc_flags[r] = (uint8_t)(A.state[r] | (on ? TBC_LEDGER_CYC_ON_CYCLE : 0u)); }
    const unsigned long long b = wv::ballot(on), heads = wv::ballot(on && label == r);
    if (!b) continue;                                                       // (uniform)
    if (lane == 0u) {
      atomicAdd(&A.acc->n_on_cycle, (uint32_t)__popcll(b));
      atomicMin(&A.acc->first, wave_r0 + (uint32_t)__builtin_ctzll(b));
      if (heads) atomicAdd(&A.acc->n_components, (uint32_t)__popcll(heads));
    }
    if (on && label == r) atomicMax(&A.acc->largest_size, A.k_size[k]);
  }
}

__global__ __launch_bounds__(256) void cy_largest_kernel(CyArgs A, uint32_t grid) {
  for (uint32_t r = wv::wg_index() * 256u + wv::wg_thread(); r < A.n_reads; r += grid * 256u) {
    const uint32_t k = cy_comp_of(A, r);
    if (k != kCyNone && A.k_label[k] == r && A.k_size[k] == A.acc->largest_size) atomicMin(&A.acc->largest, r);
  }
}

__global__ __launch_bounds__(64) void cy_summary_kernel(CyArgs A, uint32_t rounds) {
  if (wv::wg_thread() != 0u) return;
  const lgcy::CyAcc& a = *A.acc;
  tbc_ledger_cycles_summary s{};
  s.read_count = A.n_reads; s.n_partial = A.sn.acc->n_partial; s.n_core = a.n_core; s.valid = a.n_on_cycle == 0u;
  s.n_on_cycle = a.n_on_cycle; s.n_components = a.n_components; s.first = a.first; s.largest = a.largest;
  s.largest_size = a.largest_size; s.closure_rounds = rounds; s.bad_values = A.sn.acc->bad_values; s.n_checked = A.sn.acc->n_checked;
  *A.summary = s;
}

}  // namespace

namespace lgcy {

// The kernels of the call in order, over a launcher (oneshot_plan.h): THE statement of the launches -- the library runs them over a
// stream (ledger_cycles.hip), the tests over the emulator and over a recorder.  Four sequences, because the host reads the core's size
// after the first (it allocates the matrices, or refuses) and the changed flag after every round.  A kernel with nothing to do is not
// launched: no reads -- only the summary; no core read -- no class, no descriptor, no matrix, no closure, no component, no member.
constexpr uint32_t kCyInvDigits = 4;                  // the inv sort's passes: 8 bits of the 32-bit inv1 each (an even number: the order ends in [0])

template <class Launcher>
void prepare_sequence(Launcher& go, const CyArgs& A) {
  lgsn::filter_sequence(go, A.sn);
  if (!A.n_reads) return;
  const uint32_t grid = lgsn::grid_of(go, A.n_reads, 256u, 16384u);
  go.launch(cy_sums_kernel, grid, 256u, A, grid);
  go.launch(cy_pmax_kernel, 1u, 256u, A);
  go.launch(cy_clean_kernel, grid, 256u, A, grid);
  go.launch(cy_core_scan_kernel, 1u, 256u, A);
}

template <class Launcher>
void describe_sequence(Launcher& go, const CyArgs& A) {
  if (!A.n_core) return;
  go.launch(cy_class_scan_kernel, 1u, 256u, A);
  lgsn::SnArgs B = A.sn;                                                    // the snapshot sort's kernels over the inv sort's buffers
  for (int k = 0; k < 2; k++) { B.sort_key[k] = A.ikey[k]; B.sort_perm[k] = A.iperm[k]; }
  const uint32_t grid_sort = go.grid(B.sort_chunks, lgsn::kSnSortChunksMax);
  for (uint32_t pass = 0; pass < kCyInvDigits; pass++) {
    go.launch(sn_hist_kernel, grid_sort, 64u, B, pass, grid_sort);
    go.launch(sn_carry_kernel, 1u, 256u, B);
    go.launch(sn_scatter_kernel, grid_sort, 64u, B, pass, grid_sort);
  }
  go.launch(cy_rt_scan_kernel, 1u, 256u, A);
  const uint32_t grid_core = lgsn::grid_of(go, A.n_core, 256u, 16384u);
  go.launch(cy_desc_kernel, grid_core, 256u, A, grid_core);
  const uint32_t grid_rows = go.grid(A.n_core, 16384u);
  go.launch(cy_matrix_kernel, grid_rows, 256u, A, grid_rows);
}

template <class Launcher>
void round_sequence(Launcher& go, const CyArgs& A, uint32_t round) {
  const uint32_t grid_rows = go.grid(A.n_core, 16384u);
  go.launch(cy_closure_kernel, grid_rows, 256u, A, round, grid_rows);
}

template <class Launcher>
void finish_sequence(Launcher& go, const CyArgs& A, uint32_t final_side, uint32_t rounds) {
  if (A.n_reads) {
    const uint32_t grid = lgsn::grid_of(go, A.n_reads, 256u, 16384u);
    if (A.n_core) {
      const uint32_t grid_rows = go.grid(A.n_core, 16384u);
      go.launch(cy_comp_kernel, grid_rows, 256u, A, final_side, grid_rows);
      go.launch(cy_member_kernel, grid, 256u, A, grid);
    }
    go.launch(cy_labels_kernel, grid, 256u, A, grid);
    go.launch(cy_largest_kernel, grid, 256u, A, grid);
  }
  go.launch(cy_summary_kernel, 1u, 64u, A, rounds);
}

}  // namespace lgcy
