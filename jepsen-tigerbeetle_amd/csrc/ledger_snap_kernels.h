// ledger_snap_kernels.h -- tbc_ledger_snapshots on the MI355X (gfx950): the kernel bodies.  ledger_snap.hip compiles them into
// libtbcheck.so; their launches are lgsn::filter_sequence and lgsn::rest_sequence at the end of this file; the host plan (the reads'
// rows, the gathered columns, the chunks, the arena) is ledger_snap_plan.h;
// the rules are stated in jepsen/ledger.py ("Snapshot order").  A read is a dense ROW of C = 2 x n_accounts counters as
// order-preserving keys (lg_key) with a bit per counter that says whether the read checks it.  The pairwise rule is O(R^2 C); a valid
// history never pays it: for complete reads i before j in the order of (sum, read number), skewed(i, j) <=> some v_i[c] > v_j[c], so an
// exclusive prefix maximum and an exclusive suffix minimum per counter along that order FLAG exactly the complete reads skewed with a
// complete read.  Those and the partial reads are the CANDIDATES; every skewed pair has one in it.  In launch order; no kernel holds an
// agent-scope fence, none uses scratch, every grid strides:
//
//   sn_layout_kernel        a wavefront per read, four to a workgroup: lane = micro-op, its account's number by a binary search of the sorted accounts (in LDS
//                           up to kLgAcctLds), the two keys stored at counters 2k and 2k + 1 (k the account's position in the caller's
//                           list), the checked bits OR-ed in.  Per read the checked count, the sum (the sort's key; 0 for a partial read,
//                           whose place in the order does not matter) and the sum of |v|, saturating: 2^63 or more is a bad value.
//   the sort, 8 passes of 8 bits, least significant first, each a STABLE PARTITION BY DIGIT over chunks of whole wavefronts:
//     sn_hist_kernel        a wavefront per chunk: lanes of one digit found by 8 ballots, the digit's first lane adds their number in LDS; the
//                           chunk's 256 counts stored
//     sn_carry_kernel       ONE workgroup, thread = digit: its column of the counts summed exclusively down the chunks (256 at most), then
//                           the digits' totals scanned (wg_scan.h): where each digit's run starts
//     sn_scatter_kernel     per chunk again: run start + carried count + rank among the step's lanes of the digit
//   the scan, along the sorted order in chunks of scan_rows reads, a thread per (chunk, counter):
//     sn_extremes_kernel    the chunk's maximum and minimum over its complete reads
//     sn_scan_carry_kernel  a workgroup per counter: exclusive prefix maximum and exclusive suffix minimum over the chunks, 256 a step
//     sn_flag_kernel        the chunk walked forwards under the running maximum and backwards under the running minimum: a complete read
//                           above the one or below the other is flagged
//   sn_compact_kernel       lane = read: the candidates' read numbers listed (ballot, one atomic per wavefront), counted
//   sn_pair_kernel          (only with candidates.)  thread = candidate, its row in registers kSnPairK counters at a time as (lo, hi) keys
//                           -- an unchecked counter is (all ones, 0), which compares false both ways --; every read goes through LDS in
//                           tiles of 64, each read broadcast to all lanes, its unchecked counters masked by its bits.  A candidate counts its
//                           partners and keeps the least; a partner that is no candidate gets an atomic add and an atomic min
//   sn_keys_kernel          lane = read: skew_key against skew_first, the flags
//   sn_count_kernel, sn_worst_kernel, sn_summary_kernel   as rt_count / rt_worst / rt_summary: count, first, last, the greatest count and
//                           the EARLIEST read that holds it, the pairs
// Ballots, lane reads, barriers and index / thread go through wave_env.h / wave_env_wg.h; the atomics are plain HIP, which
// tests/emu/oneshot_emu.h states for the host emulator -- these very kernels run there lane by lane.
#pragma once
#include "wave_env_wg.h"
#include "wg_scan.h"
#include "ledger_snap_plan.h"
#include "ledger_search.h"

namespace {

using lgsn::SnArgs;
using lgsn::kSnNone;

__device__ __forceinline__ unsigned long long sn_abs(long long v) { return v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v; }
__device__ __forceinline__ unsigned long long sn_sat_add(unsigned long long a, unsigned long long b) { return a + b < a ? ~0ull : a + b; }
__device__ __forceinline__ bool sn_bit(const uint32_t* __restrict__ words, uint32_t c) { return (words[c >> 5] >> (c & 31u)) & 1u; }

__global__ __launch_bounds__(256) void sn_layout_kernel(SnArgs A, uint32_t grid) {
  __shared__ long long s_acct[lg::kLgAcctLds];
  __shared__ unsigned long long s_sum[256], s_mag[256];
  __shared__ uint32_t s_cnt[256];
  const uint32_t t = wv::wg_thread(), lane = t & 63u, w0 = t & ~63u;       // (a wavefront's own 64 words of each array)
  const bool acct_lds = A.n_accounts <= lg::kLgAcctLds;
  if (acct_lds) for (uint32_t i = t; i < A.n_accounts; i += 256u) s_acct[i] = A.accounts[i];
  wv::wg_barrier();
  const long long* const acct = acct_lds ? s_acct : A.accounts;
  uint32_t n_partial = 0, bad = 0;
  unsigned long long n_checked = 0;
  // (whole wavefronts: every lane of one makes the same trips, the barriers are the wavefront's own)
  for (uint32_t r = wv::wg_index() * 4u + (t >> 6); r < A.n_reads; r += grid * 4u) {
    const unsigned long long lo = A.row_cum[r], hi = A.row_cum[r + 1u];
    unsigned long long sum = 0ull, mag = 0ull;
    uint32_t cnt = 0;
    for (unsigned long long m = lo + lane; m < hi; m += 64u) {
      const long long id = A.mop_id[m], va = A.mop_a[m], vb = A.mop_b[m];   // (four loads in flight before the search)
      const uint32_t a = (A.mop_flags[m] & TBC_LEDGER_M_NIL) ? kSnNone : lg_account_no(acct, A.n_accounts, id);
      if (a == kSnNone) continue;
      const uint32_t c = 2u * A.acct_pos[a];
      unsigned long long* const row = A.val + (unsigned long long)r * A.n_class;
      row[c] = lg_key(va); row[c + 1u] = lg_key(vb);
      atomicOr(&A.chk[(unsigned long long)r * A.n_words + (c >> 5)], 3u << (c & 31u));
      sum += (unsigned long long)va + (unsigned long long)vb;
      mag = sn_sat_add(sn_sat_add(mag, sn_abs(va)), sn_abs(vb));
      cnt++;
    }
    s_sum[t] = sum; s_mag[t] = mag; s_cnt[t] = cnt;
    WV_NOUNROLL
    for (uint32_t d = 32u; d; d >>= 1) {                                     // the lanes' shares folded in halves
      wv::barrier();
      if (lane < d) { s_sum[t] += s_sum[t + d]; s_mag[t] = sn_sat_add(s_mag[t], s_mag[t + d]); s_cnt[t] += s_cnt[t + d]; }
    }
    if (lane == 0u) {
      sum = s_sum[w0]; mag = s_mag[w0]; cnt = s_cnt[w0];
      const bool complete = cnt == A.n_accounts;
      A.sort_key[0][r] = complete ? lg_key((long long)sum) : 0ull;
      A.sort_perm[0][r] = r;
      if (!complete) { A.cand_flag[r] = lgsn::kSnPartial; n_partial++; }
      n_checked += cnt;
      bad += mag >= (1ull << 63);
    }
    wv::barrier();
  }
  if (lane == 0u) {
    if (n_partial) atomicAdd(&A.acc->n_partial, n_partial);
    if (bad) atomicAdd(&A.acc->bad_values, bad);
    if (n_checked) atomicAdd(&A.acc->n_checked, n_checked);
  }
}

// ---- the sort

// the lanes that are `in` and hold this lane's digit (called by whole wavefronts)
__device__ __forceinline__ unsigned long long sn_match(bool in, uint32_t digit) {
  unsigned long long m = wv::ballot(in);
  for (uint32_t b = 0; b < 8u; b++) {
    const bool one = ((digit >> b) & 1u) != 0u;
    const unsigned long long with = wv::ballot(in && one);
    m &= one ? with : ~with;
  }
  return m;
}

__global__ __launch_bounds__(64) void sn_hist_kernel(SnArgs A, uint32_t pass, uint32_t grid) {
  __shared__ uint32_t s_hist[256];
  const uint32_t lane = wv::wg_thread();
  const unsigned long long* __restrict__ key = A.sort_key[pass & 1u];
  for (uint32_t g = wv::wg_index(); g < A.sort_chunks; g += grid) {
    for (uint32_t k = lane; k < 256u; k += 64u) s_hist[k] = 0u;
    wv::barrier();
    const uint32_t lo = g * A.sort_chunk_entries, hi = lo + A.sort_chunk_entries < A.n_reads ? lo + A.sort_chunk_entries : A.n_reads;
    for (uint32_t base = lo; base < hi; base += 64u) {
      const uint32_t e = base + lane;
      const bool in = e < hi;
      const uint32_t digit = in ? (uint32_t)(key[e] >> (8u * pass)) & 255u : 0u;
      const unsigned long long m = sn_match(in, digit);
      if (in && lane == (uint32_t)__builtin_ctzll(m)) wv::lds_add32(&s_hist[digit], (uint32_t)__popcll(m));
    }
    wv::barrier();
    for (uint32_t k = lane; k < 256u; k += 64u) A.hist[(unsigned long long)g * 256u + k] = s_hist[k];
    wv::barrier();
  }
}

__global__ __launch_bounds__(256) void sn_carry_kernel(SnArgs A) {    // (ONE workgroup, thread = digit)
  __shared__ uint32_t s_scan[256];
  const uint32_t t = wv::wg_thread();
  uint32_t run = 0;
  for (uint32_t g0 = 0; g0 < A.sort_chunks; g0 += 16u) {                    // the digit's column of the counts, exclusive, down the chunks:
    uint32_t n[16];                                                         // 16 loads in flight, then their running sums stored
    WV_UNROLL
    for (uint32_t k = 0; k < 16u; k++) n[k] = g0 + k < A.sort_chunks ? A.hist[(unsigned long long)(g0 + k) * 256u + t] : 0u;
    WV_UNROLL
    for (uint32_t k = 0; k < 16u; k++) {
      if (g0 + k < A.sort_chunks) A.hist[(unsigned long long)(g0 + k) * 256u + t] = run;
      run += n[k];
    }
  }
  uint32_t total;
  A.off[t] = wg_scan_excl(run, s_scan, t, 0u, total, [](uint32_t a, uint32_t b) { return a + b; });   // where the digit's run starts
}

__global__ __launch_bounds__(64) void sn_scatter_kernel(SnArgs A, uint32_t pass, uint32_t grid) {
  __shared__ uint32_t s_base[256];
  const uint32_t lane = wv::wg_thread();
  const unsigned long long* __restrict__ key = A.sort_key[pass & 1u];
  const uint32_t* __restrict__ perm = A.sort_perm[pass & 1u];
  unsigned long long* __restrict__ key_out = A.sort_key[(pass & 1u) ^ 1u];
  uint32_t* __restrict__ perm_out = A.sort_perm[(pass & 1u) ^ 1u];
  const unsigned long long below = (2ull << lane) - 1ull;                   // the lanes at or below this one
  for (uint32_t g = wv::wg_index(); g < A.sort_chunks; g += grid) {
    for (uint32_t k = lane; k < 256u; k += 64u) s_base[k] = A.off[k] + A.hist[(unsigned long long)g * 256u + k];
    wv::barrier();
    const uint32_t lo = g * A.sort_chunk_entries, hi = lo + A.sort_chunk_entries < A.n_reads ? lo + A.sort_chunk_entries : A.n_reads;
    for (uint32_t base = lo; base < hi; base += 64u) {
      const uint32_t e = base + lane;
      const bool in = e < hi;
      const unsigned long long k = in ? key[e] : 0ull;
      const uint32_t digit = (uint32_t)(k >> (8u * pass)) & 255u;
      const unsigned long long m = sn_match(in, digit);
      const uint32_t at = in ? s_base[digit] + (uint32_t)__popcll(m & below) - 1u : 0u;
      wv::barrier();                                                        // (every lane has read its base before a leader moves it)
      if (in && lane == (uint32_t)__builtin_ctzll(m)) wv::lds_add32(&s_base[digit], (uint32_t)__popcll(m));
      wv::barrier();
      if (in) { key_out[at] = k; perm_out[at] = perm[e]; }
    }
    wv::barrier();
  }
}

// ---- the scan along the sorted order (sort_perm[0])

__global__ __launch_bounds__(256) void sn_extremes_kernel(SnArgs A, uint32_t grid) {
  const uint32_t* __restrict__ perm = A.sort_perm[0];
  const unsigned long long n = (unsigned long long)A.scan_chunks * A.n_class;
  for (unsigned long long q = (unsigned long long)wv::wg_index() * 256u + wv::wg_thread(); q < n; q += (unsigned long long)grid * 256u) {
    const uint32_t g = (uint32_t)(q / A.n_class), c = (uint32_t)(q % A.n_class);
    const uint32_t lo = g * A.scan_rows, hi = lo + A.scan_rows < A.n_reads ? lo + A.scan_rows : A.n_reads;
    unsigned long long mx = 0ull, mn = ~0ull;
    for (uint32_t p = lo; p < hi; p++) {
      const uint32_t r = perm[p];
      if (A.cand_flag[r] & lgsn::kSnPartial) continue;
      const unsigned long long v = A.val[(unsigned long long)r * A.n_class + c];
      mx = v > mx ? v : mx; mn = v < mn ? v : mn;
    }
    A.cmax[q] = mx; A.cmin[q] = mn;
  }
}

__global__ __launch_bounds__(256) void sn_scan_carry_kernel(SnArgs A, uint32_t grid) {
  __shared__ unsigned long long s_val[256];
  const uint32_t t = wv::wg_thread(), G = A.scan_chunks;
  for (uint32_t c = wv::wg_index(); c < A.n_class; c += grid) {
    unsigned long long run_max = 0ull, run_min = ~0ull;
    for (uint32_t g0 = 0; g0 < G; g0 += 256u) {
      const bool in = g0 + t < G;
      const unsigned long long up = (unsigned long long)(g0 + t) * A.n_class + c;               // chunks ascending: the prefix maximum
      const unsigned long long down = in ? (unsigned long long)(G - 1u - (g0 + t)) * A.n_class + c : 0ull;   // descending: the suffix minimum
      unsigned long long total_max, total_min;
      const unsigned long long ex_max = wg_scan_excl(in ? A.cmax[up] : 0ull, s_val, t, 0ull, total_max, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; });
      const unsigned long long ex_min = wg_scan_excl(in ? A.cmin[down] : ~0ull, s_val, t, ~0ull, total_min, [](unsigned long long a, unsigned long long b) { return a < b ? a : b; });
      if (in) { A.cmax[up] = run_max > ex_max ? run_max : ex_max; A.cmin[down] = run_min < ex_min ? run_min : ex_min; }
      run_max = run_max > total_max ? run_max : total_max; run_min = run_min < total_min ? run_min : total_min;
    }
  }
}

__global__ __launch_bounds__(256) void sn_flag_kernel(SnArgs A, uint32_t grid) {
  const uint32_t* __restrict__ perm = A.sort_perm[0];
  const unsigned long long n = (unsigned long long)A.scan_chunks * A.n_class;
  for (unsigned long long q = (unsigned long long)wv::wg_index() * 256u + wv::wg_thread(); q < n; q += (unsigned long long)grid * 256u) {
    const uint32_t g = (uint32_t)(q / A.n_class), c = (uint32_t)(q % A.n_class);
    const uint32_t lo = g * A.scan_rows, hi = lo + A.scan_rows < A.n_reads ? lo + A.scan_rows : A.n_reads;
    unsigned long long run = A.cmax[q];
    for (uint32_t p = lo; p < hi; p++) {                                     // some earlier complete read is above this one on c
      const uint32_t r = perm[p];
      if (A.cand_flag[r] & lgsn::kSnPartial) continue;
      const unsigned long long v = A.val[(unsigned long long)r * A.n_class + c];
      if (run > v) atomicOr(&A.cand_flag[r], (uint32_t)lgsn::kSnFlagged);
      run = v > run ? v : run;
    }
    run = A.cmin[q];
    for (uint32_t p = hi; p > lo; p--) {                                     // some later complete read is below this one on c
      const uint32_t r = perm[p - 1u];
      if (A.cand_flag[r] & lgsn::kSnPartial) continue;
      const unsigned long long v = A.val[(unsigned long long)r * A.n_class + c];
      if (run < v) atomicOr(&A.cand_flag[r], (uint32_t)lgsn::kSnFlagged);
      run = v < run ? v : run;
    }
  }
}

__global__ __launch_bounds__(256) void sn_compact_kernel(SnArgs A, uint32_t grid) {
  const uint32_t lane = wv::wg_thread() & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  // (whole wavefronts: every lane of one makes the same trips, the ballot is wavefront-uniform)
  for (uint32_t wave_r0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_r0 < A.n_reads; wave_r0 += grid * 256u) {
    const uint32_t r = wave_r0 + lane;
    const bool cand = r < A.n_reads && A.cand_flag[r] != 0u;
    const unsigned long long b = wv::ballot(cand);
    if (!b) continue;                                                       // (uniform)
    uint32_t start = 0u;
    if (lane == 0u) start = atomicAdd(&A.acc->n_candidates, (uint32_t)__popcll(b));
    start = wv::readlane(start, 0u);
    if (cand) A.cand_list[start + (uint32_t)__popcll(b & below)] = r;
  }
}

// ---- the pairs

// workgroup w takes candidates 256 * (w % n_blocks) .. and the tiles w / n_blocks, + n_slices, ...
__global__ __launch_bounds__(256) void sn_pair_kernel(SnArgs A, uint32_t n_candidates, uint32_t n_blocks, uint32_t n_slices) {
  constexpr uint32_t K = lgsn::kSnPairK, T = lgsn::kSnTile;
  __shared__ unsigned long long s_key[T * K];
  __shared__ uint32_t s_msk[T];
  __shared__ unsigned long long s_cand;                                     // the tile's reads that are candidates, a bit each
  const uint32_t t = wv::wg_thread();
  const uint32_t ci = (wv::wg_index() % n_blocks) * 256u + t, slice = wv::wg_index() / n_blocks;
  const bool has = ci < n_candidates;
  const uint32_t i = has ? A.cand_list[ci] : 0u;
  const unsigned long long* const row_i = A.val + (unsigned long long)i * A.n_class;
  const uint32_t* const chk_i = A.chk + (unsigned long long)i * A.n_words;
  const uint32_t n_tiles = (A.n_reads + T - 1u) / T;
  uint32_t count = 0u, first = kSnNone;
  for (uint32_t tile = slice; tile < n_tiles; tile += n_slices) {
    const uint32_t j0 = tile * T;
    unsigned long long ltm = 0ull, gtm = 0ull;                              // a bit per read of the tile: the candidate is below it / above it somewhere
    for (uint32_t c0 = 0; c0 < A.n_class; c0 += K) {
      unsigned long long lo[K], hi[K];
      const uint32_t mine = has ? (chk_i[c0 >> 5] >> (c0 & 31u)) & ((1u << K) - 1u) : 0u;
      WV_UNROLL
      for (uint32_t k = 0; k < K; k++) {
        const bool chk = (mine >> k) & 1u;
        const unsigned long long v = chk ? row_i[c0 + k] : 0ull;
        lo[k] = chk ? v : ~0ull; hi[k] = v;
      }
      wv::wg_barrier();                                                     // (the step before has been read)
      for (uint32_t e = t; e < T * K; e += 256u) {
        const uint32_t r = j0 + e / K, c = c0 + e % K;
        s_key[e] = r < A.n_reads && c < A.n_class ? A.val[(unsigned long long)r * A.n_class + c] : 0ull;
      }
      if (t < T) {                                                          // (the first wavefront, whole)
        const uint32_t r = j0 + t;
        s_msk[t] = r < A.n_reads ? (A.chk[(unsigned long long)r * A.n_words + (c0 >> 5)] >> (c0 & 31u)) & ((1u << K) - 1u) : 0u;
        const unsigned long long cand = wv::ballot(r < A.n_reads && A.cand_flag[r] != 0u);
        if (t == 0u) s_cand = cand;
      }
      wv::wg_barrier();
      if (has) {
        for (uint32_t j = 0; j < T; j++) {
          uint32_t lt = 0u, gt = 0u;
          WV_UNROLL
          for (uint32_t k = 0; k < K; k++) {
            const unsigned long long kj = s_key[j * K + k];
            lt |= (uint32_t)(lo[k] < kj) << k; gt |= (uint32_t)(kj < hi[k]) << k;
          }
          const uint32_t mj = s_msk[j];
          ltm |= (unsigned long long)((lt & mj) != 0u) << j; gtm |= (unsigned long long)((gt & mj) != 0u) << j;
        }
      }
    }
    const unsigned long long skewed = ltm & gtm;
    if (skewed) {
      count += (uint32_t)__popcll(skewed);
      const uint32_t least = j0 + (uint32_t)__builtin_ctzll(skewed);
      first = least < first ? least : first;
      for (unsigned long long rest = skewed & ~s_cand; rest; rest &= rest - 1ull) {      // partners that are no candidates: nobody else counts these pairs
        const uint32_t j = j0 + (uint32_t)__builtin_ctzll(rest);
        atomicAdd(&A.skew_count[j], 1u); atomicMin(&A.skew_first[j], i);
      }
    }
  }
  if (count) { atomicAdd(&A.skew_count[i], count); atomicMin(&A.skew_first[i], first); }
}

// ---- keys and summary

__global__ __launch_bounds__(256) void sn_keys_kernel(SnArgs A, uint32_t grid) {
  for (uint32_t r = wv::wg_index() * 256u + wv::wg_thread(); r < A.n_reads; r += grid * 256u) {
    const uint32_t p = A.skew_first[r];
    uint32_t below = kSnNone, above = kSnNone;
    if (p != kSnNone) {
      const unsigned long long *vr = A.val + (unsigned long long)r * A.n_class, *vp = A.val + (unsigned long long)p * A.n_class;
      const uint32_t *cr = A.chk + (unsigned long long)r * A.n_words, *cp = A.chk + (unsigned long long)p * A.n_words;
      for (uint32_t c = 0; c < A.n_class && (below == kSnNone || above == kSnNone); c++) {
        if (!sn_bit(cr, c) || !sn_bit(cp, c)) continue;
        if (below == kSnNone && vr[c] < vp[c]) below = c;
        if (above == kSnNone && vr[c] > vp[c]) above = c;
      }
    }
    A.skew_key[2ull * r] = below; A.skew_key[2ull * r + 1u] = above;
    A.snap_flags[r] = (uint8_t)(((A.cand_flag[r] & lgsn::kSnPartial) ? TBC_LEDGER_SNAP_PARTIAL : 0u) | (A.skew_count[r] ? TBC_LEDGER_SNAP_SKEWED : 0u));
  }
}

__global__ __launch_bounds__(256) void sn_count_kernel(SnArgs A, uint32_t grid) {
  const bool lane0 = (wv::wg_thread() & 63u) == 0u;
  // (whole wavefronts: every lane of one makes the same trips, the ballot is wavefront-uniform)
  for (uint32_t wave_r0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_r0 < A.n_reads; wave_r0 += grid * 256u) {
    const uint32_t r = wave_r0 + (wv::wg_thread() & 63u);
    const uint32_t n = r < A.n_reads ? A.skew_count[r] : 0u;
    const unsigned long long b = wv::ballot(n != 0u);
    if (!b) continue;                                                       // (uniform)
    if (lane0) {
      atomicAdd(&A.acc->count, (uint32_t)__popcll(b));
      atomicMin(&A.acc->first, wave_r0 + (uint32_t)__builtin_ctzll(b));
      atomicMax(&A.acc->last1, wave_r0 + 64u - (uint32_t)__builtin_clzll(b));
    }
    if (n) { atomicMax(&A.acc->worst_count, n); atomicAdd(&A.acc->sum_counts, (unsigned long long)n); }
  }
}

__global__ __launch_bounds__(256) void sn_worst_kernel(SnArgs A, uint32_t grid) {
  const bool lane0 = (wv::wg_thread() & 63u) == 0u;
  for (uint32_t wave_r0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_r0 < A.n_reads; wave_r0 += grid * 256u) {
    const uint32_t r = wave_r0 + (wv::wg_thread() & 63u);
    const uint32_t n = r < A.n_reads ? A.skew_count[r] : 0u;
    const unsigned long long b = wv::ballot(n != 0u && n == A.acc->worst_count);
    if (b && lane0) atomicMin(&A.acc->worst, wave_r0 + (uint32_t)__builtin_ctzll(b));
  }
}

__global__ __launch_bounds__(64) void sn_summary_kernel(SnArgs A) {
  if (wv::wg_thread() != 0u) return;
  const lgsn::SnAcc& a = *A.acc;
  tbc_ledger_snap_summary s{};
  s.read_count = A.n_reads; s.n_partial = a.n_partial; s.valid = a.count == 0u; s.bad_values = a.bad_values;
  s.skewed.count = a.count; s.skewed.first = a.first; s.skewed.last = a.last1 ? a.last1 - 1u : kSnNone; s.skewed.worst = a.worst;
  s.n_candidates = a.n_candidates; s.n_checked = a.n_checked; s.n_pairs = a.sum_counts / 2ull;
  *A.summary = s;
}

}  // namespace

namespace lgsn {

// The kernels of the call in order, over a launcher (oneshot_plan.h): THE statement of the launches -- the library runs them over a
// stream (ledger_snap.hip), the tests over the emulator and over a recorder.  Two sequences, because the host reads the candidates'
// number between them.  A kernel with nothing to do is not launched: no reads -- only the summary; no accounts -- no counter, so no
// sort, no scan and no candidate; no candidate -- no pair kernel.
template <class Launcher>
uint32_t grid_of(Launcher& go, unsigned long long items, uint32_t per, uint32_t cap) { return std::max(1u, go.grid((items + per - 1u) / per, cap)); }

template <class Launcher>
void filter_sequence(Launcher& go, const SnArgs& A) {
  if (!A.n_reads) return;
  const uint32_t grid_layout = grid_of(go, A.n_reads, 4u, 4096u);            // (a wavefront per read, four to a workgroup)
  go.launch(sn_layout_kernel, grid_layout, 256u, A, grid_layout);
  if (!A.n_class) return;
  const uint32_t grid_sort = go.grid(A.sort_chunks, kSnSortChunksMax);      // (the plan cuts no more chunks than that)
  for (uint32_t pass = 0; pass < kSnDigits; pass++) {
    go.launch(sn_hist_kernel, grid_sort, 64u, A, pass, grid_sort);
    go.launch(sn_carry_kernel, 1u, 256u, A);
    go.launch(sn_scatter_kernel, grid_sort, 64u, A, pass, grid_sort);
  }
  const uint32_t grid_scan = grid_of(go, (unsigned long long)A.scan_chunks * A.n_class, 256u, 16384u);
  const uint32_t grid_carry = go.grid(A.n_class, 4096u);
  go.launch(sn_extremes_kernel, grid_scan, 256u, A, grid_scan);
  go.launch(sn_scan_carry_kernel, grid_carry, 256u, A, grid_carry);
  go.launch(sn_flag_kernel, grid_scan, 256u, A, grid_scan);
  const uint32_t grid_reads = grid_of(go, A.n_reads, 256u, 16384u);
  go.launch(sn_compact_kernel, grid_reads, 256u, A, grid_reads);
}

template <class Launcher>
void rest_sequence(Launcher& go, const SnArgs& A, uint32_t n_candidates) {
  if (A.n_reads) {
    if (n_candidates) {
      // the candidates in blocks of 256, the tiles of reads in as many slices as make about 2,048 workgroups
      const uint32_t n_blocks = (n_candidates + 255u) / 256u, n_tiles = (A.n_reads + kSnTile - 1u) / kSnTile;
      const uint32_t n_slices = std::max(1u, go.grid(n_tiles, 2048u / std::min<uint32_t>(n_blocks, 2048u)));
      go.launch(sn_pair_kernel, n_blocks * n_slices, 256u, A, n_candidates, n_blocks, n_slices);
    }
    const uint32_t grid = grid_of(go, A.n_reads, 256u, 16384u);
    go.launch(sn_keys_kernel, grid, 256u, A, grid);
    go.launch(sn_count_kernel, grid, 256u, A, grid);
    go.launch(sn_worst_kernel, grid, 256u, A, grid);
  }
  go.launch(sn_summary_kernel, 1u, 64u, A);
}

}  // namespace lgsn
