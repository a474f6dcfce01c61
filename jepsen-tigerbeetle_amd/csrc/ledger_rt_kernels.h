// ledger_rt_kernels.h -- the O(micro-ops) part of tbc_ledger_realtime on the MI355X (gfx950): the kernel bodies.  ledger_rt.hip compiles
// them into libtbcheck.so; their launches are lgrt::sequence at the end of this file; the host plan (pairing, statuses, the three
// streams of rows, the arena) is ledger_rt_plan.h;
// the rules are stated in jepsen/ledger.py.  A micro-op of a stream gives two ENTRIES, credits (e & 1 = 0) then debits, each of a CLASS
// side * n_accounts + account number and a VALUE: a transfer's amount (summed) or a read's counter as an order-preserving key (maximum).
// What the query needs per class is its entries in position order with the inclusive running sum / maximum beside each: a STABLE
// PARTITION BY CLASS WITH A RUNNING VALUE, done as the open scan of perf_kernels.h is -- chunks of whole wavefronts, per-class carries
// scanned across chunks, ordered by kernel boundaries only -- with (count, value) in the place of +-1.  In launch order, the first four
// once per stream; no kernel holds an agent-scope fence, none uses scratch, every sum is 64 bits, every grid strides:
//
//   rt_number_kernel<kReads>  a wavefront-sized workgroup per chunk.  Lane = entry: its row by a binary search of the stream's running
//                           lengths, its account's number by a binary search of the sorted accounts (in LDS up to kLgAcctLds), stored as
//                           (class, position, value).  A transfer's side that names no account and a read's micro-op that is nil or
//                           names none get no class: skipped from here on.  Per step and distinct class of the wavefront the count and
//                           the sum / maximum go into the chunk's row of the carries, one atomic each.  The possible stream counts the
//                           sides without an account and the amounts out of range.
//   rt_carry_kernel<kReads>   a workgroup per class: its column of the carries scanned exclusively down the chunks, 256 a step (wg_scan.h);
//                           the class's total count is its list's length
//   rt_offsets_kernel       ONE workgroup: the lengths scanned over the classes, 256 a step with a carried base: where each list starts
//   rt_scan_kernel<kReads>    per chunk again, 64 entries a step: per distinct class the first lane takes the class's carried (count, value) and
//                           adds the step's (one atomic with return each, on the chunk's own row), every lane of the class stores its
//                           position and the running value up to itself at list start + carried count + its rank in the step
//   rt_query_kernel         lane = read micro-op (grid-stride): per field a search by position into its class's definite list (lo), possible
//                           list (hi) and reads list (floor); the bounds stored, the read's bits OR-ed into its byte, its misses raised by
//                           atomic max; a micro-op that is not checked stores INT64_MIN
//   rt_count_kernel         lane = read (grid-stride): per kind the count (ballot + popcount), the first and last read, the greatest miss
//   rt_worst_kernel         lane = read (grid-stride): the EARLIEST read that holds each kind's greatest miss (atomic min of the read number)
//   rt_summary_kernel       one thread: the summary as the caller gets it
// Ballots, lane reads, the workgroup barrier and index / thread go through wave_env.h / wave_env_wg.h; the atomics are plain HIP, which
// tests/emu/oneshot_emu.h states for the host emulator -- these very kernels run there lane by lane (tests/test_ledger_realtime_emu.py).
#pragma once
#include "wave_env_wg.h"
#include "wg_scan.h"
#include "ledger_rt_plan.h"
#include "ledger_search.h"

namespace {

using lgrt::RtArgs;
using lgrt::RtStream;
using lgrt::kRtNone;

template <bool kMax>
__device__ __forceinline__ unsigned long long rt_op(unsigned long long a, unsigned long long b) { return kMax ? (a > b ? a : b) : a + b; }

// a - b, saturating
__device__ __forceinline__ long long rt_sat_sub(long long a, long long b) {
  long long r;
  if (__builtin_sub_overflow(a, b, &r)) r = a < 0 ? INT64_MIN : INT64_MAX;
  return r;
}

// The lanes that `has`, class by class (called by whole wavefronts; `visit` is called by every lane, once per distinct class c):
//   visit(c, lead, mine, rank, incl, n, total)   lead: the class's first lane; mine: this lane is of the class; rank: the class's lanes
//   at or below this one; incl: op over their values; n, total: the same over all the class's lanes
template <bool kMax, class Visit>
__device__ __forceinline__ void rt_wave_classes(bool has, uint32_t cls, unsigned long long val, uint32_t lane, Visit visit) {
  const unsigned long long below = (2ull << lane) - 1ull;                   // the lanes at or below this one
  unsigned long long rem = wv::ballot(has);
  while (rem) {                                                             // (uniform) a trip per distinct class of the 64 entries
    const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
    const uint32_t c = wv::readlane(cls, lead);
    const bool mine = has && cls == c;
    const unsigned long long m = wv::ballot(mine);
    unsigned long long incl = 0ull;
    for (unsigned long long mm = m; mm; mm &= mm - 1ull) {                  // (uniform) a trip per lane of the class
      const uint32_t j = (uint32_t)__builtin_ctzll(mm);
      const unsigned long long vj = wv::readlane64(val, j);
      if (j <= lane) incl = rt_op<kMax>(incl, vj);
    }
    const unsigned long long total = wv::readlane64(incl, 63u - (uint32_t)__builtin_clzll(m));
    visit(c, lead, mine, (uint32_t)__popcll(m & below), incl, (uint32_t)__popcll(m), total);
    rem &= ~m;
  }
}

template <bool kReads>
__global__ __launch_bounds__(64) void rt_number_kernel(RtArgs A, RtStream S, uint32_t count_sides) {
  __shared__ long long s_acct[lg::kLgAcctLds];
  const uint32_t lane = wv::wg_thread();
  const bool acct_lds = A.n_accounts <= lg::kLgAcctLds;
  if (acct_lds) for (uint32_t i = lane; i < A.n_accounts; i += 64u) s_acct[i] = A.accounts[i];
  wv::wg_barrier();
  const long long* const acct = acct_lds ? s_acct : A.accounts;
  uint32_t foreign = 0, bad = 0;
  for (uint32_t g = wv::wg_index(); g < S.n_chunks; g += S.grid) {
    const unsigned long long lo = (unsigned long long)g * S.chunk_entries, hi = lo + S.chunk_entries < S.n_entries ? lo + S.chunk_entries : S.n_entries;
    uint32_t* const row_cnt = S.carry_cnt + (unsigned long long)g * A.n_class;
    unsigned long long* const row_val = S.carry_val + (unsigned long long)g * A.n_class;
    for (unsigned long long base = lo; base < hi; base += 64u) {
      const unsigned long long e = base + lane;
      uint32_t cls = kRtNone;
      unsigned long long val = 0ull;
      if (e < hi) {
        const uint32_t row = lg_row_of(S.cum, S.n_rows, e >> 1), side = (uint32_t)e & 1u;
        const unsigned long long m = S.lo[row] + ((e >> 1) - S.cum[row]);
        const bool nil = (A.mop_flags[m] & TBC_LEDGER_M_NIL) != 0;
        if (kReads) {
          const uint32_t a = nil ? kRtNone : lg_account_no(acct, A.n_accounts, A.mop_id[m]);
          if (a != kRtNone) { cls = side * A.n_accounts + a; val = lg_key(side ? A.mop_b[m] : A.mop_a[m]); }
        } else {
          const uint32_t a = nil ? kRtNone : lg_account_no(acct, A.n_accounts, side ? A.mop_a[m] : A.mop_b[m]);   // credits: credit-acct (b); debits: debit-acct (a)
          const long long amount = A.mop_c[m];
          if (a != kRtNone) { cls = side * A.n_accounts + a; val = (unsigned long long)amount; }
          foreign += a == kRtNone;
          bad += !nil && side == 0u && (amount < 0 || amount >= lgrt::kRtAmountEnd);
        }
        S.ent_cls[e] = cls; S.ent_pos[e] = S.pos[row]; S.ent_val[e] = val;
      }
      rt_wave_classes<kReads>(cls != kRtNone, cls, val, lane, [&](uint32_t c, uint32_t lead, bool, uint32_t, unsigned long long, uint32_t n, unsigned long long total) {
        if (lane == lead) {
          atomicAdd(&row_cnt[c], n);
          if (kReads) atomicMax(&row_val[c], total); else atomicAdd(&row_val[c], total);
        }
      });
    }
  }
  if (!kReads && count_sides) {
    if (foreign) atomicAdd(&A.acc->foreign_sides, foreign);
    if (bad) atomicAdd(&A.acc->bad_amounts, bad);
  }
}

template <bool kReads>
__global__ __launch_bounds__(256) void rt_carry_kernel(RtArgs A, RtStream S) {
  __shared__ uint32_t s_cnt[256];
  __shared__ unsigned long long s_val[256];
  const uint32_t t = wv::wg_thread();
  for (uint32_t c = wv::wg_index(); c < A.n_class; c += S.grid) {
    uint32_t run_cnt = 0;
    unsigned long long run_val = 0ull;
    for (uint32_t g0 = 0; g0 < S.n_chunks; g0 += 256u) {
      const bool in = g0 + t < S.n_chunks;
      const unsigned long long at = (unsigned long long)(g0 + t) * A.n_class + c;
      uint32_t total_cnt;
      unsigned long long total_val;
      const uint32_t ex_cnt = wg_scan_excl(in ? S.carry_cnt[at] : 0u, s_cnt, t, 0u, total_cnt, [](uint32_t a, uint32_t b) { return a + b; });
      const unsigned long long ex_val = wg_scan_excl(in ? S.carry_val[at] : 0ull, s_val, t, 0ull, total_val, [](unsigned long long a, unsigned long long b) { return rt_op<kReads>(a, b); });
      if (in) { S.carry_cnt[at] = run_cnt + ex_cnt; S.carry_val[at] = rt_op<kReads>(run_val, ex_val); }
      run_cnt += total_cnt; run_val = rt_op<kReads>(run_val, total_val);
    }
    if (t == 0u) S.off[c + 1u] = run_cnt;                                   // (the class's length, one place up: the scan below turns it into starts)
  }
}

__global__ __launch_bounds__(256) void rt_offsets_kernel(RtArgs A, RtStream S) {   // (one workgroup)
  __shared__ uint32_t s_scan[256];
  const uint32_t t = wv::wg_thread();
  uint32_t base = 0;
  // off[0] = 0 stays; off[c + 1] = the lengths of classes 0 .. c: an inclusive scan of the lengths where they lie
  for (uint32_t c0 = 0; c0 < A.n_class; c0 += 256u) {
    const bool in = c0 + t < A.n_class;
    const uint32_t len = in ? S.off[c0 + t + 1u] : 0u;
    uint32_t total;
    const uint32_t ex = wg_scan_excl(len, s_scan, t, 0u, total, [](uint32_t a, uint32_t b) { return a + b; });
    if (in) S.off[c0 + t + 1u] = base + ex + len;
    base += total;
  }
}

template <bool kReads>
__global__ __launch_bounds__(64) void rt_scan_kernel(RtArgs A, RtStream S) {
  const uint32_t lane = wv::wg_thread();
  for (uint32_t g = wv::wg_index(); g < S.n_chunks; g += S.grid) {
    const unsigned long long lo = (unsigned long long)g * S.chunk_entries, hi = lo + S.chunk_entries < S.n_entries ? lo + S.chunk_entries : S.n_entries;
    uint32_t* const row_cnt = S.carry_cnt + (unsigned long long)g * A.n_class;
    unsigned long long* const row_val = S.carry_val + (unsigned long long)g * A.n_class;
    for (unsigned long long base = lo; base < hi; base += 64u) {
      const unsigned long long e = base + lane;
      uint32_t cls = kRtNone, pos = 0u;
      unsigned long long val = 0ull;
      if (e < hi) { cls = S.ent_cls[e]; pos = S.ent_pos[e]; val = S.ent_val[e]; }
      rt_wave_classes<kReads>(cls != kRtNone, cls, val, lane, [&](uint32_t c, uint32_t lead, bool mine, uint32_t rank, unsigned long long incl, uint32_t n, unsigned long long total) {
        uint32_t before_cnt = 0u;
        unsigned long long before_val = 0ull;
        if (lane == lead) {
          before_cnt = atomicAdd(&row_cnt[c], n);
          before_val = kReads ? atomicMax(&row_val[c], total) : atomicAdd(&row_val[c], total);
        }
        before_cnt = wv::readlane(before_cnt, lead); before_val = wv::readlane64(before_val, lead);
        if (mine) {
          const uint32_t at = S.off[c] + before_cnt + rank - 1u;
          S.list_pos[at] = pos; S.list_val[at] = rt_op<kReads>(before_val, incl);
        }
      });
    }
  }
}

// class c's list in S: the running value at its last entry whose position is below `p`, `none` if there is no such entry
__device__ __forceinline__ unsigned long long rt_before(const RtStream& S, uint32_t c, uint32_t p, unsigned long long none) {
  const uint32_t start = S.off[c], n = S.off[c + 1u] - start;
  const uint32_t* __restrict__ pos = S.list_pos + start;
  uint32_t lo = 0, hi = n;                                                  // the entries below `lo` lie before p
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (pos[mid] < p) lo = mid + 1u; else hi = mid; }
  return lo ? S.list_val[start + lo - 1u] : none;
}

__global__ __launch_bounds__(256) void rt_query_kernel(RtArgs A) {
  __shared__ long long s_acct[lg::kLgAcctLds];
  const uint32_t t = wv::wg_thread(), lane = t & 63u;
  const bool acct_lds = A.n_accounts <= lg::kLgAcctLds;
  if (acct_lds) for (uint32_t i = t; i < A.n_accounts; i += 256u) s_acct[i] = A.accounts[i];
  wv::wg_barrier();
  const long long* const acct = acct_lds ? s_acct : A.accounts;
  const RtStream& R = A.s[lgrt::kReads];
  const unsigned long long stride = (unsigned long long)A.grid_query * 256u;
  uint32_t n_checked = 0;
  // (every lane of a wavefront makes the same number of trips: the ballot below is wavefront-uniform)
  for (unsigned long long base = (unsigned long long)wv::wg_index() * 256u + (t & ~63u); base < A.n_read_mops; base += stride) {
    const unsigned long long q = base + lane;
    bool checked = false;
    if (q < A.n_read_mops) {
      const uint32_t row = lg_row_of(R.cum, R.n_rows, q);
      const unsigned long long m = R.lo[row] + (q - R.cum[row]);
      const uint32_t a = (A.mop_flags[m] & TBC_LEDGER_M_NIL) ? kRtNone : lg_account_no(acct, A.n_accounts, A.mop_id[m]);
      checked = a != kRtNone;
      uint32_t bits = 0;
      long long miss[3] = {0, 0, 0};
      for (uint32_t x = 0; x < 2u; x++) {
        long long lo = INT64_MIN, hi = INT64_MIN, floor = INT64_MIN;
        if (checked) {
          const uint32_t c = x * A.n_accounts + a, ret = R.pos[row], inv = A.read_inv[row];
          const long long v = x ? A.mop_b[m] : A.mop_a[m], init = A.init[c];
          lo = init + (A.ok_transfers_apply ? (long long)rt_before(A.s[lgrt::kDefinite], c, inv, 0ull) : 0ll);
          hi = init + (long long)rt_before(A.s[lgrt::kPossible], c, ret, 0ull);
          floor = lg_unkey(rt_before(R, c, inv, 0ull));                     // (key 0 is INT64_MIN: no earlier read)
          const long long d[3] = {rt_sat_sub(lo, v), rt_sat_sub(v, hi), rt_sat_sub(floor, v)};
          for (uint32_t k = 0; k < 3u; k++)
            if (d[k] > 0) { bits |= 1u << (2u * k + x); miss[k] = d[k] > miss[k] ? d[k] : miss[k]; }
        }
        A.mop_lo[2u * q + x] = lo; A.mop_hi[2u * q + x] = hi; A.mop_floor[2u * q + x] = floor;
      }
      if (bits) {
        atomicOr(&A.rt_bits[row >> 2], bits << (8u * (row & 3u)));
        for (uint32_t k = 0; k < 3u; k++)
          if (miss[k] > 0) atomicMax(&A.rt_miss[3ull * row + k], (unsigned long long)miss[k]);
      }
    }
    n_checked += (uint32_t)__popcll(wv::ballot(checked));
  }
  if (lane == 0u && n_checked) atomicAdd(&A.acc->n_checked, (unsigned long long)n_checked);
}

__device__ __forceinline__ uint32_t rt_bits_of(const RtArgs& A, uint32_t r) { return (A.rt_bits[r >> 2] >> (8u * (r & 3u))) & 255u; }

__global__ __launch_bounds__(256) void rt_count_kernel(RtArgs A, uint32_t grid) {
  const bool lane0 = (wv::wg_thread() & 63u) == 0u;
  // (whole wavefronts: every lane of one makes the same trips, the ballots are wavefront-uniform)
  for (uint32_t wave_g0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_g0 < A.n_reads; wave_g0 += grid * 256u) {
    const uint32_t g = wave_g0 + (wv::wg_thread() & 63u);
    const uint32_t bits = g < A.n_reads ? rt_bits_of(A, g) : 0u;
    const unsigned long long any = wv::ballot(bits != 0u);
    if (!any) continue;                                                     // (uniform)
    for (uint32_t k = 0; k < 3u; k++) {
      const bool has = (bits & (3u << (2u * k))) != 0u;
      const unsigned long long b = wv::ballot(has);
      if (b && lane0) {
        atomicAdd(&A.acc->count[k], (uint32_t)__popcll(b));
        atomicMin(&A.acc->first[k], wave_g0 + (uint32_t)__builtin_ctzll(b));
        atomicMax(&A.acc->last1[k], wave_g0 + 64u - (uint32_t)__builtin_clzll(b));
      }
      if (has) atomicMax(&A.acc->worst_miss[k], A.rt_miss[3ull * g + k]);
    }
    if (lane0) {
      atomicAdd(&A.acc->error_count, (uint32_t)__popcll(any));
      atomicMin(&A.acc->first_error, wave_g0 + (uint32_t)__builtin_ctzll(any));
    }
  }
}

__global__ __launch_bounds__(256) void rt_worst_kernel(RtArgs A, uint32_t grid) {
  const bool lane0 = (wv::wg_thread() & 63u) == 0u;
  for (uint32_t wave_g0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_g0 < A.n_reads; wave_g0 += grid * 256u) {
    const uint32_t g = wave_g0 + (wv::wg_thread() & 63u);
    const uint32_t bits = g < A.n_reads ? rt_bits_of(A, g) : 0u;
    if (!wv::ballot(bits != 0u)) continue;                                  // (uniform)
    for (uint32_t k = 0; k < 3u; k++) {
      const unsigned long long b = wv::ballot((bits & (3u << (2u * k))) != 0u && A.rt_miss[3ull * g + k] == A.acc->worst_miss[k]);
      if (b && lane0) atomicMin(&A.acc->worst[k], wave_g0 + (uint32_t)__builtin_ctzll(b));
    }
  }
}

__global__ __launch_bounds__(64) void rt_summary_kernel(RtArgs A) {
  if (wv::wg_thread() != 0u) return;
  const lgrt::RtAcc& a = *A.acc;
  tbc_ledger_rt_summary s{};
  s.read_count = A.n_reads; s.error_count = a.error_count; s.first_error = a.first_error; s.valid = a.error_count == 0u;
  for (int k = 0; k < 3; k++) {
    s.errors[k].count = a.count[k]; s.errors[k].first = a.first[k];
    s.errors[k].last = a.last1[k] ? a.last1[k] - 1u : kRtNone; s.errors[k].worst = a.worst[k];
  }
  s.n_definite = A.n_definite; s.n_possible = A.n_possible; s.foreign_sides = a.foreign_sides; s.bad_amounts = a.bad_amounts;
  s.n_checked = a.n_checked;
  *A.summary = s;
}

}  // namespace

namespace lgrt {

// Every kernel of the call in order, over a launcher (oneshot_plan.h): THE statement of the launches -- the library runs it over a
// stream (ledger_rt.hip), the tests over the emulator and over a recorder.  A kernel with nothing to do is not launched: a stream
// without entries, no reads; without accounts only the numbering runs (it counts the sides and the amounts).
template <bool kReads, class Launcher>
void stream_sequence(Launcher& go, const RtArgs& A, RtStream S, uint32_t count_sides) {
  if (!S.n_entries) return;
  S.grid = go.grid(S.n_chunks, 8192u);
  go.launch(rt_number_kernel<kReads>, S.grid, 64u, A, S, count_sides);
  if (!A.n_class) return;                                                   // (no account: every side was counted as naming none, and there is no list)
  RtStream C = S;
  C.grid = go.grid(A.n_class, 4096u);
  go.launch(rt_carry_kernel<kReads>, C.grid, 256u, A, C);
  go.launch(rt_offsets_kernel, 1u, 256u, A, S);
  go.launch(rt_scan_kernel<kReads>, S.grid, 64u, A, S);
}

template <class Launcher>
void sequence(Launcher& go, RtArgs A) {
  stream_sequence<false>(go, A, A.s[kDefinite], 0u);
  stream_sequence<false>(go, A, A.s[kPossible], 1u);
  stream_sequence<true>(go, A, A.s[kReads], 0u);
  if (A.n_read_mops) {
    A.grid_query = go.grid((A.n_read_mops + 255u) / 256u, 16384u);
    go.launch(rt_query_kernel, A.grid_query, 256u, A);
  }
  if (A.n_reads) {
    const uint32_t grid = go.grid((A.n_reads + 255u) / 256u, 16384u);
    go.launch(rt_count_kernel, grid, 256u, A, grid);
    go.launch(rt_worst_kernel, grid, 256u, A, grid);
  }
  go.launch(rt_summary_kernel, 1u, 64u, A);
}

}  // namespace lgrt
