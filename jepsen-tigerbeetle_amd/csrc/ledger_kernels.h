// ledger_kernels.h -- the O(micro-ops) part of tbc_ledger_check on the MI355X (gfx950): the kernel bodies.  ledger.hip compiles them
// into libtbcheck.so; their launches are lg::sequence at the end of this file; the host plan (which op is which row, the runs, the
// transfer ids, the arena) is ledger_plan.h.
// In launch order -- the kernel boundary is the only ordering between them, and no kernel holds an agent-scope fence:
//
//   lg_si_kernel            a workgroup of 256 per RUN of consecutive OK reads (grid-stride).  Lane = micro-op: 256 micro-ops a step, each
//                           lane finds its read by a binary search of the run's running lengths in LDS, loads id, a, b (8 B a lane)
//                           and the flag byte, and adds into its read's LDS words -- total, negative sum (64-bit LDS adds), unexpected,
//                           nil -- so no lane ever walks a read.  A read longer than a step is alone in its run and takes several,
//                           each lane adding up in registers and touching the LDS words once.
//                           Whether an id is an account is a binary search of the sorted accounts, in LDS when they fit.  Then a
//                           thread per read classifies (check-op's cond order) and stores read_error / read_total / read_badness;
//                           per error type the wavefront's count (ballot + popcount), first and last read go out as one atomic
//                           each, none where the wavefront has no such error; an erring read raises its type's extreme values.
//   lg_table_build_kernel   a thread per distinct invoked transfer id: the table of enc_table.h (the build of sf_table_build_kernel)
//   lg_lookup_kernel<W>     a workgroup of 256 per final lookup (grid-stride): its ids streamed coalesced, each probed, the number's bit
//                           OR-ed into an LDS window of W words; found = the popcount of the window, summed over one pass per window
//                           when |T| > 32 W; lookup_missing = |T| - found.  Repeated ids set one bit, ids nobody invoked none.
//   lg_rows_equal_kernel    (once for the final reads, once for the final lookups) grid-stride over the micro-ops of the final rows,
//                           lane = micro-op: its five fields against the first row's at the same position; a row's unlike byte is
//                           set by an atomic OR on its word, one per wavefront where the wavefront is within one row.  A row of
//                           another length is unlike without a load (a thread per row sees to that).
//   lg_finish_kernel        a thread per read: the EARLIEST read that holds each extreme value the first pass left (worst per type,
//                           lowest, highest: atomic min of the read number) -- no 128-bit keys; a thread per final row: the unlike
//                           rows and the suspect lookups counted (ballot + popcount)
//   lg_summary_kernel       one thread: counts, verdicts, the summary as the caller gets it
// Ballots, lane reads, the workgroup barrier and index / thread go through wave_env.h / wave_env_wg.h; the atomics (on LDS words and on
// global memory) are plain HIP, which tests/emu/oneshot_emu.h states for the host emulator -- these very kernels run there lane by
// lane, with a window of a few words, against the host statement of jepsen/ledger.py (tests/test_ledger_emu.py).
#pragma once
#include "wave_env_wg.h"
#include "ledger_plan.h"
#include "ledger_search.h"

namespace {

using lg::LgArgs;
using lg::LgRows;

__global__ __launch_bounds__(256) void lg_si_kernel(LgArgs A) {
  __shared__ long long s_acct[lg::kLgAcctLds];
  __shared__ uint32_t s_cum[lg::kLgRunReads + 1];
  __shared__ unsigned long long s_total[lg::kLgRunReads], s_neg[lg::kLgRunReads];
  __shared__ uint32_t s_unexp[lg::kLgRunReads], s_nil[lg::kLgRunReads];
  const uint32_t t = wv::wg_thread();
  const bool acct_lds = A.n_accounts <= lg::kLgAcctLds;
  if (acct_lds) for (uint32_t i = t; i < A.n_accounts; i += 256u) s_acct[i] = A.accounts[i];
  const long long* const acct = acct_lds ? s_acct : A.accounts;
  for (uint32_t run = wv::wg_index(); run < A.n_runs; run += A.grid_si) {
    const uint32_t r0 = A.run_first[run], R = A.run_first[run + 1u] - r0;
    const unsigned long long c0 = A.read_cum[r0];
    for (uint32_t i = t; i <= R; i += 256u) s_cum[i] = (uint32_t)(A.read_cum[r0 + i] - c0);      // (a run of several reads has at most kLgRunMops micro-ops)
    if (t < R) { s_total[t] = 0ull; s_neg[t] = 0ull; s_unexp[t] = 0u; s_nil[t] = 0u; }
    wv::wg_barrier();
    // (a read alone in its run may be longer than 2^32 micro-ops in principle: its length is taken from the 64-bit sums)
    const unsigned long long M = A.read_cum[r0 + R] - c0;
    // (a lane adds up in registers what it meets and adds to its read's words once: in a run of several reads that is one micro-op, in
    // a long read alone in its run one micro-op a step -- all of them the same read's)
    uint32_t j = 0, unexp = 0, nils = 0;
    unsigned long long sum = 0, neg_sum = 0;
    for (unsigned long long base = 0; base < M; base += 256u) {
      const unsigned long long i = base + t;
      if (i < M) {
        j = R == 1u ? 0u : lg_row_of(s_cum, R, i);
        const unsigned long long m = A.read_lo[r0 + j] + (i - (R == 1u ? 0ull : (unsigned long long)s_cum[j]));
        const long long id = A.mop_id[m];
        unexp += !lg_is_account(acct, A.n_accounts, id);
        if (A.mop_flags[m] & TBC_LEDGER_M_NIL) {
          nils++;
        } else {
          const unsigned long long bal = (unsigned long long)A.mop_a[m] - (unsigned long long)A.mop_b[m];
          sum += bal;
          if ((long long)bal < 0) neg_sum += bal;
        }
      }
    }
    if (unexp) atomicAdd(&s_unexp[j], unexp);
    if (nils) atomicAdd(&s_nil[j], nils);
    if (sum) atomicAdd(&s_total[j], sum);
    if (neg_sum) atomicAdd(&s_neg[j], neg_sum);
    wv::wg_barrier();
    // ---- a thread per read of the run
    const bool in = t < R;
    const uint32_t r = r0 + t;
    uint32_t err = 0;
    long long total = 0, bad = 0;
    if (in) {
      total = (long long)s_total[t];
      const long long neg = (long long)s_neg[t];
      if (s_unexp[t]) { err = TBC_LEDGER_E_UNEXPECTED_KEY; bad = (long long)s_unexp[t]; }
      else if (s_nil[t]) { err = TBC_LEDGER_E_NIL_BALANCE; bad = (long long)s_nil[t]; }
      else if (total != A.total_amount) {
        err = TBC_LEDGER_E_WRONG_TOTAL;
        const unsigned long long d = (unsigned long long)total - (unsigned long long)A.total_amount;
        bad = (long long)(total > A.total_amount ? d : 0ull - d);
      } else if (!A.negative_balances && neg != 0) { err = TBC_LEDGER_E_NEGATIVE_VALUE; bad = (long long)(0ull - (unsigned long long)neg); }
      A.read_error[r] = (uint8_t)err; A.read_total[r] = total; A.read_badness[r] = bad;
    }
    const uint32_t wave_r0 = r0 + (t & ~63u);
    const unsigned long long any = wv::ballot(err != 0u);
    if (any) {                                                  // (uniform across the wavefront)
      for (uint32_t k = 1; k <= 4u; k++) {
        const unsigned long long b = wv::ballot(err == k);
        if (b && (t & 63u) == 0u) {
          atomicAdd(&A.acc->count[k], (uint32_t)__popcll(b));
          atomicMin(&A.acc->first[k], wave_r0 + (uint32_t)__builtin_ctzll(b));
          atomicMax(&A.acc->last1[k], wave_r0 + 64u - (uint32_t)__builtin_clzll(b));
        }
      }
      if ((t & 63u) == 0u) {
        atomicAdd(&A.acc->error_count, (uint32_t)__popcll(any));
        atomicMin(&A.acc->first_error, wave_r0 + (uint32_t)__builtin_ctzll(any));
      }
      if (err) {
        atomicMax(&A.acc->worst_key[err], lg_key(bad));
        if (err == TBC_LEDGER_E_WRONG_TOTAL) { atomicMin(&A.acc->lowest_key, lg_key(total)); atomicMax(&A.acc->highest_key, lg_key(total)); }
      }
    }
    wv::wg_barrier();                                           // (the run's LDS words are set again only when every read is classified)
  }
}

__global__ __launch_bounds__(256) void lg_table_build_kernel(LgArgs A) {
  const uint32_t g = wv::wg_index() * 256u + wv::wg_thread();
  if (g >= A.n_transfers) return;
  const long long v = A.transfer[g];
  SfEncSlot* const tab = static_cast<SfEncSlot*>(A.slots);
  for (uint32_t s = sf_enc_hash(v) & A.tab_mask;; s = (s + 1u) & A.tab_mask)
    if (atomicCAS(&tab[s].col1, 0u, g + 1u) == 0u) { tab[s].value = v; return; }
}

template <uint32_t W>
__global__ __launch_bounds__(256) void lg_lookup_kernel(LgArgs A) {
  __shared__ uint32_t s_win[W];
  __shared__ uint32_t s_found;
  const uint32_t t = wv::wg_thread();
  const uint32_t WORDS = (A.n_transfers + 31u) / 32u;
  const SfEncSlot* __restrict__ tab = static_cast<const SfEncSlot*>(A.slots);
  for (uint32_t l = wv::wg_index(); l < A.n_final_lookups; l += A.grid_lookup) {
    const unsigned long long lo = A.fl_lo[l], hi = lo + (A.fl_cum[l + 1u] - A.fl_cum[l]);
    if (t == 0u) s_found = 0u;
    for (uint32_t w0 = 0; w0 < WORDS; w0 += W) {
      const uint32_t wn = WORDS - w0 < W ? WORDS - w0 : W;
      for (uint32_t i = t; i < wn; i += 256u) s_win[i] = 0u;
      wv::wg_barrier();
      for (unsigned long long i = lo + t; i < hi; i += 256u) {
        const uint32_t col = sf_enc_lookup(tab, A.tab_mask, A.mop_id[i]);
        if (col != kNoneU && (col >> 5) - w0 < wn) atomicOr(&s_win[(col >> 5) - w0], 1u << (col & 31u));    // (unsigned: a number below the window wraps past wn)
      }
      wv::wg_barrier();
      uint32_t n = 0;
      for (uint32_t i = t; i < wn; i += 256u) n += (uint32_t)__popc(s_win[i]);
      if (n) atomicAdd(&s_found, n);
      wv::wg_barrier();                                         // (the window is zeroed again only when everybody has counted it)
    }
    if (t == 0u) A.missing[l] = A.n_transfers - s_found;
    wv::wg_barrier();
  }
}

__device__ __forceinline__ void lg_set_unlike(uint32_t* unlike, uint32_t row) { atomicOr(&unlike[row >> 2], 1u << (8u * (row & 3u))); }

__global__ __launch_bounds__(256) void lg_rows_equal_kernel(LgArgs A, LgRows F) {
  const unsigned long long g0 = (unsigned long long)wv::wg_index() * 256u + wv::wg_thread(), stride = (unsigned long long)F.grid * 256u;
  const unsigned long long len0 = F.cum[1], total = F.cum[F.n], lo0 = F.lo[0];
  for (unsigned long long r = g0 + 1u; r < F.n; r += stride)                // a row of another length
    if (F.cum[r + 1u] - F.cum[r] != len0) lg_set_unlike(F.unlike, (uint32_t)r);
  // (every lane of a wavefront makes the same number of trips: the ballots below are wavefront-uniform)
  for (unsigned long long base = g0 - wv::wg_thread() % 64u + len0; base < total; base += stride) {
    const unsigned long long g = base + wv::wg_thread() % 64u;
    uint32_t row = 0;
    bool differs = false;
    if (g < total) {
      row = lg_row_of(F.cum, F.n, g);
      const unsigned long long pos = g - F.cum[row];
      if (F.cum[row + 1u] - F.cum[row] == len0) {
        const unsigned long long m = F.lo[row] + pos, m0 = lo0 + pos;
        differs = A.mop_id[m] != A.mop_id[m0] || A.mop_a[m] != A.mop_a[m0] || A.mop_b[m] != A.mop_b[m0] || A.mop_c[m] != A.mop_c[m0] ||
                  A.mop_flags[m] != A.mop_flags[m0];
      }
    }
    const unsigned long long b = wv::ballot(differs);
    if (b) {                                                                // (uniform) the first differing lane speaks for its row
      const uint32_t lead = (uint32_t)__builtin_ctzll(b);
      const uint32_t lead_row = wv::readlane(row, lead);
      if (differs && (row != lead_row || wv::wg_thread() % 64u == lead)) lg_set_unlike(F.unlike, row);
    }
  }
}

__global__ __launch_bounds__(256) void lg_finish_kernel(LgArgs A, uint32_t n_threads) {
  const uint32_t g = wv::wg_index() * 256u + wv::wg_thread();
  const bool lane0 = (wv::wg_thread() & 63u) == 0u;
  const uint32_t wave_g0 = g & ~63u;
  if (wave_g0 >= n_threads) return;                                         // (a whole wavefront)
  uint32_t err = 0;
  unsigned long long bad = 0, tot = 0;
  if (g < A.n_reads) { err = A.read_error[g]; bad = lg_key(A.read_badness[g]); tot = lg_key(A.read_total[g]); }
  if (wv::ballot(err != 0u)) {
    for (uint32_t k = 1; k <= 4u; k++) {
      const unsigned long long b = wv::ballot(err == k && bad == A.acc->worst_key[k]);
      if (b && lane0) atomicMin(&A.acc->worst[k], wave_g0 + (uint32_t)__builtin_ctzll(b));
    }
    const unsigned long long bl = wv::ballot(err == TBC_LEDGER_E_WRONG_TOTAL && tot == A.acc->lowest_key);
    if (bl && lane0) atomicMin(&A.acc->lowest, wave_g0 + (uint32_t)__builtin_ctzll(bl));
    const unsigned long long bh = wv::ballot(err == TBC_LEDGER_E_WRONG_TOTAL && tot == A.acc->highest_key);
    if (bh && lane0) atomicMin(&A.acc->highest, wave_g0 + (uint32_t)__builtin_ctzll(bh));
  }
  const uint8_t* const fr = reinterpret_cast<const uint8_t*>(A.fr_unlike);
  const uint8_t* const fl = reinterpret_cast<const uint8_t*>(A.fl_unlike);
  const unsigned long long b_fr = wv::ballot(g < A.n_final_reads && fr[g] != 0);
  if (b_fr && lane0) atomicAdd(&A.acc->reads_unlike, (uint32_t)__popcll(b_fr));
  const unsigned long long b_fl = wv::ballot(g < A.n_final_lookups && fl[g] != 0);
  if (b_fl && lane0) atomicAdd(&A.acc->lookups_unlike, (uint32_t)__popcll(b_fl));
  const unsigned long long b_su = wv::ballot(g < A.n_final_lookups && A.missing[g] != 0u);
  if (b_su && lane0) atomicAdd(&A.acc->suspect, (uint32_t)__popcll(b_su));
}

__global__ __launch_bounds__(64) void lg_summary_kernel(LgArgs A) {
  if (wv::wg_thread() != 0u) return;
  const lg::LgAcc& a = *A.acc;
  tbc_ledger_summary s{};
  s.read_count = A.n_reads; s.error_count = a.error_count; s.first_error = a.first_error;
  s.lowest = a.lowest; s.highest = a.highest; s.n_transfers = A.n_transfers;
  for (int k = 1; k <= 4; k++) {
    s.errors[k].count = a.count[k]; s.errors[k].first = a.first[k];
    s.errors[k].last = a.last1[k] ? a.last1[k] - 1u : 0xFFFFFFFFu; s.errors[k].worst = a.worst[k];
  }
  s.errors[0].first = s.errors[0].last = s.errors[0].worst = 0xFFFFFFFFu;
  s.n_final_reads = A.n_final_reads; s.final_reads_unlike = a.reads_unlike;
  s.n_final_lookups = A.n_final_lookups; s.final_lookups_unlike = a.lookups_unlike; s.suspect_lookups = a.suspect;
  s.valid_si = a.error_count == 0u; s.valid_lookups = a.suspect == 0u;
  s.valid_final_reads = A.n_final_reads >= 1u && A.n_final_lookups >= 1u && a.reads_unlike == 0u && a.lookups_unlike == 0u;
  *A.summary = s;
}

}  // namespace

namespace lg {

// Every kernel of the call in order, over a launcher (oneshot_plan.h): THE statement of the launches -- the library runs it over a
// stream (ledger.hip), the tests over the emulator and over a recorder.  A kernel with nothing to do is not launched: no reads, no
// invoked transfers, fewer than two final rows of a kind.  kWindowWords: the lookup kernel's LDS window.
template <uint32_t kWindowWords, class Launcher>
void sequence(Launcher& go, LgArgs A, unsigned long long fr_mops, unsigned long long fl_mops) {
  A.grid_si = go.grid(A.n_runs, 16384u);
  A.grid_lookup = go.grid(A.n_final_lookups, 4096u);
  if (A.n_runs) go.launch(lg_si_kernel, A.grid_si, 256u, A);
  if (A.n_transfers) go.launch(lg_table_build_kernel, (A.n_transfers + 255u) / 256u, 256u, A);
  if (A.n_transfers && A.n_final_lookups) go.launch(lg_lookup_kernel<kWindowWords>, A.grid_lookup, 256u, A);
  const auto rows_equal = [&](LgRows F, unsigned long long mops) {
    if (F.n < 2u) return;
    F.grid = std::max(1u, go.grid((mops + 255u) / 256u, 8192u));
    go.launch(lg_rows_equal_kernel, F.grid, 256u, A, F);
  };
  rows_equal(LgRows{A.fr_lo, A.fr_cum, A.n_final_reads, 0u, A.fr_unlike}, fr_mops);
  rows_equal(LgRows{A.fl_lo, A.fl_cum, A.n_final_lookups, 0u, A.fl_unlike}, fl_mops);
  const uint32_t n_threads = std::max(A.n_reads, std::max(A.n_final_reads, A.n_final_lookups));
  if (n_threads) go.launch(lg_finish_kernel, (n_threads + 255u) / 256u, 256u, A, n_threads);
  go.launch(lg_summary_kernel, 1u, 64u, A);
}

}  // namespace lg
