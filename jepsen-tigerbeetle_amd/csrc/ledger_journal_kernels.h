// ledger_journal_kernels.h -- tbc_ledger_journal on the MI355X (gfx950): the kernel bodies.  ledger_journal.hip compiles them into
// libtbcheck.so; their launches are lgjn::sequence at the end of this file; the host plan (which op owns which transfer micro-op, which
// lookup has which entries, the slices, the gathered columns, the arena) is ledger_journal_plan.h; the rules are stated in
// jepsen/ledger.py ("Journal audit").  In launch order; no kernel holds an agent-scope fence, none uses scratch, every grid strides, the
// kernel boundary is the only ordering between them:
//
//   jn_claim_kernel        lane = transfer micro-op m: the table of enc_table.h over ALL of them -- a slot claimed by a CAS of m + 1, the id
//                          written behind it; micro-ops of one id take slots of their own along one probe run
//   jn_records_kernel      lane = transfer micro-op: its probe run walked to the free slot that ends it; the least number among the slots
//                          of its id is the id's RECORD, whatever the schedule of the claims was, and goes into the `pad` word of the
//                          micro-op's own slot (nobody else writes that word, no probe of this kernel reads it).  xfer_flags; the
//                          records, the reinvoked, the bad amounts and the foreign sides counted (ballot + popcount).  THE BOUND: every
//                          micro-op of an id walks all the slots of that id, so an id invoked k times costs k^2 dependent loads
//                          here and lengthens its neighbours' probes by k -- nothing for a workload that draws fresh ids (a
//                          reinvocation is an anomaly the summary counts), quadratic for a history that reuses one id throughout
//   jn_entries_kernel<W>   THE HOT ONE.  A workgroup of 256 per SLICE of a lookup (slice_entries entries; a lookup of 40k is ten).  Lane =
//                          entry: id, a, b, c and flags loaded coalesced (33 B), one probe (a 16 B slot), the record's fields gathered
//                          and compared, entry_bits stored.  The record's bit goes into a window of W LDS words -- the first W of the
//                          lookup's row of the bitmap; words past it take a global atomic OR each -- and the window's non-zero words are
//                          OR-ed into the row at the end: the slices of one lookup OR their rows.  Unknown, altered and known entries are
//                          counted per wavefront by ballot + popcount, one atomic each per slice
//   jn_members_kernel      a workgroup per CHUNK of transfer micro-ops (lane = micro-op), its owner's inv / ret / status, its amount and
//                          its two counters in registers, walking the lookups in order: its bit of row l, present -> failed / early,
//                          absent -> lost / vanished (the first lookup that showed it is known by then: lookups are numbered by ret),
//                          counted per wavefront by ballots into LDS words; the present records' amounts added into 64-bit LDS words
//                          per (lookup, counter) (up to kJnVecLds words; a row of more counters takes global atomics).  The lookups go
//                          in TILES of as many as the LDS words hold, with no barrier inside a tile; the tile's non-zero words go out
//                          as one global atomic each -- with a global atomic per (workgroup, lookup) inside the walk every workgroup
//                          waits at its next barrier for its add to one hot word.  xfer_present / early /
//                          lost / vanished are the lane's own registers, stored once: no atomic per (lookup, record)
//   jn_books_kernel        thread = (lookup, counter): init added to the vector; thread = lookup: repeated = known entries - present
//   jn_reads_kernel        a wavefront per read, four to a workgroup (lane = micro-op, the account's number by a binary search as
//                          sn_layout_kernel does), the first 64 micro-ops in registers.  A read of 8 micro-ops fills 8 lanes: the other lanes
//                          take the same micro-ops against the NEXT lookups, 64 / P side by side (P the power of two at or above the
//                          read's length), so the walk over the lookups -- a dependent load a step -- is that much shorter.  A lookup that
//                          neither began after the read ended nor ended before it began compares nothing; else the two counters against
//                          the vector, ahead / behind by one ballot for all sides, one atomic per (read, lookup) that offends.  rd_bits, rd_first stored by
//                          lane 0: a read is one wavefront's
//   jn_count_kernel, jn_worst_kernel, jn_summary_kernel   as sn_count / sn_worst / sn_summary, per kind over the lookups
// Ballots, lane reads, barriers and index / thread go through wave_env.h / wave_env_wg.h; the atomics are plain HIP, which
// tests/emu/oneshot_emu.h states for the host emulator -- these very kernels run there lane by lane.
#pragma once
#include "wave_env_wg.h"
#include "ledger_journal_plan.h"
#include "ledger_search.h"

namespace {

using lgjn::JnArgs;
using lgjn::kJnKinds;
using lgjn::kJnNone;

// the record of id v: what jn_records_kernel left in the slots of v; kJnNone if nobody invoked v
__device__ __forceinline__ uint32_t jn_record_of(const SfEncSlot* __restrict__ tab, uint32_t mask, uint32_t n_xfer, long long v) {
  if (!n_xfer) return kJnNone;
  for (uint32_t s = sf_enc_hash(v) & mask;; s = (s + 1u) & mask) {
    const SfEncSlot e = tab[s];
    if (e.col1 == 0u) return kJnNone;
    if (e.value == v) return e.pad - 1u;
  }
}

__global__ __launch_bounds__(256) void jn_claim_kernel(JnArgs A, uint32_t grid) {
  SfEncSlot* const tab = static_cast<SfEncSlot*>(A.slots);
  for (uint32_t m = wv::wg_index() * 256u + wv::wg_thread(); m < A.n_xfer; m += grid * 256u) {
    const long long v = A.x_id[m];
    for (uint32_t s = sf_enc_hash(v) & A.tab_mask;; s = (s + 1u) & A.tab_mask)
      if (atomicCAS(&tab[s].col1, 0u, m + 1u) == 0u) { tab[s].value = v; break; }
  }
}

__global__ __launch_bounds__(256) void jn_records_kernel(JnArgs A, uint32_t grid) {
  SfEncSlot* const tab = static_cast<SfEncSlot*>(A.slots);
  const uint32_t lane = wv::wg_thread() & 63u;
  uint32_t n_rec = 0, n_re = 0;                                             // (wavefront-uniform)
  // (whole wavefronts: every lane of one makes the same trips, the ballots are wavefront-uniform)
  for (uint32_t wave_m0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_m0 < A.n_xfer; wave_m0 += grid * 256u) {
    const uint32_t m = wave_m0 + lane;
    const bool in = m < A.n_xfer;
    uint32_t first = kJnNone;
    if (in) {
      const long long v = A.x_id[m];
      uint32_t mine = 0u;
      for (uint32_t s = sf_enc_hash(v) & A.tab_mask;; s = (s + 1u) & A.tab_mask) {
        const SfEncSlot e = tab[s];
        if (e.col1 == 0u) break;
        if (e.value != v) continue;
        first = e.col1 - 1u < first ? e.col1 - 1u : first;
        if (e.col1 == m + 1u) mine = s;
      }
      tab[mine].pad = first + 1u;
      const bool nil = (A.x_flags[m] & TBC_LEDGER_M_NIL) != 0;
      A.xfer_flags[m] = (uint8_t)((first != m ? TBC_LEDGER_JN_XFER_REINVOKED : 0u) | (nil ? TBC_LEDGER_JN_XFER_NIL : 0u));
      if (first == m) {                                                     // a record: its amount's range, its sides
        uint32_t foreign = 2u;
        if (!nil) {
          const long long amount = A.x_c[m];
          if (amount < 0 || amount >= lgrt::kRtAmountEnd) atomicAdd(&A.acc->bad_amounts, 1u);
          foreign = (uint32_t)!lg_is_account(A.accounts, A.n_accounts, A.x_a[m]) + (uint32_t)!lg_is_account(A.accounts, A.n_accounts, A.x_b[m]);
        }
        if (foreign) atomicAdd(&A.acc->foreign_sides, foreign);
      }
    }
    n_rec += (uint32_t)__popcll(wv::ballot(in && first == m));
    n_re += (uint32_t)__popcll(wv::ballot(in && first != m));
  }
  if (lane == 0u) {
    if (n_rec) atomicAdd(A.n_records, n_rec);
    if (n_re) atomicAdd(&A.acc->n_reinvoked, n_re);
  }
}

template <uint32_t W>
__global__ __launch_bounds__(256) void jn_entries_kernel(JnArgs A, uint32_t grid) {
  __shared__ uint32_t s_win[W];
  const uint32_t t = wv::wg_thread(), lane = t & 63u;
  const uint32_t wn = A.n_words < W ? A.n_words : W;
  const SfEncSlot* __restrict__ tab = static_cast<const SfEncSlot*>(A.slots);
  for (uint32_t item = wv::wg_index(); item < A.n_slices; item += grid) {
    const uint32_t l = lg_row_of(A.slice_cum, A.n_lookups, item);
    const unsigned long long end = A.lk_cum[l + 1u];
    const unsigned long long lo = A.lk_cum[l] + (unsigned long long)(item - A.slice_cum[l]) * A.slice_entries;
    const unsigned long long hi = lo + A.slice_entries < end ? lo + A.slice_entries : end;
    uint32_t* const row = A.bitmap + (unsigned long long)l * A.n_words;
    for (uint32_t i = t; i < wn; i += 256u) s_win[i] = 0u;
    wv::wg_barrier();
    uint32_t n_unknown = 0, n_altered = 0, n_known = 0;                     // (wavefront-uniform)
    // (whole wavefronts: every lane of one makes the same trips, the ballots are wavefront-uniform)
    for (unsigned long long e0 = lo + (t & ~63u); e0 < hi; e0 += 256u) {
      const unsigned long long e = e0 + lane;
      uint32_t bits = 0u;
      bool known = false;
      if (e < hi) {
        const long long id = A.e_id[e], ea = A.e_a[e], eb = A.e_b[e], ec = A.e_c[e];   // (five loads in flight before the probe)
        const uint8_t ef = A.e_flags[e];
        const uint32_t rec = jn_record_of(tab, A.tab_mask, A.n_xfer, id);
        if (rec == kJnNone) {
          bits = TBC_LEDGER_JN_ENTRY_UNKNOWN;
        } else {
          known = true;
          const long long xa = A.x_a[rec], xb = A.x_b[rec], xc = A.x_c[rec];
          const uint8_t xf = A.x_flags[rec];
          if ((rec >> 5) < wn) atomicOr(&s_win[rec >> 5], 1u << (rec & 31u));
          else atomicOr(&row[rec >> 5], 1u << (rec & 31u));
          if (((ef | xf) & TBC_LEDGER_M_NIL) || xa != ea || xb != eb || xc != ec) bits = TBC_LEDGER_JN_ENTRY_ALTERED;
        }
        A.entry_bits[e] = (uint8_t)bits;
      }
      n_unknown += (uint32_t)__popcll(wv::ballot(bits == TBC_LEDGER_JN_ENTRY_UNKNOWN));
      n_altered += (uint32_t)__popcll(wv::ballot(bits == TBC_LEDGER_JN_ENTRY_ALTERED));
      n_known += (uint32_t)__popcll(wv::ballot(known));
    }
    if (lane == 0u) {
      uint32_t* const counts = A.lk_counts + (unsigned long long)l * kJnKinds;
      if (n_unknown) atomicAdd(&counts[TBC_LEDGER_JN_UNKNOWN], n_unknown);
      if (n_altered) atomicAdd(&counts[TBC_LEDGER_JN_ALTERED], n_altered);
      if (n_known) atomicAdd(&A.lk_known[l], n_known);
    }
    wv::wg_barrier();
    for (uint32_t i = t; i < wn; i += 256u)
      if (s_win[i]) atomicOr(&row[i], s_win[i]);
    wv::wg_barrier();                                                       // (the window is zeroed again only when everybody has written it out)
  }
}

__global__ __launch_bounds__(256) void jn_members_kernel(JnArgs A, uint32_t n_chunks, uint32_t grid) {
  __shared__ unsigned long long s_vec[lgjn::kJnVecLds];                     // [lookup of the tile][counter]
  __shared__ uint32_t s_cnt[lgjn::kJnTile * 5u];                            // [lookup of the tile][present, failed, early, lost, vanished]
  const uint32_t t = wv::wg_thread(), lane = t & 63u;
  const bool vec_lds = A.n_class <= lgjn::kJnVecLds;
  const uint32_t fit = vec_lds && A.n_class ? lgjn::kJnVecLds / A.n_class : lgjn::kJnTile;
  const uint32_t tile = fit < A.tile ? fit : A.tile;                        // lookups whose counts and sums the LDS words hold at a time
  for (uint32_t chunk = wv::wg_index(); chunk < n_chunks; chunk += grid) {
    const uint32_t m = chunk * A.chunk + t;
    const bool in = t < A.chunk && m < A.n_xfer;
    const uint32_t flags = in ? A.xfer_flags[m] : (uint32_t)TBC_LEDGER_JN_XFER_REINVOKED;
    const bool record = !(flags & TBC_LEDGER_JN_XFER_REINVOKED), moves = record && !(flags & TBC_LEDGER_JN_XFER_NIL);
    uint32_t inv = 0u, ret = kJnNone, status = TBC_LEDGER_T_INVOKE, cc = kJnNone, dc = kJnNone;
    unsigned long long amount = 0ull;
    if (record) { inv = A.x_inv[m]; ret = A.x_ret[m]; status = A.x_status[m]; }
    if (moves) {                                                            // credit-acct: counter 2k; debit-acct: counter 2k' + 1
      amount = (unsigned long long)A.x_c[m];
      const uint32_t ka = lg_account_no(A.accounts, A.n_accounts, A.x_b[m]), kb = lg_account_no(A.accounts, A.n_accounts, A.x_a[m]);
      if (ka != kJnNone) cc = 2u * A.acct_pos[ka];
      if (kb != kJnNone) dc = 2u * A.acct_pos[kb] + 1u;
    }
    const uint32_t word = m >> 5, bit = 1u << (m & 31u);
    uint32_t n_present = 0, n_early = 0, n_lost = 0, n_vanished = 0, seen_ret = kJnNone;
    // (every lane of the workgroup walks every lookup: the ballots are wavefront-uniform, the barriers the workgroup's)
    for (uint32_t l0 = 0; l0 < A.n_lookups; l0 += tile) {
      const uint32_t tn = A.n_lookups - l0 < tile ? A.n_lookups - l0 : tile;
      for (uint32_t i = t; i < tn * 5u; i += 256u) s_cnt[i] = 0u;
      if (vec_lds) for (uint32_t i = t; i < tn * A.n_class; i += 256u) s_vec[i] = 0ull;
      wv::wg_barrier();
      for (uint32_t k = 0; k < tn; k++) {
        const uint32_t l = l0 + k, l_inv = A.lk_inv[l], l_ret = A.lk_ret[l];
        const bool present = record && (A.bitmap[(unsigned long long)l * A.n_words + word] & bit) != 0u;
        const bool absent = record && !present;
        const bool failed = present && status == TBC_LEDGER_T_FAIL, early = present && inv > l_ret;
        const bool lost = absent && A.ok_transfers_apply && status == TBC_LEDGER_T_OK && ret < l_inv;
        const bool vanished = absent && seen_ret < l_inv;                   // (seen_ret: all ones until a lookup has shown it; l_inv: 0 without an invocation)
        if (present && seen_ret == kJnNone) seen_ret = l_ret;
        n_present += present; n_early += early; n_lost += lost; n_vanished += vanished;
        const unsigned long long bp = wv::ballot(present), bf = wv::ballot(failed), be = wv::ballot(early), bl = wv::ballot(lost), bv = wv::ballot(vanished);
        if (lane == 0u) {
          uint32_t* const cnt = s_cnt + k * 5u;
          if (bp) atomicAdd(&cnt[0], (uint32_t)__popcll(bp));
          if (bf) atomicAdd(&cnt[1], (uint32_t)__popcll(bf));
          if (be) atomicAdd(&cnt[2], (uint32_t)__popcll(be));
          if (bl) atomicAdd(&cnt[3], (uint32_t)__popcll(bl));
          if (bv) atomicAdd(&cnt[4], (uint32_t)__popcll(bv));
        }
        if (present && moves) {
          unsigned long long* const vec = vec_lds ? s_vec + k * A.n_class : reinterpret_cast<unsigned long long*>(A.lk_vector) + (unsigned long long)l * A.n_class;
          if (cc != kJnNone) atomicAdd(&vec[cc], amount);
          if (dc != kJnNone) atomicAdd(&vec[dc], amount);
        }
      }
      wv::wg_barrier();
      // the tile's non-zero words out (the thread that zeroes word i next is the one that reads it here)
      for (uint32_t i = t; i < tn * 5u; i += 256u) {
        if (!s_cnt[i]) continue;
        const uint32_t l = l0 + i / 5u, kind = i % 5u;
        atomicAdd(kind ? &A.lk_counts[(unsigned long long)l * kJnKinds + (TBC_LEDGER_JN_FAILED - 1u) + kind] : &A.lk_present[l], s_cnt[i]);
      }
      if (vec_lds) {
        unsigned long long* const vec = reinterpret_cast<unsigned long long*>(A.lk_vector) + (unsigned long long)l0 * A.n_class;
        for (uint32_t i = t; i < tn * A.n_class; i += 256u)
          if (s_vec[i]) atomicAdd(&vec[i], s_vec[i]);
      }
    }
    if (in) { A.xfer_present[m] = n_present; A.xfer_early[m] = n_early; A.xfer_lost[m] = n_lost; A.xfer_vanished[m] = n_vanished; }
  }
}

__global__ __launch_bounds__(256) void jn_books_kernel(JnArgs A, uint32_t grid) {
  const uint32_t cx = A.n_class ? A.n_class : 1u;
  const unsigned long long n = (unsigned long long)A.n_lookups * cx;
  for (unsigned long long q = (unsigned long long)wv::wg_index() * 256u + wv::wg_thread(); q < n; q += (unsigned long long)grid * 256u) {
    const uint32_t l = (uint32_t)(q / cx), c = (uint32_t)(q % cx);
    if (c < A.n_class) A.lk_vector[(unsigned long long)l * A.n_class + c] += A.init[c];
    if (c == 0u) A.lk_counts[(unsigned long long)l * kJnKinds + TBC_LEDGER_JN_REPEATED] = A.lk_known[l] - A.lk_present[l];
  }
}

__global__ __launch_bounds__(256) void jn_reads_kernel(JnArgs A, uint32_t grid) {
  __shared__ long long s_acct[lg::kLgAcctLds];
  __shared__ unsigned long long s_checked;
  const uint32_t t = wv::wg_thread(), lane = t & 63u;
  const bool acct_lds = A.n_accounts <= lg::kLgAcctLds;
  if (acct_lds) for (uint32_t i = t; i < A.n_accounts; i += 256u) s_acct[i] = A.accounts[i];
  if (t == 0u) s_checked = 0ull;
  wv::wg_barrier();
  const long long* const acct = acct_lds ? s_acct : A.accounts;
  // the counter (credits-posted) of read micro-op m, kJnNone where it is not checked
  const auto counter_of = [&](unsigned long long m) {
    const uint32_t a = (A.r_flags[m] & TBC_LEDGER_M_NIL) ? kJnNone : lg_account_no(acct, A.n_accounts, A.r_id[m]);
    return a == kJnNone ? kJnNone : 2u * A.acct_pos[a];
  };
  unsigned long long n_checked = 0;                                         // (wavefront-uniform)
  // (whole wavefronts: a read is one wavefront's, the ballots are wavefront-uniform)
  for (uint32_t r = wv::wg_index() * 4u + (t >> 6); r < A.n_reads; r += grid * 4u) {
    const unsigned long long lo = A.rd_cum[r], hi = A.rd_cum[r + 1u];
    const uint32_t r_inv = A.rd_inv[r], r_ret = A.rd_ret[r];
    // a read of n micro-ops takes P = the power of two at or above n lanes (64 at most) a lookup, so 64 / P lookups go side by side:
    // lane = (micro-op j, side s)
    uint32_t P = 1u;
    while (P < 64u && P < hi - lo) P <<= 1;
    const uint32_t G = 64u / P, j = lane & (P - 1u), side = lane / P;
    const unsigned long long mine = P == 64u ? ~0ull : ((1ull << P) - 1ull) << (side * P);      // the lanes of this lane's side
    uint32_t c0 = kJnNone;                                                  // the lane's first micro-op, in registers
    long long va0 = 0, vb0 = 0;
    if (lo + j < hi) { c0 = counter_of(lo + j); va0 = A.r_a[lo + j]; vb0 = A.r_b[lo + j]; }
    n_checked += (unsigned long long)__popcll(wv::ballot(side == 0u && c0 != kJnNone));
    for (unsigned long long m0 = lo + 64u; m0 < hi; m0 += 64u) n_checked += (unsigned long long)__popcll(wv::ballot(m0 + lane < hi && counter_of(m0 + lane) != kJnNone));
    uint32_t bits = 0u, first_ahead = kJnNone, first_behind = kJnNone;
    for (uint32_t l0 = 0; l0 < A.n_lookups; l0 += G) {
      const uint32_t l = l0 + side;
      const bool has = l < A.n_lookups;
      const bool before = has && r_ret < A.lk_inv[l], after = has && A.lk_ret[l] < r_inv;   // the read ended before the lookup began; the lookup ended before the read began
      bool ahead = false, behind = false;
      if (before || after) {
        const long long* const vec = A.lk_vector + (unsigned long long)l * A.n_class;
        if (c0 != kJnNone) {
          const long long j0 = vec[c0], j1 = vec[c0 + 1u];
          ahead = before && (va0 > j0 || vb0 > j1); behind = after && (va0 < j0 || vb0 < j1);
        }
        for (unsigned long long m = lo + lane + 64u; m < hi; m += 64u) {    // (a read of more than 64 micro-ops -- one lookup at a time: the rest from memory)
          const uint32_t c = counter_of(m);
          if (c == kJnNone) continue;
          const long long va = A.r_a[m], vb = A.r_b[m], j0 = vec[c], j1 = vec[c + 1u];
          ahead = ahead || (before && (va > j0 || vb > j1)); behind = behind || (after && (va < j0 || vb < j1));
        }
      }
      const unsigned long long ba = wv::ballot(ahead), bb = wv::ballot(behind);
      if (ba) {                                                             // (the sides hold ascending lookups: the lowest lane set is the least lookup)
        bits |= TBC_LEDGER_JN_READ_AHEAD; first_ahead = first_ahead == kJnNone ? l0 + (uint32_t)__builtin_ctzll(ba) / P : first_ahead;
        if (j == 0u && (ba & mine)) atomicAdd(&A.lk_counts[(unsigned long long)l * kJnKinds + TBC_LEDGER_JN_AHEAD], 1u);
      }
      if (bb) {
        bits |= TBC_LEDGER_JN_READ_BEHIND; first_behind = first_behind == kJnNone ? l0 + (uint32_t)__builtin_ctzll(bb) / P : first_behind;
        if (j == 0u && (bb & mine)) atomicAdd(&A.lk_counts[(unsigned long long)l * kJnKinds + TBC_LEDGER_JN_BEHIND], 1u);
      }
    }
    if (lane == 0u) { A.rd_bits[r] = (uint8_t)bits; A.rd_first[2ull * r] = first_ahead; A.rd_first[2ull * r + 1u] = first_behind; }
  }
  // (one global atomic a workgroup, not one a wavefront: they all go to the one word)
  if (n_checked && lane == 0u) atomicAdd(&s_checked, n_checked);
  wv::wg_barrier();
  if (t == 0u && s_checked) atomicAdd(&A.acc->n_checked, s_checked);
}

// ---- per kind over the lookups: count, first, last, the greatest count, the total; then the earliest lookup that holds the greatest

__global__ __launch_bounds__(256) void jn_count_kernel(JnArgs A, uint32_t grid) {
  const uint32_t lane = wv::wg_thread() & 63u;
  // (whole wavefronts: every lane of one makes the same trips, the ballots are wavefront-uniform)
  for (uint32_t wave_l0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_l0 < A.n_lookups; wave_l0 += grid * 256u) {
    const uint32_t l = wave_l0 + lane;
    for (uint32_t k = 0; k < kJnKinds; k++) {
      const uint32_t n = l < A.n_lookups ? A.lk_counts[(unsigned long long)l * kJnKinds + k] : 0u;
      const unsigned long long b = wv::ballot(n != 0u);
      if (!b) continue;                                                     // (uniform)
      if (lane == 0u) {
        atomicAdd(&A.acc->count[k], (uint32_t)__popcll(b));
        atomicMin(&A.acc->first[k], wave_l0 + (uint32_t)__builtin_ctzll(b));
        atomicMax(&A.acc->last1[k], wave_l0 + 64u - (uint32_t)__builtin_clzll(b));
      }
      if (n) { atomicMax(&A.acc->worst_count[k], n); atomicAdd(&A.acc->total[k], (unsigned long long)n); }
    }
  }
}

__global__ __launch_bounds__(256) void jn_worst_kernel(JnArgs A, uint32_t grid) {
  const uint32_t lane = wv::wg_thread() & 63u;
  for (uint32_t wave_l0 = wv::wg_index() * 256u + (wv::wg_thread() & ~63u); wave_l0 < A.n_lookups; wave_l0 += grid * 256u) {
    const uint32_t l = wave_l0 + lane;
    for (uint32_t k = 0; k < kJnKinds; k++) {
      const uint32_t n = l < A.n_lookups ? A.lk_counts[(unsigned long long)l * kJnKinds + k] : 0u;
      const unsigned long long b = wv::ballot(n != 0u && n == A.acc->worst_count[k]);
      if (b && lane == 0u) atomicMin(&A.acc->worst[k], wave_l0 + (uint32_t)__builtin_ctzll(b));
    }
  }
}

__global__ __launch_bounds__(64) void jn_summary_kernel(JnArgs A) {
  if (wv::wg_thread() != 0u) return;
  const lgjn::JnAcc& a = *A.acc;
  tbc_ledger_journal_summary s{};
  s.n_lookups = A.n_lookups; s.n_xfer_mops = A.n_xfer; s.n_records = *A.n_records; s.n_reinvoked = a.n_reinvoked;
  s.foreign_sides = a.foreign_sides; s.bad_amounts = a.bad_amounts; s.read_count = A.n_reads; s.valid = 1u;
  for (uint32_t k = 0; k < kJnKinds; k++) {
    s.errors[k].count = a.count[k]; s.errors[k].first = a.first[k]; s.errors[k].last = a.last1[k] ? a.last1[k] - 1u : kJnNone; s.errors[k].worst = a.worst[k];
    s.totals[k] = a.total[k];
    if (a.total[k]) s.valid = 0u;
  }
  s.n_entries = A.n_entries; s.n_checked = a.n_checked;
  *A.summary = s;
}

}  // namespace

namespace lgjn {

// Every kernel of the call in order, over a launcher (oneshot_plan.h): THE statement of the launches -- the library runs it over a
// stream (ledger_journal.hip), the tests over the emulator and over a recorder.  A kernel with nothing to do is not launched: no
// transfer micro-op -- no table, no records, no members; no entry -- no entries kernel; no lookup -- no books and nothing to count; no
// read -- no reads kernel.  kWindowWords: the entries kernel's LDS window.
template <class Launcher>
uint32_t grid_of(Launcher& go, unsigned long long items, uint32_t per, uint32_t cap) { return std::max(1u, go.grid((items + per - 1u) / per, cap)); }

// the grid of the kernels that stride over transfer micro-ops, slices, chunks and reads: 8 workgroups of 256 for each of the 256
// compute units fill the device; more only queue
constexpr uint32_t kGridCap = 2048;

template <uint32_t kWindowWords, class Launcher>
void sequence(Launcher& go, const JnArgs& A) {
  if (A.n_xfer) {
    const uint32_t grid = grid_of(go, A.n_xfer, 256u, kGridCap);
    go.launch(jn_claim_kernel, grid, 256u, A, grid);
    go.launch(jn_records_kernel, grid, 256u, A, grid);
  }
  if (A.n_slices) {
    const uint32_t grid = go.grid(A.n_slices, kGridCap);
    go.launch(jn_entries_kernel<kWindowWords>, grid, 256u, A, grid);
  }
  if (A.n_xfer) {
    const uint32_t n_chunks = (A.n_xfer + A.chunk - 1u) / A.chunk, grid = go.grid(n_chunks, kGridCap);
    go.launch(jn_members_kernel, grid, 256u, A, n_chunks, grid);
  }
  if (A.n_lookups) {
    const uint32_t grid = grid_of(go, (unsigned long long)A.n_lookups * std::max(1u, A.n_class), 256u, 16384u);
    go.launch(jn_books_kernel, grid, 256u, A, grid);
  }
  if (A.n_reads) {
    const uint32_t grid = grid_of(go, A.n_reads, 4u, kGridCap);               // (a wavefront per read, four to a workgroup)
    go.launch(jn_reads_kernel, grid, 256u, A, grid);
  }
  if (A.n_lookups) {
    const uint32_t grid = grid_of(go, A.n_lookups, 256u, 4096u);
    go.launch(jn_count_kernel, grid, 256u, A, grid);
    go.launch(jn_worst_kernel, grid, 256u, A, grid);
  }
  go.launch(jn_summary_kernel, 1u, 64u, A);
}

}  // namespace lgjn
