// ledger_plan.h -- the host plan of tbc_ledger_check (the ledger workload's checkers, include/tbcheck.h): plain C++ with no HIP call in
// it.  ledger_host.hip runs every call through it, and so do the emulator program of the kernels (tests/emu/emu_ledger.cpp) and the
// stand-alone program of the plan (tests/emu/ledger_plan.cpp), so the rules below have one statement in C.
//
//   validate   every rule of tbc_ledger_in that the kernels trust, O(ops) + O(read micro-ops)
//   plan       O(ops) + O(invoked transfer micro-ops): the row tables -- for each OK read, final read and final lookup its slice of
//              the micro-op columns (where it starts, and a running sum of the lengths: a lane finds its row by a binary search of
//              that) --, the RUNS the SI kernel's workgroups take (consecutive reads of at most kLgRunMops micro-ops and kLgRunReads
//              reads together; a longer read is a run of its own), the distinct invoked transfer ids, the sorted accounts, and the
//              arena as named regions with 256 B starts.  The lookups' micro-ops -- the big part -- are never looked at here.
//   steps      the call from the plan to the filled output, over a call frame: the library's and the emulator's run this one list
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_set>
#include <vector>
#include "../../include/tbcheck.h"
#include "enc_table.h"
#include "oneshot_plan.h"
#include "set_full_encode_plan.h"          // sfenc::table_slots

namespace lg {

constexpr uint32_t kLgRunMops = 256;        // micro-ops a run's reads have together (one step of a workgroup of 256), unless it is one long read
constexpr uint32_t kLgRunReads = 256;       // reads per run at most: their accumulators are LDS words, a thread per read classifies
constexpr uint32_t kLgAcctLds = 1024;       // accounts kept in LDS at most (more: the binary search reads global memory)

// what the kernels add up, in device memory (the head of the arena; the host writes the start values).  Read numbers; a `last` is
// kept as number + 1 (0: none), the extremes' values as order-preserving unsigned keys (lg_key)
struct LgAcc {
  uint32_t count[5], first[5], last1[5], worst[5];
  uint32_t lowest, highest, first_error, error_count;
  unsigned long long worst_key[5], lowest_key, highest_key;
  uint32_t reads_unlike, lookups_unlike, suspect, pad;
};

// what the kernels take (ledger_kernels.h), every pointer into the arena
struct LgArgs {
  LgAcc* acc; tbc_ledger_summary* summary;
  const long long *mop_id, *mop_a, *mop_b, *mop_c; const uint8_t* mop_flags;
  const long long* accounts; uint32_t n_accounts, negative_balances; long long total_amount;
  const unsigned long long *read_lo, *read_cum; const uint32_t* run_first; uint32_t n_reads, n_runs, grid_si;
  uint8_t* read_error; long long *read_total, *read_badness;
  const long long* transfer; void* slots /* SfEncSlot[] */; uint32_t n_transfers, tab_mask;
  const unsigned long long *fl_lo, *fl_cum; uint32_t n_final_lookups, grid_lookup; uint32_t* missing;
  const unsigned long long *fr_lo, *fr_cum; uint32_t n_final_reads;
  uint32_t *fr_unlike, *fl_unlike;          // a byte per row, in whole words
};

// the final rows of one kind, as lg_rows_equal_kernel takes them
struct LgRows { const unsigned long long *lo, *cum; uint32_t n, grid; uint32_t* unlike; };

// Every kernel of the call on `stream` (a hipStream_t: this header names no HIP type): lg::sequence of ledger_kernels.h over the
// library's launcher; defined in ledger.hip, the unit that holds the kernels.  fr_mops / fl_mops: the micro-ops of all final reads /
// final lookups.  The grids are the sequence's to choose (grid_si, grid_lookup of `A` are ignored).
void launch(void* stream, LgArgs A, unsigned long long fr_mops, unsigned long long fl_mops);

using oneshot::Region;
using LgRegion = Region;                   // (the name it had while this header held it: programs written against that still build)

// The call's one arena, in order: the head the host makes (ONE image, one copy), the caller's micro-op columns, what the device
// makes (zeroed before the kernels: the table's slots, the unlike bytes, the lookups' missing counts), the per-read results.
struct LgArena {
  Region acc, summary, accounts, transfer, read_lo, read_cum, run_first, fr_lo, fr_cum, fl_lo, fl_cum;        // the head
  Region mop_id, mop_a, mop_b, mop_c, mop_flags;                                                              // the caller's
  Region slots, fr_unlike, fl_unlike, missing;                                                                // zeroed
  Region read_error, read_total, read_badness;
  size_t bytes = 0;
  size_t head_bytes() const { return mop_id.at; }
  size_t zero_bytes() const { return read_error.at - slots.at; }
};

struct Plan {
  uint32_t n_reads = 0, n_runs = 0, n_final_reads = 0, n_final_lookups = 0, n_transfers = 0, tab_mask = 0;
  uint64_t n_mops = 0, tab_slots = 0;
  std::vector<uint64_t> read_lo, read_cum;            // [n_reads], [n_reads + 1]: read r's micro-ops start at read_lo[r]; read_cum: the lengths summed
  std::vector<uint32_t> run_first;                    // [n_runs + 1]: run k is reads run_first[k] .. run_first[k + 1]
  std::vector<uint64_t> fr_lo, fr_cum, fl_lo, fl_cum; // the final reads and the final lookups likewise
  std::vector<int64_t> transfer;                      // [n_transfers] the distinct invoked transfer ids, in order of first invocation
  std::vector<int64_t> accounts;                      // sorted
  LgArena arena;
};

// false: `err` names the entry point and the op (by its row and its index)
inline bool validate(const char* fn, const tbc_ledger_in* in, std::string& err) {
  char buf[256];
  const auto say = [&](const char* what) { std::snprintf(buf, sizeof buf, "%s: %s", fn, what); err = buf; return false; };
  const auto fail = [&](const char* what, uint32_t i) {
    std::snprintf(buf, sizeof buf, "%s: op %u (index %u): %s", fn, i, in->index[i], what);
    err = buf;
    return false;
  };
  if (!in->mop_off) return say("null argument (mop_off)");
  if (in->n_ops && (!in->index || !in->type || !in->kind || !in->flags)) return say("null argument (index, type, kind, flags)");
  if (in->n_accounts && !in->accounts) return say("null argument (accounts)");
  if (in->negative_balances > 1u) return say("negative_balances is 0 or 1");
  if (in->mop_off[0] != 0) return say("mop_off[0] must be 0");
  for (uint32_t i = 0; i < in->n_ops; i++) {
    if (i && in->index[i] <= in->index[i - 1]) return fail("index must be strictly ascending", i);
    if (in->index[i] == 0xFFFFFFFFu) return fail("index 2^32 - 1 is TBC_NO_OP", i);
    if (in->type[i] > TBC_LEDGER_T_INFO) return fail("type is not a TBC_LEDGER_T_*", i);
    if (in->kind[i] > TBC_LEDGER_K_LOOKUP) return fail("kind is not a TBC_LEDGER_K_*", i);
    if (in->flags[i] & ~TBC_LEDGER_F_FINAL) return fail("unknown op flags", i);
    if (in->mop_off[i + 1] < in->mop_off[i]) return fail("mop_off must be ascending", i);
  }
  if (in->mop_off[in->n_ops] && (!in->mop_id || !in->mop_a || !in->mop_b || !in->mop_c || !in->mop_flags)) return say("null argument (the micro-op columns)");
  {
    std::vector<int64_t> a(in->accounts, in->accounts + in->n_accounts);
    std::sort(a.begin(), a.end());
    for (size_t k = 1; k < a.size(); k++)
      if (a[k] == a[k - 1]) { std::snprintf(buf, sizeof buf, "%s: account %lld is listed twice (accounts must be distinct)", fn, (long long)a[k]); err = buf; return false; }
  }
  std::vector<int64_t> ids;
  for (uint32_t i = 0; i < in->n_ops; i++) {
    if (in->type[i] != TBC_LEDGER_T_OK || in->kind[i] != TBC_LEDGER_K_READ) continue;
    const uint64_t lo = in->mop_off[i], hi = in->mop_off[i + 1];
    bool ascending = true;
    for (uint64_t m = lo; m < hi; m++) {
      if (in->mop_flags[m] & ~TBC_LEDGER_M_NIL) return fail("unknown micro-op flags", i);
      if (m > lo && in->mop_id[m] <= in->mop_id[m - 1]) ascending = false;
    }
    if (ascending) continue;                  // (what a read of the accounts in order gives: seen to be distinct in the one pass)
    ids.assign(in->mop_id + lo, in->mop_id + hi);
    std::sort(ids.begin(), ids.end());
    for (size_t k = 1; k < ids.size(); k++)
      if (ids[k] == ids[k - 1]) return fail("an :ok read names an id twice (ids must be distinct within a read)", i);
  }
  return true;
}

// (the input has passed `validate`.)  false: too much for one call (`err` says what)
inline bool plan(const char* fn, const tbc_ledger_in* in, Plan& P, std::string& err) {
  P = Plan{};
  P.n_mops = in->mop_off[in->n_ops];
  P.read_cum.push_back(0); P.fr_cum.push_back(0); P.fl_cum.push_back(0);
  std::unordered_set<int64_t> seen;
  for (uint32_t i = 0; i < in->n_ops; i++) {
    const uint64_t lo = in->mop_off[i], n = in->mop_off[i + 1] - lo;
    const bool final = (in->flags[i] & TBC_LEDGER_F_FINAL) != 0;
    if (in->type[i] == TBC_LEDGER_T_INVOKE && in->kind[i] == TBC_LEDGER_K_TRANSFER) {
      for (uint64_t m = lo; m < lo + n; m++)
        if (seen.insert(in->mop_id[m]).second) P.transfer.push_back(in->mop_id[m]);
    } else if (in->type[i] == TBC_LEDGER_T_OK && in->kind[i] == TBC_LEDGER_K_READ) {
      P.read_lo.push_back(lo); P.read_cum.push_back(P.read_cum.back() + n);
      if (final) { P.fr_lo.push_back(lo); P.fr_cum.push_back(P.fr_cum.back() + n); }
    } else if (in->type[i] == TBC_LEDGER_T_OK && in->kind[i] == TBC_LEDGER_K_LOOKUP && final) {
      P.fl_lo.push_back(lo); P.fl_cum.push_back(P.fl_cum.back() + n);
    }
  }
  if (P.transfer.size() >= 0x40000000ull) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: more than 2^30 - 1 distinct invoked transfers in one call", fn);
    err = buf;
    return false;
  }
  P.n_reads = (uint32_t)P.read_lo.size(); P.n_final_reads = (uint32_t)P.fr_lo.size(); P.n_final_lookups = (uint32_t)P.fl_lo.size();
  P.n_transfers = (uint32_t)P.transfer.size();
  P.tab_slots = sfenc::table_slots(P.n_transfers); P.tab_mask = P.tab_slots ? (uint32_t)(P.tab_slots - 1u) : 0u;
  // the runs: as many consecutive reads as stay within kLgRunMops micro-ops and kLgRunReads reads; a read of more is alone in its run
  P.run_first.push_back(0);
  for (uint32_t r = 0; r < P.n_reads;) {
    uint32_t e = r + 1;
    while (e < P.n_reads && e - r < kLgRunReads && P.read_cum[e + 1] - P.read_cum[r] <= kLgRunMops) e++;
    P.run_first.push_back(e);
    r = e;
  }
  P.n_runs = (uint32_t)P.run_first.size() - 1u;
  for (uint32_t k : oneshot::sorted_accounts(in->accounts, in->n_accounts)) P.accounts.push_back(in->accounts[k]);
  LgArena& A = P.arena;
  oneshot::Cursor c;
  const size_t nm = (size_t)P.n_mops, R = P.n_reads, FR = P.n_final_reads, FL = P.n_final_lookups;
  A.acc = c.take(sizeof(LgAcc)); A.summary = c.take(sizeof(tbc_ledger_summary));
  A.accounts = c.take(P.accounts.size() * 8); A.transfer = c.take((size_t)P.n_transfers * 8);
  A.read_lo = c.take(R * 8); A.read_cum = c.take((R + 1) * 8); A.run_first = c.take(P.run_first.size() * 4);
  A.fr_lo = c.take(FR * 8); A.fr_cum = c.take((FR + 1) * 8); A.fl_lo = c.take(FL * 8); A.fl_cum = c.take((FL + 1) * 8);
  A.mop_id = c.take(nm * 8); A.mop_a = c.take(nm * 8); A.mop_b = c.take(nm * 8); A.mop_c = c.take(nm * 8); A.mop_flags = c.take(nm);
  A.slots = c.take((size_t)P.tab_slots * sizeof(SfEncSlot));
  A.fr_unlike = c.take((FR + 3) / 4 * 4); A.fl_unlike = c.take((FL + 3) / 4 * 4);      // (whole 32-bit words: a byte is set by an atomic OR on its word)
  A.missing = c.take(FL * 4);
  A.read_error = c.take(R); A.read_total = c.take(R * 8); A.read_badness = c.take(R * 8);
  A.bytes = c.at;
  return true;
}

// the accumulators' start values
inline LgAcc acc_start() {
  LgAcc a{};
  for (int k = 0; k < 5; k++) { a.first[k] = 0xFFFFFFFFu; a.worst[k] = 0xFFFFFFFFu; }
  a.lowest = a.highest = a.first_error = 0xFFFFFFFFu;
  a.lowest_key = ~0ull;
  return a;
}

// the head of the arena as one image
inline std::vector<unsigned char> head_image(const Plan& P) {
  const LgArena& A = P.arena;
  std::vector<unsigned char> img(A.head_bytes(), 0);
  const LgAcc a = acc_start();
  const auto put = [&](const Region& r, const void* src) { oneshot::put(img, r, src); };
  put(A.acc, &a);
  put(A.accounts, P.accounts.data()); put(A.transfer, P.transfer.data());
  put(A.read_lo, P.read_lo.data()); put(A.read_cum, P.read_cum.data()); put(A.run_first, P.run_first.data());
  put(A.fr_lo, P.fr_lo.data()); put(A.fr_cum, P.fr_cum.data()); put(A.fl_lo, P.fl_lo.data()); put(A.fl_cum, P.fl_cum.data());
  return img;
}

// the kernels' arguments over an arena at `base`
inline LgArgs args(const tbc_ledger_in* in, const Plan& P, char* base) {
  const LgArena& L = P.arena;
  const auto at = [&](const Region& r) { return base + r.at; };
  LgArgs A{};
  A.acc = (LgAcc*)at(L.acc); A.summary = (tbc_ledger_summary*)at(L.summary);
  A.mop_id = (const long long*)at(L.mop_id); A.mop_a = (const long long*)at(L.mop_a); A.mop_b = (const long long*)at(L.mop_b);
  A.mop_c = (const long long*)at(L.mop_c); A.mop_flags = (const uint8_t*)at(L.mop_flags);
  A.accounts = (const long long*)at(L.accounts); A.n_accounts = in->n_accounts; A.negative_balances = in->negative_balances;
  A.total_amount = in->total_amount;
  A.read_lo = (const unsigned long long*)at(L.read_lo); A.read_cum = (const unsigned long long*)at(L.read_cum);
  A.run_first = (const uint32_t*)at(L.run_first); A.n_reads = P.n_reads; A.n_runs = P.n_runs;
  A.read_error = (uint8_t*)at(L.read_error); A.read_total = (long long*)at(L.read_total); A.read_badness = (long long*)at(L.read_badness);
  A.transfer = (const long long*)at(L.transfer); A.slots = at(L.slots); A.n_transfers = P.n_transfers; A.tab_mask = P.tab_mask;
  A.fl_lo = (const unsigned long long*)at(L.fl_lo); A.fl_cum = (const unsigned long long*)at(L.fl_cum); A.n_final_lookups = P.n_final_lookups;
  A.missing = (uint32_t*)at(L.missing);
  A.fr_lo = (const unsigned long long*)at(L.fr_lo); A.fr_cum = (const unsigned long long*)at(L.fr_cum); A.n_final_reads = P.n_final_reads;
  A.fr_unlike = (uint32_t*)at(L.fr_unlike); A.fl_unlike = (uint32_t*)at(L.fl_unlike);
  return A;
}

// The call from a finished plan to the filled `out`, over an open frame (oneshot_plan.h, "the frame interface"): the head as one image
// and the caller's micro-op columns straight to their regions, the zeroed regions, the kernels -- run.sequence(A, fr_mops, fl_mops) --,
// and the results back in one copy per array the caller asked for.
template <class Frame, class Run>
tbc_status steps(Frame& C, Run&& run, const tbc_ledger_in* in, const Plan& P, tbc_ledger_out* out) {
  const LgArena& L = P.arena;
  const std::vector<unsigned char> img = head_image(P);
  C.image(img);
  C.put(L.mop_id, in->mop_id); C.put(L.mop_a, in->mop_a); C.put(L.mop_b, in->mop_b); C.put(L.mop_c, in->mop_c); C.put(L.mop_flags, in->mop_flags);
  C.fill(L.slots, 0, L.zero_bytes());
  C.timed([&] { run.sequence(args(in, P, C.base()), P.fr_cum.back(), P.fl_cum.back()); });
  const size_t R = P.n_reads, FR = P.n_final_reads, FL = P.n_final_lookups;
  C.get(out->read_error, L.read_error, R); C.get(out->read_total, L.read_total, R * 8); C.get(out->read_badness, L.read_badness, R * 8);
  C.get(out->lookup_missing, L.missing, FL * 4);
  C.get(out->final_read_unlike, L.fr_unlike, FR); C.get(out->final_lookup_unlike, L.fl_unlike, FL);
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_summary));
  if (C.sync() != TBC_OK) return C.status;
  oneshot::account(C, out->summary);
  return TBC_OK;
}

}  // namespace lg
