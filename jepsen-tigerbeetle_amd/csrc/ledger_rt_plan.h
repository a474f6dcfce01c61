// ledger_rt_plan.h -- the host plan of tbc_ledger_realtime (realtime bounds on the posted counters, include/tbcheck.h; the rules are
// stated in jepsen/ledger.py): plain C++ with no HIP call in it.  ledger_rt_host.hip runs every call through it, and so do the emulator
// program of the kernels (tests/emu/emu_ledger_rt.cpp) and the stand-alone program of the plan (tests/emu/ledger_rt_plan.cpp).
//
//   validate   lg::validate of ledger_plan.h on the tbc_ledger_in, then the fields this entry point adds
//   plan       O(ops); it never reads a transfer's or a lookup's micro-ops (the image copies the former, blindly, and leaves the latter out).  Pairing by process (knossos.history/pair-index); per
//              invoked transfer its status; three STREAMS of rows, each in ascending position order, as (where the row's micro-ops start,
//              a running sum of the lengths, the row's position):
//                definite   the transfers that completed :ok, in COMPLETION order, position = the completion's index
//                possible   the transfers that did not fail, in invocation order, position = the invocation's index
//                reads      the :ok reads, position = the read's own index (ret); beside it the invocation's index (inv)
//              A micro-op gives two ENTRIES, credits then debits; a stream of M micro-ops is cut into chunks of whole wavefronts'
//              worth of entries.  Then the sorted accounts with `init` permuted to match, and the arena as named regions.
//   steps      the call from the plan to the filled output, over a call frame: the library's and the emulator's run this one list
#pragma once
#include <unordered_map>
#include "ledger_plan.h"

namespace lgrt {

using oneshot::Region;
using oneshot::Span;                       // (lgrt::Span, as it was named while this header held it)

constexpr uint32_t kRtNone = 0xFFFFFFFFu;
constexpr uint64_t kRtCarryWords = 1ull << 22;      // a stream's carried totals: chunks x classes at most (but one chunk at least)
constexpr uint32_t kRtChunksMax = 4096;
constexpr uint64_t kRtInitEnd = 1ull << 61;         // |init| stays below this
constexpr long long kRtAmountEnd = 1ll << 31;       // an amount is in [0, this)

enum { kDefinite = 0, kPossible = 1, kReads = 2, kStreams = 3 };

// what the kernels add up, in device memory (zeroed but for `first`, `worst`, `first_error`, which the summary kernel reads as none
// when the counts are 0)
struct RtAcc {
  uint32_t count[3], first[3], last1[3], worst[3];
  uint32_t first_error, error_count, foreign_sides, bad_amounts;
  unsigned long long worst_miss[3], n_checked;
};

// one stream as the kernels take it, every pointer into the arena.  Entry e is side e & 1 (0 credits, 1 debits) of micro-op e >> 1 of the
// stream; its class is side * n_accounts + the account's number
struct RtStream {
  const unsigned long long *lo, *cum; const uint32_t* pos;       // the rows
  uint32_t n_rows, n_chunks, chunk_entries, grid;
  unsigned long long n_entries;
  uint32_t *ent_cls, *ent_pos; unsigned long long* ent_val;       // [n_entries] what the numbering leaves
  uint32_t* carry_cnt; unsigned long long* carry_val;             // [n_chunks][n_class], zeroed
  uint32_t* off;                                                  // [n_class + 1] where each class's list starts, zeroed
  uint32_t* list_pos; unsigned long long* list_val;               // [n_entries] the lists: position, inclusive running sum / maximum (as a key)
};

struct RtArgs {
  RtAcc* acc; tbc_ledger_rt_summary* summary;
  const long long *mop_id, *mop_a, *mop_b, *mop_c; const uint8_t* mop_flags;
  const long long *accounts, *init;                               // sorted; init: [2][n_accounts] credits then debits, in that order
  uint32_t n_accounts, n_class, ok_transfers_apply, n_reads;
  const uint32_t* read_inv;                                       // [n_reads] the invocation's index, 0 if the read has none (nothing lies before either)
  unsigned long long n_read_mops;
  uint32_t grid_query, n_definite, n_possible, pad;
  RtStream s[kStreams];
  uint32_t* rt_bits;                                              // a byte per read, in whole words
  unsigned long long* rt_miss;                                    // [n_reads][3]
  long long *mop_lo, *mop_hi, *mop_floor;                         // [n_read_mops][2]
};

// Every kernel of the call on `stream` (a hipStream_t): lgrt::sequence of ledger_rt_kernels.h over the library's launcher; defined in
// ledger_rt.hip.  The grids are the sequence's to choose.
void launch(void* stream, RtArgs A);

// The call's one arena, in order: what the host makes (ONE image, one copy: the head, then the micro-op columns of the ops the kernels
// look at, gathered), what the device adds into (zeroed before the kernels), what the kernels write in full.
struct RtArena {
  Region acc, accounts, init, read_inv, row_lo[kStreams], row_cum[kStreams], row_pos[kStreams];                 // the head
  Region mop_id, mop_a, mop_b, mop_c, mop_flags;                                                                // the caller's
  Region carry_cnt[kStreams], carry_val[kStreams], off[kStreams], rt_bits, rt_miss;                             // zeroed
  Region summary, ent_cls[kStreams], ent_pos[kStreams], ent_val[kStreams], list_pos[kStreams], list_val[kStreams], mop_lo, mop_hi, mop_floor;
  size_t bytes = 0;
  size_t image_bytes() const { return carry_cnt[0].at; }
  size_t zero_bytes() const { return summary.at - carry_cnt[0].at; }
};

struct Rows {
  std::vector<uint64_t> lo, cum{0};
  std::vector<uint32_t> pos;
  uint32_t n_chunks = 0, chunk_entries = 64;
  uint64_t mops() const { return cum.back(); }
  void push(uint64_t at, uint64_t n, uint32_t p) { lo.push_back(at); cum.push_back(cum.back() + n); pos.push_back(p); }
};

// (its Spans: the micro-ops the device gets are those of the :ok reads and of the transfers that did not fail)
struct Plan : oneshot::Spans {
  uint32_t n_reads = 0, n_class = 0;
  std::vector<uint32_t> partner;                      // [n_ops] the row of the op's completion / invocation, kRtNone
  std::vector<uint8_t> status;                        // [n_ops] of an invoked transfer: the TBC_LEDGER_T_* of its completion, TBC_LEDGER_T_INVOKE = open
  Rows rows[kStreams];
  std::vector<uint32_t> read_inv;
  std::vector<int64_t> accounts, init;                // sorted; [2][n_accounts]
  RtArena arena;
};

inline bool validate(const char* fn, const tbc_ledger_rt_in* in, std::string& err) {
  if (!lg::validate(fn, &in->ledger, err)) return false;
  char buf[256];
  const auto say = [&](const char* what) { std::snprintf(buf, sizeof buf, "%s: %s", fn, what); err = buf; return false; };
  if (in->ledger.n_ops && !in->process) return say("null argument (process)");
  if (in->ok_transfers_apply > 1u) return say("ok_transfers_apply is 0 or 1");
  for (const int64_t* init : {in->init_credits, in->init_debits})
    for (uint32_t k = 0; init && k < in->ledger.n_accounts; k++)
      if (init[k] <= -(int64_t)kRtInitEnd || init[k] >= (int64_t)kRtInitEnd) {
        std::snprintf(buf, sizeof buf, "%s: the initial value of account %lld is 2^61 or more in magnitude", fn, (long long)in->ledger.accounts[k]);
        err = buf;
        return false;
      }
  return true;
}

// Pairing by process (knossos.history/pair-index), which tbc_ledger_journal's plan shares: partner[i] the row of op i's completion /
// invocation, kRtNone; status[i] of an invoked transfer the TBC_LEDGER_T_* of its completion, TBC_LEDGER_T_INVOKE = open
inline void pair(const tbc_ledger_rt_in* rin, std::vector<uint32_t>& partner, std::vector<uint8_t>& status) {
  const tbc_ledger_in* in = &rin->ledger;
  partner.assign(in->n_ops, kRtNone);
  status.assign(in->n_ops, TBC_LEDGER_T_INVOKE);
  std::unordered_map<int32_t, uint32_t> open;         // process -> its open invocation
  for (uint32_t i = 0; i < in->n_ops; i++) {
    if (in->type[i] == TBC_LEDGER_T_INVOKE) { open[rin->process[i]] = i; continue; }
    const auto it = open.find(rin->process[i]);
    if (it == open.end()) continue;
    const uint32_t inv = it->second;
    partner[inv] = i; partner[i] = inv;
    if (in->kind[inv] == TBC_LEDGER_K_TRANSFER) status[inv] = in->type[i];
    open.erase(it);
  }
}

// (the input has passed `validate`.)  false: too much for one call (`err` says what)
// chunks_cap: the most chunks a stream is cut into (the tests' emulator passes a few, so that a chunk is several wavefronts' worth)
inline bool plan(const char* fn, const tbc_ledger_rt_in* rin, Plan& P, std::string& err, uint32_t chunks_cap = kRtChunksMax) {
  const tbc_ledger_in* in = &rin->ledger;
  P = Plan{};
  pair(rin, P.partner, P.status);
  // the micro-ops the device gets, numbered in the caller's order: at[i] = where op i's begin there
  std::vector<uint64_t> at(in->n_ops, 0);
  for (uint32_t i = 0; i < in->n_ops; i++) {
    const bool transfer = in->type[i] == TBC_LEDGER_T_INVOKE && in->kind[i] == TBC_LEDGER_K_TRANSFER && P.status[i] != TBC_LEDGER_T_FAIL;
    const bool read = in->type[i] == TBC_LEDGER_T_OK && in->kind[i] == TBC_LEDGER_K_READ;
    if (!transfer && !read) continue;
    at[i] = P.push(in->mop_off[i], in->mop_off[i + 1] - in->mop_off[i]);
  }
  for (uint32_t i = 0; i < in->n_ops; i++) {
    const uint64_t n = in->mop_off[i + 1] - in->mop_off[i];
    const uint32_t inv = in->type[i] == TBC_LEDGER_T_INVOKE ? kRtNone : P.partner[i];
    if (in->type[i] == TBC_LEDGER_T_INVOKE && in->kind[i] == TBC_LEDGER_K_TRANSFER && P.status[i] != TBC_LEDGER_T_FAIL) P.rows[kPossible].push(at[i], n, in->index[i]);
    if (in->type[i] == TBC_LEDGER_T_OK && inv != kRtNone && in->kind[inv] == TBC_LEDGER_K_TRANSFER)
      P.rows[kDefinite].push(at[inv], in->mop_off[inv + 1] - in->mop_off[inv], in->index[i]);
    if (in->type[i] == TBC_LEDGER_T_OK && in->kind[i] == TBC_LEDGER_K_READ) {
      P.rows[kReads].push(at[i], n, in->index[i]);
      P.read_inv.push_back(inv == kRtNone ? 0u : in->index[inv]);
    }
  }
  if (P.rows[kPossible].mops() >= (1ull << 31) || P.rows[kReads].mops() >= (1ull << 31)) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "%s: 2^31 or more micro-ops of transfers, or of reads, in one call", fn);
    err = buf;
    return false;
  }
  P.n_reads = (uint32_t)P.rows[kReads].lo.size();
  // the accounts, sorted, and init in that order
  const uint32_t nA = in->n_accounts;
  const std::vector<uint32_t> perm = oneshot::sorted_accounts(in->accounts, nA);
  P.accounts.resize(nA); P.init.assign(2 * (size_t)nA, 0);
  for (uint32_t k = 0; k < nA; k++) {
    P.accounts[k] = in->accounts[perm[k]];
    if (rin->init_credits) P.init[k] = rin->init_credits[perm[k]];
    if (rin->init_debits) P.init[nA + k] = rin->init_debits[perm[k]];
  }
  P.n_class = 2u * nA;
  // the chunks: whole wavefronts' worth of entries, as many as keep chunks x classes carried totals within bounds
  const uint64_t chunks_max = std::max<uint64_t>(1, std::min<uint64_t>(chunks_cap, kRtCarryWords / std::max<uint32_t>(1u, P.n_class)));
  for (Rows& R : P.rows) {
    const uint64_t entries = 2 * R.mops();
    R.chunk_entries = oneshot::chunk_size(entries, chunks_max);
    R.n_chunks = (uint32_t)((entries + R.chunk_entries - 1u) / R.chunk_entries);
  }
  RtArena& A = P.arena;
  oneshot::Cursor c;
  const size_t nm = (size_t)P.n_mops, R = P.n_reads, Mr = (size_t)P.rows[kReads].mops(), C = P.n_class;
  A.acc = c.take(sizeof(RtAcc)); A.accounts = c.take((size_t)nA * 8); A.init = c.take(2 * (size_t)nA * 8); A.read_inv = c.take(R * 4);
  for (int k = 0; k < kStreams; k++) A.row_lo[k] = c.take(P.rows[k].lo.size() * 8);
  for (int k = 0; k < kStreams; k++) A.row_cum[k] = c.take(P.rows[k].cum.size() * 8);
  for (int k = 0; k < kStreams; k++) A.row_pos[k] = c.take(P.rows[k].pos.size() * 4);
  A.mop_id = c.take(nm * 8); A.mop_a = c.take(nm * 8); A.mop_b = c.take(nm * 8); A.mop_c = c.take(nm * 8); A.mop_flags = c.take(nm);
  for (int k = 0; k < kStreams; k++) A.carry_cnt[k] = c.take((size_t)P.rows[k].n_chunks * C * 4);
  for (int k = 0; k < kStreams; k++) A.carry_val[k] = c.take((size_t)P.rows[k].n_chunks * C * 8);
  for (int k = 0; k < kStreams; k++) A.off[k] = c.take((C + 1) * 4);
  A.rt_bits = c.take((R + 3) / 4 * 4); A.rt_miss = c.take(R * 3 * 8);
  A.summary = c.take(sizeof(tbc_ledger_rt_summary));
  const auto entries = [&](int k) { return 2 * (size_t)P.rows[k].mops(); };
  for (int k = 0; k < kStreams; k++) A.ent_cls[k] = c.take(entries(k) * 4);
  for (int k = 0; k < kStreams; k++) A.ent_pos[k] = c.take(entries(k) * 4);
  for (int k = 0; k < kStreams; k++) A.ent_val[k] = c.take(entries(k) * 8);
  for (int k = 0; k < kStreams; k++) A.list_pos[k] = c.take(entries(k) * 4);
  for (int k = 0; k < kStreams; k++) A.list_val[k] = c.take(entries(k) * 8);
  A.mop_lo = c.take(Mr * 16); A.mop_hi = c.take(Mr * 16); A.mop_floor = c.take(Mr * 16);
  A.bytes = c.at;
  return true;
}

// the accumulators' start values
inline RtAcc acc_start() {
  RtAcc a{};
  for (int k = 0; k < 3; k++) { a.first[k] = kRtNone; a.worst[k] = kRtNone; }
  a.first_error = kRtNone;
  return a;
}

// what the host makes, as one image: the head, and the caller's columns gathered by the plan's spans
inline std::vector<unsigned char> image(const tbc_ledger_rt_in* in, const Plan& P) {
  const RtArena& A = P.arena;
  std::vector<unsigned char> img(A.image_bytes(), 0);
  const RtAcc a = acc_start();
  const auto put = [&](const Region& r, const void* src) { oneshot::put(img, r, src); };
  put(A.acc, &a);
  put(A.accounts, P.accounts.data()); put(A.init, P.init.data()); put(A.read_inv, P.read_inv.data());
  for (int k = 0; k < kStreams; k++) { put(A.row_lo[k], P.rows[k].lo.data()); put(A.row_cum[k], P.rows[k].cum.data()); put(A.row_pos[k], P.rows[k].pos.data()); }
  const auto gather = [&](const Region& r, const void* src, size_t width) { P.gather(img, r, src, width); };
  gather(A.mop_id, in->ledger.mop_id, 8); gather(A.mop_a, in->ledger.mop_a, 8); gather(A.mop_b, in->ledger.mop_b, 8); gather(A.mop_c, in->ledger.mop_c, 8);
  gather(A.mop_flags, in->ledger.mop_flags, 1);
  return img;
}

// the kernels' arguments over an arena at `base`
inline RtArgs args(const tbc_ledger_rt_in* in, const Plan& P, char* base) {
  const RtArena& L = P.arena;
  const auto at = [&](const Region& r) { return base + r.at; };
  RtArgs A{};
  A.acc = (RtAcc*)at(L.acc); A.summary = (tbc_ledger_rt_summary*)at(L.summary);
  A.mop_id = (const long long*)at(L.mop_id); A.mop_a = (const long long*)at(L.mop_a); A.mop_b = (const long long*)at(L.mop_b);
  A.mop_c = (const long long*)at(L.mop_c); A.mop_flags = (const uint8_t*)at(L.mop_flags);
  A.accounts = (const long long*)at(L.accounts); A.init = (const long long*)at(L.init);
  A.n_accounts = in->ledger.n_accounts; A.n_class = P.n_class; A.ok_transfers_apply = in->ok_transfers_apply; A.n_reads = P.n_reads;
  A.read_inv = (const uint32_t*)at(L.read_inv); A.n_read_mops = P.rows[kReads].mops();
  A.n_definite = (uint32_t)P.rows[kDefinite].lo.size(); A.n_possible = (uint32_t)P.rows[kPossible].lo.size();
  for (int k = 0; k < kStreams; k++) {
    RtStream& S = A.s[k];
    S.lo = (const unsigned long long*)at(L.row_lo[k]); S.cum = (const unsigned long long*)at(L.row_cum[k]); S.pos = (const uint32_t*)at(L.row_pos[k]);
    S.n_rows = (uint32_t)P.rows[k].lo.size(); S.n_chunks = P.rows[k].n_chunks; S.chunk_entries = P.rows[k].chunk_entries; S.n_entries = 2 * P.rows[k].mops();
    S.ent_cls = (uint32_t*)at(L.ent_cls[k]); S.ent_pos = (uint32_t*)at(L.ent_pos[k]); S.ent_val = (unsigned long long*)at(L.ent_val[k]);
    S.carry_cnt = (uint32_t*)at(L.carry_cnt[k]); S.carry_val = (unsigned long long*)at(L.carry_val[k]); S.off = (uint32_t*)at(L.off[k]);
    S.list_pos = (uint32_t*)at(L.list_pos[k]); S.list_val = (unsigned long long*)at(L.list_val[k]);
  }
  A.rt_bits = (uint32_t*)at(L.rt_bits); A.rt_miss = (unsigned long long*)at(L.rt_miss);
  A.mop_lo = (long long*)at(L.mop_lo); A.mop_hi = (long long*)at(L.mop_hi); A.mop_floor = (long long*)at(L.mop_floor);
  return A;
}

// The call from a finished plan to the filled `out`, over an open frame (oneshot_plan.h, "the frame interface"): the head and the
// micro-op columns of the ops the kernels look at as one image in one copy, the zeroed regions, the kernels -- run.sequence(A) --, the
// summary back -- an amount out of range, which only the device has looked at, ends the call there -- and then one copy per array the
// caller asked for.
template <class Frame, class Run>
tbc_status steps(const char* fn, Frame& C, Run&& run, const tbc_ledger_rt_in* in, const Plan& P, tbc_ledger_rt_out* out) {
  const RtArena& L = P.arena;
  const std::vector<unsigned char> img = image(in, P);
  C.image(img);
  C.fill(L.carry_cnt[0], 0, L.zero_bytes());
  C.timed([&] { run.sequence(args(in, P, C.base())); });
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_rt_summary));
  if (C.sync() != TBC_OK) return C.status;
  oneshot::account(C, out->summary);
  if (out->summary.bad_amounts) return C.fail(TBC_ERR_UNSUPPORTED, "%s: %u transfer amounts are outside [0, 2^31)", fn, out->summary.bad_amounts);
  const size_t R = P.n_reads, Mr = (size_t)P.rows[kReads].mops();
  C.get(out->rt_bits, L.rt_bits, R); C.get(out->rt_miss, L.rt_miss, R * 24);
  C.get(out->mop_lo, L.mop_lo, Mr * 16); C.get(out->mop_hi, L.mop_hi, Mr * 16); C.get(out->mop_floor, L.mop_floor, Mr * 16);
  return C.sync();
}

}  // namespace lgrt
