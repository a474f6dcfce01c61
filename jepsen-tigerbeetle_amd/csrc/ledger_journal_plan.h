// ledger_journal_plan.h -- the host plan of tbc_ledger_journal (the lookups of a ledger audited against the transfers, real time and
// the reads, include/tbcheck.h; the rules are stated in jepsen/ledger.py, "Journal audit"): plain C++ with no HIP call in it.
// ledger_journal_host.hip runs every call through it, and so do the emulator program of the kernels (tests/emu/emu_ledger_journal.cpp)
// and the stand-alone program of the plan (tests/emu/ledger_journal_plan.cpp).
//
//   validate   lgrt::validate of ledger_rt_plan.h: this entry point adds no field
//   plan       O(ops) + O(transfer micro-ops), and it reads no transfer or lookup micro-op: from mop_off it knows which op owns which
//              transfer micro-op and which lookup has which entries.  Pairing by process is lgrt::pair (ledger_rt_plan.h), shared.  Three
//              groups of the caller's columns go to the device, each gathered by spans of its own: the transfer micro-ops (numbered as
//              they lie there), the entries (lookup l's are lk_cum[l] .. lk_cum[l + 1]) -- id, a, b, c, flags: 33 B each -- and the
//              reads' micro-ops -- id, a, b, flags: 25 B.  Per transfer micro-op its owner's inv, ret and status; per lookup inv and
//              ret; per read inv and ret; the SLICES the entries kernel's workgroups take (a lookup's entries in runs of slice_entries);
//              the sorted accounts with their positions, `init` per counter; the arena as named regions.
//   steps      the call from the plan to the filled output, over a call frame: the library's and the emulator's run this one list
#pragma once
#include "ledger_rt_plan.h"

namespace lgjn {

using oneshot::Region;

constexpr uint32_t kJnNone = 0xFFFFFFFFu;
constexpr uint32_t kJnKinds = TBC_LEDGER_JN_KINDS;
constexpr uint32_t kJnWindowWords = 8192;           // the entries kernel's LDS window: the first so many words of a lookup's row of the bitmap
constexpr uint32_t kJnSliceEntries = 4096;          // entries per slice of a lookup (16 a thread of the entries kernel)
constexpr uint32_t kJnChunk = 256;                  // transfer micro-ops per chunk of the members kernel (lane = micro-op)
constexpr uint32_t kJnVecLds = 2048;                // 64-bit LDS words of the members kernel's sums per (lookup, counter); a row of more counters: global atomics
constexpr uint32_t kJnTile = 256;                   // lookups per tile of the members kernel at most

// what the kernels add up, in device memory (zeroed but for `first` and `worst`)
struct JnAcc {
  uint32_t count[kJnKinds], first[kJnKinds], last1[kJnKinds], worst[kJnKinds], worst_count[kJnKinds];
  uint32_t n_reinvoked, foreign_sides, bad_amounts;
  unsigned long long total[kJnKinds], n_checked;
};

struct JnArgs {
  JnAcc* acc; tbc_ledger_journal_summary* summary;
  // the transfer micro-ops, and per micro-op its owner
  const long long *x_id, *x_a, *x_b, *x_c; const uint8_t* x_flags;
  const uint32_t *x_inv, *x_ret; const uint8_t* x_status;         // x_ret: kJnNone where the owner has no completion
  uint32_t n_xfer, n_words;                                       // n_words = ceil(n_xfer / 32): a row of the bitmap
  void* slots /* SfEncSlot[] */; uint32_t tab_mask, ok_transfers_apply;
  // the lookups and their entries
  const long long *e_id, *e_a, *e_b, *e_c; const uint8_t* e_flags;
  const unsigned long long* lk_cum;                               // [n_lookups + 1]
  const uint32_t *lk_inv, *lk_ret;                                // lk_inv: 0 where the lookup has no invocation (nothing lies before either)
  const uint32_t* slice_cum;                                      // [n_lookups + 1] the slices of the lookups before
  uint32_t n_lookups, n_slices, slice_entries, chunk;
  unsigned long long n_entries;
  uint32_t tile, pad0;                                            // lookups per tile of the members kernel at most
  // the reads
  const long long *r_id, *r_a, *r_b; const uint8_t* r_flags;
  const unsigned long long* rd_cum;                               // [n_reads + 1]
  const uint32_t *rd_inv, *rd_ret;                                // rd_inv: 0 where the read has no invocation
  uint32_t n_reads, n_accounts, n_class, pad;
  const long long* accounts; const uint32_t* acct_pos;            // sorted; the sorted account's position in the caller's list
  const long long* init;                                          // [n_class] per counter
  // what the kernels make
  uint32_t* bitmap;                                               // [n_lookups][n_words], zeroed
  uint32_t* lk_known;                                             // [n_lookups] entries with a record, zeroed
  uint32_t* n_records;                                            // [1], zeroed
  uint8_t* entry_bits; uint32_t *lk_counts, *lk_present; long long* lk_vector;      // lk_counts, lk_present, lk_vector zeroed
  uint8_t* rd_bits; uint32_t* rd_first;
  uint32_t *xfer_present, *xfer_early, *xfer_lost, *xfer_vanished; uint8_t* xfer_flags;
};

// Every kernel of the call on `stream` (a hipStream_t): lgjn::sequence of ledger_journal_kernels.h over the library's launcher; defined in
// ledger_journal.hip.  The grids are the sequence's to choose.
void launch(void* stream, const JnArgs& A);

// The call's one arena, in order: what the host makes (ONE image, one copy: the head, then the three groups of columns, gathered), what
// starts as zeros, what the kernels write in full.
struct JnArena {
  Region acc, accounts, acct_pos, init, x_inv, x_ret, x_status, lk_cum, lk_inv, lk_ret, slice_cum, rd_cum, rd_inv, rd_ret;   // the head
  Region x_id, x_a, x_b, x_c, x_flags, e_id, e_a, e_b, e_c, e_flags, r_id, r_a, r_b, r_flags;                             // the caller's
  Region slots, bitmap, lk_known, n_records, lk_counts, lk_present, lk_vector;                                              // zeroed
  Region summary, entry_bits, rd_bits, rd_first, xfer_present, xfer_early, xfer_lost, xfer_vanished, xfer_flags;
  size_t bytes = 0;
  size_t head_bytes() const { return x_id.at; }
  size_t image_bytes() const { return slots.at; }
  size_t zero_bytes() const { return summary.at - slots.at; }
};

struct Plan {
  oneshot::Spans xf, lk, rd;                          // the micro-ops the device gets: transfers', lookups', reads'
  uint32_t n_lookups = 0, n_reads = 0, n_class = 0, n_words = 0, n_slices = 0, slice_entries = kJnSliceEntries, chunk = kJnChunk, tile = kJnTile, tab_mask = 0;
  uint64_t tab_slots = 0;
  std::vector<uint32_t> x_inv, x_ret; std::vector<uint8_t> x_status;
  std::vector<uint64_t> lk_cum{0}, rd_cum{0};
  std::vector<uint32_t> lk_inv, lk_ret, slice_cum{0}, rd_inv, rd_ret;
  std::vector<int64_t> accounts, init;                // sorted; per counter
  std::vector<uint32_t> acct_pos;
  JnArena arena;
};

inline bool validate(const char* fn, const tbc_ledger_rt_in* in, std::string& err) { return lgrt::validate(fn, in, err); }

// (the input has passed `validate`.)  false: too much for one call (`err` says what)
// slice_entries, chunk, tile: the entries of a slice of a lookup, the transfer micro-ops of a chunk of the members kernel and the lookups
// of a tile of it (the tests' emulator passes small ones, so that a lookup is several slices, the micro-ops several chunks and the
// lookups several tiles)
inline bool plan(const char* fn, const tbc_ledger_rt_in* rin, Plan& P, std::string& err, uint32_t slice_entries = kJnSliceEntries, uint32_t chunk = kJnChunk, uint32_t tile = kJnTile) {
  const tbc_ledger_in* in = &rin->ledger;
  P = Plan{};
  P.slice_entries = std::max<uint32_t>(1u, slice_entries);
  P.chunk = std::min<uint32_t>(256u, std::max<uint32_t>(64u, chunk / 64u * 64u));          // (whole wavefronts of a workgroup of 256)
  P.tile = std::min<uint32_t>(kJnTile, std::max<uint32_t>(1u, tile));
  std::vector<uint32_t> partner; std::vector<uint8_t> status;
  lgrt::pair(rin, partner, status);
  char buf[200];
  const auto refuse = [&](const char* what) { std::snprintf(buf, sizeof buf, "%s: %s in one call", fn, what); err = buf; return false; };
  for (uint32_t i = 0; i < in->n_ops; i++) {
    const uint64_t lo = in->mop_off[i], n = in->mop_off[i + 1] - lo;
    const uint32_t other = partner[i];
    if (in->type[i] == TBC_LEDGER_T_INVOKE && in->kind[i] == TBC_LEDGER_K_TRANSFER) {
      P.xf.push(lo, n);
      if (P.xf.n_mops >= (1ull << 31)) return refuse("2^31 or more transfer micro-ops");
      P.x_inv.insert(P.x_inv.end(), n, in->index[i]);
      P.x_ret.insert(P.x_ret.end(), n, other == lgrt::kRtNone ? kJnNone : in->index[other]);
      P.x_status.insert(P.x_status.end(), n, status[i]);
    } else if (in->type[i] == TBC_LEDGER_T_OK && in->kind[i] == TBC_LEDGER_K_LOOKUP) {
      if (n >= (1ull << 31)) {
        std::snprintf(buf, sizeof buf, "%s: op %u (index %u): a lookup of 2^31 or more entries", fn, i, in->index[i]);
        err = buf;
        return false;
      }
      P.lk.push(lo, n);
      P.lk_cum.push_back(P.lk.n_mops);
      P.lk_inv.push_back(other == lgrt::kRtNone ? 0u : in->index[other]); P.lk_ret.push_back(in->index[i]);
      const uint64_t slices = P.slice_cum.back() + (n + P.slice_entries - 1u) / P.slice_entries;
      if (slices >= (1ull << 31)) return refuse("2^31 or more slices of lookups");
      P.slice_cum.push_back((uint32_t)slices);
    } else if (in->type[i] == TBC_LEDGER_T_OK && in->kind[i] == TBC_LEDGER_K_READ) {
      P.rd.push(lo, n);
      P.rd_cum.push_back(P.rd.n_mops);
      P.rd_inv.push_back(other == lgrt::kRtNone ? 0u : in->index[other]); P.rd_ret.push_back(in->index[i]);
    }
  }
  P.n_lookups = (uint32_t)P.lk_inv.size(); P.n_reads = (uint32_t)P.rd_inv.size(); P.n_slices = P.slice_cum.back();
  const uint32_t nA = in->n_accounts, M = (uint32_t)P.xf.n_mops;
  P.n_class = 2u * nA; P.n_words = (M + 31u) / 32u;
  if ((uint64_t)P.n_lookups * P.n_words >= (1ull << 31)) {
    std::snprintf(buf, sizeof buf, "%s: lookups x words of transfer micro-ops (%u x %u) is 2^31 or more in one call", fn, P.n_lookups, P.n_words);
    err = buf;
    return false;
  }
  if (nA >= (1u << 30) || (uint64_t)P.n_reads * P.n_class >= (1ull << 31) || (uint64_t)P.n_lookups * P.n_class >= (1ull << 31)) {
    std::snprintf(buf, sizeof buf, "%s: reads x counters or lookups x counters (%u, %u x %llu) is 2^31 or more in one call", fn, P.n_reads, P.n_lookups, 2ull * nA);
    err = buf;
    return false;
  }
  if (P.rd.n_mops >= (1ull << 31)) return refuse("2^31 or more micro-ops of reads");
  P.acct_pos = oneshot::sorted_accounts(in->accounts, nA);
  P.accounts.resize(nA); P.init.assign(P.n_class, 0);
  for (uint32_t k = 0; k < nA; k++) {
    P.accounts[k] = in->accounts[P.acct_pos[k]];
    if (rin->init_credits) P.init[2u * k] = rin->init_credits[k];
    if (rin->init_debits) P.init[2u * k + 1u] = rin->init_debits[k];
  }
  P.tab_slots = sfenc::table_slots(M); P.tab_mask = P.tab_slots ? (uint32_t)(P.tab_slots - 1u) : 0u;
  JnArena& A = P.arena;
  oneshot::Cursor c;
  const size_t m = M, ne = (size_t)P.lk.n_mops, nr = (size_t)P.rd.n_mops, NL = P.n_lookups, R = P.n_reads, C = P.n_class;
  A.acc = c.take(sizeof(JnAcc)); A.accounts = c.take((size_t)nA * 8); A.acct_pos = c.take((size_t)nA * 4); A.init = c.take(C * 8);
  A.x_inv = c.take(m * 4); A.x_ret = c.take(m * 4); A.x_status = c.take(m);
  A.lk_cum = c.take((NL + 1) * 8); A.lk_inv = c.take(NL * 4); A.lk_ret = c.take(NL * 4); A.slice_cum = c.take((NL + 1) * 4);
  A.rd_cum = c.take((R + 1) * 8); A.rd_inv = c.take(R * 4); A.rd_ret = c.take(R * 4);
  A.x_id = c.take(m * 8); A.x_a = c.take(m * 8); A.x_b = c.take(m * 8); A.x_c = c.take(m * 8); A.x_flags = c.take(m);
  A.e_id = c.take(ne * 8); A.e_a = c.take(ne * 8); A.e_b = c.take(ne * 8); A.e_c = c.take(ne * 8); A.e_flags = c.take(ne);
  A.r_id = c.take(nr * 8); A.r_a = c.take(nr * 8); A.r_b = c.take(nr * 8); A.r_flags = c.take(nr);
  A.slots = c.take((size_t)P.tab_slots * sizeof(SfEncSlot)); A.bitmap = c.take(NL * P.n_words * 4); A.lk_known = c.take(NL * 4);
  A.n_records = c.take(4); A.lk_counts = c.take(NL * kJnKinds * 4); A.lk_present = c.take(NL * 4); A.lk_vector = c.take(NL * C * 8);
  A.summary = c.take(sizeof(tbc_ledger_journal_summary));
  A.entry_bits = c.take(ne); A.rd_bits = c.take(R); A.rd_first = c.take(R * 8);
  A.xfer_present = c.take(m * 4); A.xfer_early = c.take(m * 4); A.xfer_lost = c.take(m * 4); A.xfer_vanished = c.take(m * 4); A.xfer_flags = c.take(m);
  A.bytes = c.at;
  return true;
}

// the accumulators' start values
inline JnAcc acc_start() {
  JnAcc a{};
  for (uint32_t k = 0; k < kJnKinds; k++) a.first[k] = a.worst[k] = kJnNone;
  return a;
}

// what the host makes, as one image: the head, and the three groups of columns gathered by the plan's spans
inline std::vector<unsigned char> image(const tbc_ledger_rt_in* rin, const Plan& P) {
  const tbc_ledger_in* in = &rin->ledger;
  const JnArena& A = P.arena;
  std::vector<unsigned char> img(A.image_bytes(), 0);
  const JnAcc a = acc_start();
  const auto put = [&](const Region& r, const void* src) { oneshot::put(img, r, src); };
  put(A.acc, &a);
  put(A.accounts, P.accounts.data()); put(A.acct_pos, P.acct_pos.data()); put(A.init, P.init.data());
  put(A.x_inv, P.x_inv.data()); put(A.x_ret, P.x_ret.data()); put(A.x_status, P.x_status.data());
  put(A.lk_cum, P.lk_cum.data()); put(A.lk_inv, P.lk_inv.data()); put(A.lk_ret, P.lk_ret.data()); put(A.slice_cum, P.slice_cum.data());
  put(A.rd_cum, P.rd_cum.data()); put(A.rd_inv, P.rd_inv.data()); put(A.rd_ret, P.rd_ret.data());
  P.xf.gather(img, A.x_id, in->mop_id, 8); P.xf.gather(img, A.x_a, in->mop_a, 8); P.xf.gather(img, A.x_b, in->mop_b, 8);
  P.xf.gather(img, A.x_c, in->mop_c, 8); P.xf.gather(img, A.x_flags, in->mop_flags, 1);
  P.lk.gather(img, A.e_id, in->mop_id, 8); P.lk.gather(img, A.e_a, in->mop_a, 8); P.lk.gather(img, A.e_b, in->mop_b, 8);
  P.lk.gather(img, A.e_c, in->mop_c, 8); P.lk.gather(img, A.e_flags, in->mop_flags, 1);
  P.rd.gather(img, A.r_id, in->mop_id, 8); P.rd.gather(img, A.r_a, in->mop_a, 8); P.rd.gather(img, A.r_b, in->mop_b, 8);
  P.rd.gather(img, A.r_flags, in->mop_flags, 1);
  return img;
}

// the kernels' arguments over an arena at `base`
inline JnArgs args(const tbc_ledger_rt_in* rin, const Plan& P, char* base) {
  const JnArena& L = P.arena;
  const auto at = [&](const Region& r) { return base + r.at; };
  const auto i64 = [&](const Region& r) { return (const long long*)at(r); };
  const auto u32 = [&](const Region& r) { return (uint32_t*)at(r); };
  JnArgs A{};
  A.acc = (JnAcc*)at(L.acc); A.summary = (tbc_ledger_journal_summary*)at(L.summary);
  A.x_id = i64(L.x_id); A.x_a = i64(L.x_a); A.x_b = i64(L.x_b); A.x_c = i64(L.x_c); A.x_flags = (const uint8_t*)at(L.x_flags);
  A.x_inv = u32(L.x_inv); A.x_ret = u32(L.x_ret); A.x_status = (const uint8_t*)at(L.x_status);
  A.n_xfer = (uint32_t)P.xf.n_mops; A.n_words = P.n_words;
  A.slots = at(L.slots); A.tab_mask = P.tab_mask; A.ok_transfers_apply = rin->ok_transfers_apply;
  A.e_id = i64(L.e_id); A.e_a = i64(L.e_a); A.e_b = i64(L.e_b); A.e_c = i64(L.e_c); A.e_flags = (const uint8_t*)at(L.e_flags);
  A.lk_cum = (const unsigned long long*)at(L.lk_cum); A.lk_inv = u32(L.lk_inv); A.lk_ret = u32(L.lk_ret); A.slice_cum = u32(L.slice_cum);
  A.n_lookups = P.n_lookups; A.n_slices = P.n_slices; A.slice_entries = P.slice_entries; A.chunk = P.chunk; A.tile = P.tile; A.n_entries = P.lk.n_mops;
  A.r_id = i64(L.r_id); A.r_a = i64(L.r_a); A.r_b = i64(L.r_b); A.r_flags = (const uint8_t*)at(L.r_flags);
  A.rd_cum = (const unsigned long long*)at(L.rd_cum); A.rd_inv = u32(L.rd_inv); A.rd_ret = u32(L.rd_ret);
  A.n_reads = P.n_reads; A.n_accounts = rin->ledger.n_accounts; A.n_class = P.n_class;
  A.accounts = i64(L.accounts); A.acct_pos = u32(L.acct_pos); A.init = i64(L.init);
  A.bitmap = u32(L.bitmap); A.lk_known = u32(L.lk_known); A.n_records = u32(L.n_records);
  A.entry_bits = (uint8_t*)at(L.entry_bits); A.lk_counts = u32(L.lk_counts); A.lk_present = u32(L.lk_present); A.lk_vector = (long long*)at(L.lk_vector);
  A.rd_bits = (uint8_t*)at(L.rd_bits); A.rd_first = u32(L.rd_first);
  A.xfer_present = u32(L.xfer_present); A.xfer_early = u32(L.xfer_early); A.xfer_lost = u32(L.xfer_lost); A.xfer_vanished = u32(L.xfer_vanished);
  A.xfer_flags = (uint8_t*)at(L.xfer_flags);
  return A;
}

// The call from a finished plan to the filled `out`, over an open frame (oneshot_plan.h, "the frame interface"): the head and the three
// groups of micro-op columns as one image in one copy, the zeroed regions, the kernels -- run.sequence(A) --, the summary back -- an
// amount out of range, which only the device has looked at, ends the call there -- and then one copy per array the caller asked for.
template <class Frame, class Run>
tbc_status steps(const char* fn, Frame& C, Run&& run, const tbc_ledger_rt_in* in, const Plan& P, tbc_ledger_journal_out* out) {
  const JnArena& L = P.arena;
  const std::vector<unsigned char> img = image(in, P);
  C.image(img);
  C.fill(L.slots, 0, L.zero_bytes());
  C.timed([&] { run.sequence(args(in, P, C.base())); });
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_journal_summary));
  if (C.sync() != TBC_OK) return C.status;
  oneshot::account(C, out->summary);
  if (out->summary.bad_amounts) return C.fail(TBC_ERR_UNSUPPORTED, "%s: %u amounts of journalled transfers are outside [0, 2^31)", fn, out->summary.bad_amounts);
  const size_t M = (size_t)P.xf.n_mops, R = P.n_reads;
  C.get(out->entry_bits, L.entry_bits); C.get(out->lk_counts, L.lk_counts); C.get(out->lk_present, L.lk_present); C.get(out->lk_vector, L.lk_vector);
  C.get(out->rd_bits, L.rd_bits, R); C.get(out->rd_first, L.rd_first, R * 8);
  C.get(out->xfer_present, L.xfer_present, M * 4); C.get(out->xfer_early, L.xfer_early, M * 4); C.get(out->xfer_lost, L.xfer_lost, M * 4);
  C.get(out->xfer_vanished, L.xfer_vanished, M * 4); C.get(out->xfer_flags, L.xfer_flags, M);
  return C.sync();
}

}  // namespace lgjn
