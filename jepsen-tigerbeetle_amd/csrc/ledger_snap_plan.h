// ledger_snap_plan.h -- the host plan of tbc_ledger_snapshots (the reads of a ledger as snapshots in one order, include/tbcheck.h; the
// rules are stated in jepsen/ledger.py, "Snapshot order"): plain C++ with no HIP call in it.  ledger_snap_host.hip runs every call
// through it, and so do the emulator program of the kernels (tests/emu/emu_ledger_snap.cpp) and the stand-alone program of the plan
// (tests/emu/ledger_snap_plan.cpp).
//
//   validate   lg::validate of ledger_plan.h on the tbc_ledger_in: this entry point adds no field
//   plan       O(ops); it never reads a micro-op.  The rows of the :ok reads (a running sum of their
//              lengths), the spans of the caller's columns that hold them -- transfers' and lookups' micro-ops are not copied, and of a
//              read's only id, a, b and the flags --, the sorted accounts with each one's position in the caller's `accounts` (a counter
//              is 2 x that position + field), the chunks of the sort and of the scan, and the arena as named regions.
//              R reads x C = 2 x n_accounts counters are laid out densely: R x C < 2^31, or the call is refused.
//   steps      the call from the plan to the filled output, over a call frame: the library's and the emulator's run this one list
#pragma once
#include "ledger_plan.h"

namespace lgsn {

using oneshot::Region;
using oneshot::Span;                       // (lgsn::Span, as it was named while this header held it)

constexpr uint32_t kSnNone = 0xFFFFFFFFu;
constexpr uint32_t kSnSortChunksMax = 256;          // the sort's chunks at most: a thread sums a digit's counts down them
constexpr uint32_t kSnScanRows = 64;                // sorted reads per chunk of the prefix-maximum / suffix-minimum scan
constexpr uint32_t kSnDigits = 8;                   // the sort's passes: 8 bits of the 64-bit sum each
constexpr uint32_t kSnTile = 64;                    // reads per tile of the pair kernel
constexpr uint32_t kSnPairK = 8;                    // counters per step of the pair kernel (a candidate's, in registers)
enum { kSnPartial = 1u, kSnFlagged = 2u };         // cand_flag's bits: the read is partial; the scan flagged it

// what the kernels add up, in device memory (zeroed but for `first` and `worst`)
struct SnAcc {
  uint32_t n_partial, bad_values, n_candidates, count, first, last1, worst, worst_count;
  unsigned long long n_checked, sum_counts;
};

struct SnArgs {
  SnAcc* acc; tbc_ledger_snap_summary* summary;
  const long long *mop_id, *mop_a, *mop_b; const uint8_t* mop_flags;
  const long long* accounts; const uint32_t* acct_pos;            // sorted; the sorted account's position in the caller's list
  const unsigned long long* row_cum;                              // [n_reads + 1]: read r's micro-ops are row_cum[r] .. row_cum[r + 1] of the device's columns
  uint32_t n_accounts, n_class, n_words, n_reads;                 // n_words: 32-bit words of a read's checked bits
  unsigned long long* val; uint32_t* chk;                         // [n_reads][n_class] keys (lg_key), [n_reads][n_words]; zeroed
  uint32_t* cand_flag;                                            // [n_reads] kSnPartial | kSnFlagged; zeroed
  unsigned long long* sort_key[2]; uint32_t* sort_perm[2];        // [n_reads] each: the sort's two sides; the sorted order ends in [0]
  uint32_t *hist, *off;                                           // [sort_chunks][256]; [256] where a digit's run starts
  uint32_t sort_chunks, sort_chunk_entries, scan_rows, scan_chunks;
  unsigned long long *cmax, *cmin;                                // [scan_chunks][n_class]
  uint32_t* cand_list;                                            // [n_reads]
  uint32_t *skew_count, *skew_first, *skew_key; uint8_t* snap_flags;   // the results: [n_reads], [n_reads] (all ones at the start), [n_reads][2], [n_reads]
};

// The kernels on `stream` (a hipStream_t): lgsn::filter_sequence and lgsn::rest_sequence of ledger_snap_kernels.h over the library's
// launcher; defined in ledger_snap.hip.  launch_filter: lay out, sort, scan, the candidates -- after it acc->n_candidates and
// acc->bad_values are final; launch_rest: the pairs (n_candidates > 0 only), the keys and the summary.  The grids are the sequences' to choose.
void launch_filter(void* stream, const SnArgs& A);
void launch_rest(void* stream, const SnArgs& A, uint32_t n_candidates);

// The call's one arena, in order: what the host makes (ONE image, one copy: the head, then the reads' micro-op columns, gathered), what
// starts as zeros, what starts as all ones, what the kernels write in full.
struct SnArena {
  Region acc, accounts, acct_pos, row_cum;                                                              // the head
  Region mop_id, mop_a, mop_b, mop_flags;                                                                       // the caller's
  Region val, chk, cand_flag, skew_count;                                                                  // zeroed
  Region skew_first;                                                                                            // all ones
  Region summary, sort_key[2], sort_perm[2], hist, off, cmax, cmin, cand_list, skew_key, snap_flags;
  size_t bytes = 0;
  size_t image_bytes() const { return val.at; }
  size_t zero_bytes() const { return skew_first.at - val.at; }
  size_t ones_bytes() const { return summary.at - skew_first.at; }
};

// (its Spans: the micro-ops the device gets are those of the :ok reads)
struct Plan : oneshot::Spans {
  uint32_t n_reads = 0, n_class = 0, n_words = 0;
  std::vector<uint64_t> row_cum{0};                   // the reads' lengths summed: the device's columns hold the reads' micro-ops and nothing else
  std::vector<int64_t> accounts;                      // sorted
  std::vector<uint32_t> acct_pos;
  uint32_t sort_chunks = 0, sort_chunk_entries = 64, scan_rows = kSnScanRows, scan_chunks = 0;
  SnArena arena;
};

inline bool validate(const char* fn, const tbc_ledger_in* in, std::string& err) { return lg::validate(fn, in, err); }

// (the input has passed `validate`.)  false: too much for one call (`err` says what)
// sort_chunks_cap, scan_rows: the most chunks the sort cuts the reads into and the sorted reads per chunk of the scan (the tests' emulator
// passes small ones, so that a chunk is several wavefronts' worth and the scan's carry takes several steps)
inline bool plan(const char* fn, const tbc_ledger_in* in, Plan& P, std::string& err, uint32_t sort_chunks_cap = kSnSortChunksMax, uint32_t scan_rows = kSnScanRows) {
  P = Plan{};
  for (uint32_t i = 0; i < in->n_ops; i++) {
    if (in->type[i] != TBC_LEDGER_T_OK || in->kind[i] != TBC_LEDGER_K_READ) continue;
    P.push(in->mop_off[i], in->mop_off[i + 1] - in->mop_off[i]);
    P.row_cum.push_back(P.n_mops);
  }
  P.n_reads = (uint32_t)P.row_cum.size() - 1u;
  const uint32_t nA = in->n_accounts;
  P.n_class = 2u * nA; P.n_words = (P.n_class + 31u) / 32u;
  char buf[200];
  if (nA >= (1u << 30) || (uint64_t)P.n_reads * P.n_class >= (1ull << 31)) {
    std::snprintf(buf, sizeof buf, "%s: reads x counters (%u x %llu) is 2^31 or more in one call", fn, P.n_reads, 2ull * nA);
    err = buf;
    return false;
  }
  if (P.n_mops >= (1ull << 31)) {
    std::snprintf(buf, sizeof buf, "%s: 2^31 or more micro-ops of reads in one call", fn);
    err = buf;
    return false;
  }
  P.acct_pos = oneshot::sorted_accounts(in->accounts, nA);
  P.accounts.resize(nA);
  for (uint32_t k = 0; k < nA; k++) P.accounts[k] = in->accounts[P.acct_pos[k]];
  // the sort's chunks: whole wavefronts' worth of reads, sort_chunks_cap of them at most
  const uint64_t R = P.n_reads;
  P.sort_chunk_entries = oneshot::chunk_size(R, std::max<uint32_t>(1u, std::min(sort_chunks_cap, kSnSortChunksMax)));
  P.sort_chunks = (uint32_t)((R + P.sort_chunk_entries - 1u) / P.sort_chunk_entries);
  P.scan_rows = std::max<uint32_t>(1u, scan_rows);
  P.scan_chunks = (uint32_t)((R + P.scan_rows - 1u) / P.scan_rows);
  SnArena& A = P.arena;
  oneshot::Cursor c;
  const size_t nm = (size_t)P.n_mops, C = P.n_class;
  A.acc = c.take(sizeof(SnAcc)); A.accounts = c.take((size_t)nA * 8); A.acct_pos = c.take((size_t)nA * 4);
  A.row_cum = c.take((R + 1) * 8);
  A.mop_id = c.take(nm * 8); A.mop_a = c.take(nm * 8); A.mop_b = c.take(nm * 8); A.mop_flags = c.take(nm);
  A.val = c.take(R * C * 8); A.chk = c.take(R * P.n_words * 4); A.cand_flag = c.take(R * 4); A.skew_count = c.take(R * 4);
  A.skew_first = c.take(R * 4);
  A.summary = c.take(sizeof(tbc_ledger_snap_summary));
  for (int k = 0; k < 2; k++) A.sort_key[k] = c.take(R * 8);
  for (int k = 0; k < 2; k++) A.sort_perm[k] = c.take(R * 4);
  A.hist = c.take((size_t)P.sort_chunks * 256 * 4); A.off = c.take(256 * 4);
  A.cmax = c.take((size_t)P.scan_chunks * C * 8); A.cmin = c.take((size_t)P.scan_chunks * C * 8);
  A.cand_list = c.take(R * 4); A.skew_key = c.take(R * 8); A.snap_flags = c.take((R + 3) / 4 * 4);
  A.bytes = c.at;
  return true;
}

// the accumulators' start values
inline SnAcc acc_start() {
  SnAcc a{};
  a.first = a.worst = kSnNone;
  return a;
}

// what the host makes, as one image: the head, and the reads' columns gathered by the plan's spans
inline std::vector<unsigned char> image(const tbc_ledger_in* in, const Plan& P) {
  const SnArena& A = P.arena;
  std::vector<unsigned char> img(A.image_bytes(), 0);
  const SnAcc a = acc_start();
  const auto put = [&](const Region& r, const void* src) { oneshot::put(img, r, src); };
  put(A.acc, &a);
  put(A.accounts, P.accounts.data()); put(A.acct_pos, P.acct_pos.data()); put(A.row_cum, P.row_cum.data());
  const auto gather = [&](const Region& r, const void* src, size_t width) { P.gather(img, r, src, width); };
  gather(A.mop_id, in->mop_id, 8); gather(A.mop_a, in->mop_a, 8); gather(A.mop_b, in->mop_b, 8); gather(A.mop_flags, in->mop_flags, 1);
  return img;
}

// the kernels' arguments over an arena at `base`
inline SnArgs args(const tbc_ledger_in* in, const Plan& P, char* base) {
  const SnArena& L = P.arena;
  const auto at = [&](const Region& r) { return base + r.at; };
  SnArgs A{};
  A.acc = (SnAcc*)at(L.acc); A.summary = (tbc_ledger_snap_summary*)at(L.summary);
  A.mop_id = (const long long*)at(L.mop_id); A.mop_a = (const long long*)at(L.mop_a); A.mop_b = (const long long*)at(L.mop_b);
  A.mop_flags = (const uint8_t*)at(L.mop_flags);
  A.accounts = (const long long*)at(L.accounts); A.acct_pos = (const uint32_t*)at(L.acct_pos);
  A.row_cum = (const unsigned long long*)at(L.row_cum);
  A.n_accounts = in->n_accounts; A.n_class = P.n_class; A.n_words = P.n_words; A.n_reads = P.n_reads;
  A.val = (unsigned long long*)at(L.val); A.chk = (uint32_t*)at(L.chk); A.cand_flag = (uint32_t*)at(L.cand_flag);
  for (int k = 0; k < 2; k++) { A.sort_key[k] = (unsigned long long*)at(L.sort_key[k]); A.sort_perm[k] = (uint32_t*)at(L.sort_perm[k]); }
  A.hist = (uint32_t*)at(L.hist); A.off = (uint32_t*)at(L.off);
  A.sort_chunks = P.sort_chunks; A.sort_chunk_entries = P.sort_chunk_entries; A.scan_rows = P.scan_rows; A.scan_chunks = P.scan_chunks;
  A.cmax = (unsigned long long*)at(L.cmax); A.cmin = (unsigned long long*)at(L.cmin);
  A.cand_list = (uint32_t*)at(L.cand_list);
  A.skew_count = (uint32_t*)at(L.skew_count); A.skew_first = (uint32_t*)at(L.skew_first); A.skew_key = (uint32_t*)at(L.skew_key);
  A.snap_flags = (uint8_t*)at(L.snap_flags);
  return A;
}

// The call from a finished plan to the filled `out`, over an open frame (oneshot_plan.h, "the frame interface"): the head and the reads'
// micro-op columns as one image in one copy, the zeroed and the all-ones regions, the filter's kernels -- run.filter(A) --, the
// accumulators back -- the number of candidates decides whether a pair kernel is launched at all --, the rest of the kernels --
// run.rest(A, n_candidates) --, the summary back -- a read out of range, which only the device has looked at, ends the call there --
// and then one copy per array the caller asked for.  The two runs of kernels are timed sections of their own; ns_device is their sum.
template <class Frame, class Run>
tbc_status steps(const char* fn, Frame& C, Run&& run, const tbc_ledger_in* in, const Plan& P, tbc_ledger_snap_out* out) {
  const SnArena& L = P.arena;
  const std::vector<unsigned char> img = image(in, P);
  SnAcc acc{};
  C.image(img);
  C.fill(L.val, 0, L.zero_bytes());
  C.fill(L.skew_first, 0xFF, L.ones_bytes());
  const SnArgs A = args(in, P, C.base());
  C.timed([&] { run.filter(A); });
  C.get(&acc, L.acc, sizeof acc);
  if (C.sync() != TBC_OK) return C.status;
  C.timed([&] { run.rest(A, acc.bad_values ? 0u : acc.n_candidates); });    // (bad values: only the summary is wanted)
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_snap_summary));
  if (C.sync() != TBC_OK) return C.status;
  oneshot::account(C, out->summary);
  if (out->summary.bad_values) return C.fail(TBC_ERR_UNSUPPORTED, "%s: %u reads hold counters whose magnitudes add up to 2^63 or more", fn, out->summary.bad_values);
  const size_t R = P.n_reads;
  C.get(out->skew_count, L.skew_count, R * 4); C.get(out->skew_first, L.skew_first, R * 4);
  C.get(out->skew_key, L.skew_key, R * 8); C.get(out->snap_flags, L.snap_flags, R);
  return C.sync();
}

}  // namespace lgsn
