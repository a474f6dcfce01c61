// ledger_cycles_plan.h -- the host plan of tbc_ledger_cycles (the cycle search over monotonic-key and realtime edges of a ledger's reads,
// partial reads included, include/tbcheck.h; the rules and the reduction are stated in jepsen/ledger.py, "Cycle search"): plain C++
// with no HIP call in it.  ledger_cycles_host.hip runs every call through it, and so do the emulator program of the kernels
// (tests/emu/emu_ledger_cycles.cpp) and the stand-alone program of the plan and the kernels (tests/emu/ledger_cycles_plan.cpp).
//
//   validate   lgrt::validate of ledger_rt_plan.h on the tbc_ledger_rt_in (init_* and ok_transfers_apply are checked as there and not read)
//   plan       O(ops); the plan of tbc_ledger_snapshots (ledger_snap_plan.h) on the ledger part, unchanged -- its arena is the FIRST part
//              of this call's arena, its image the first copy --, then pairing by process (lgrt::pair) for inv(R) and ret(R) of every
//              :ok read, as index + 1 (0: the read has no invocation), and the regions of this checker after the snapshot plan's.
//              The core's two bit matrices are NOT in the arena: their size is known only when the device has counted the core.
//   steps      the call from the plan to the filled output, over a call frame: the library's and the emulator's run this one list
#pragma once
#include "ledger_rt_plan.h"
#include "ledger_snap_plan.h"

namespace lgcy {

using oneshot::Region;

constexpr uint32_t kCyNone = 0xFFFFFFFFu;
constexpr uint32_t kCyMaxRounds = 24;               // closure rounds at most: ceil(log2 m) + 1 <= 15 under TBC_LEDGER_CYCLES_MAX_CORE
constexpr uint32_t kCyTile = 64;                    // components per tile of the membership kernel

// what the kernels add up, in device memory (zeroed but for `first` and `largest`)
struct CyAcc {
  uint32_t n_core, n_cls, n_reps, n_on_cycle, n_components, first, largest, largest_size;
  uint32_t changed[kCyMaxRounds];                   // per closure round: some row grew
};

struct CyArgs {
  lgsn::SnArgs sn;                                  // the snapshot filter's: val, chk, cand_flag, the order by (sum, read number)
  CyAcc* acc; tbc_ledger_cycles_summary* summary;
  const uint32_t *inv1, *ret1;                      // [n_reads] index + 1 of the invocation (0: none) and of the read itself
  uint32_t n_reads;
  unsigned long long *sumkey, *pmax;                // [n_reads] the read's sum as a key; the prefix maximum over read numbers of U's sums
  uint32_t* state;                                  // [n_reads] TBC_LEDGER_CYC_* bits
  uint32_t *cls1, *cls_rep;                         // [n_reads] class + 1 of a clean read, 0; per class a read that holds its vector
  uint32_t *core_list, *core_pos;                   // [n_reads] the core reads ascending; a core read's place in that list
  unsigned long long* ikey[2]; uint32_t* iperm[2];  // [n_reads] each: the sort by inv1, two sides; the order ends in [0]
  uint32_t *pcls, *scls;                            // [n_reads] prefix maximum of cls1 over read numbers; suffix minimum along the inv order
  uint32_t *out_code, *in_code, *cinv, *cret;       // [n_core] 2 s_out1 - mono_out; 2 s_in1 + mono_in; inv1 and ret1 of the core read
  uint32_t* rep;                                    // [n_core] the least core read (as a place in core_list) of the read's component
  uint32_t *k_lo_code, *k_lo_ret, *k_hi_code, *k_hi_inv, *k_size, *k_label;   // [n_core] a component's, at its representative
  uint32_t *rep_list, *member_of;                   // [n_core] the representatives; [n_reads] a clean read's component, kCyNone
  uint32_t* scc; uint8_t* cyc_flags;                // the results
  uint32_t* mat[2]; uint32_t n_core, n_words;       // the two m x m bit matrices, rows of n_words 32-bit words: set once the core is counted
};

// The kernels on `stream` (a hipStream_t): the sequences of ledger_cycles_kernels.h over the library's launcher; defined in
// ledger_cycles.hip.  launch_prepare: the snapshot filter, the clean reads, the core listed -- after it acc->n_core is final;
// launch_describe (n_core > 0): classes, descriptors, the matrix in mat[0]; launch_round: one squaring mat[round & 1] -> the other,
// acc->changed[round]; launch_finish: components, members, labels, the summary (`final_side`: the matrix that holds the closure).
void launch_prepare(void* stream, const CyArgs& A);
void launch_describe(void* stream, const CyArgs& A);
void launch_round(void* stream, const CyArgs& A, uint32_t round);
void launch_finish(void* stream, const CyArgs& A, uint32_t final_side, uint32_t rounds);

struct CyArena {
  Region acc, inv1, ret1;                                                        // the head: what the host makes (one copy)
  Region summary, sumkey, pmax, state, cls1, cls_rep, core_list, core_pos, ikey[2], iperm[2], pcls, scls;
  Region out_code, in_code, cinv, cret, rep, k_lo_code, k_lo_ret, k_hi_code, k_hi_inv, k_size, k_label, rep_list, member_of, scc, cyc_flags;
  size_t bytes = 0;
  size_t head_at() const { return acc.at; }
  size_t head_bytes() const { return summary.at - acc.at; }
};

struct Plan {
  lgsn::Plan sn;
  std::vector<uint32_t> inv1, ret1;
  CyArena arena;
};

inline bool validate(const char* fn, const tbc_ledger_rt_in* in, std::string& err) { return lgrt::validate(fn, in, err); }

// (the input has passed `validate`.)  false: too much for one call (`err` says what).  sort_chunks_cap, scan_rows: the snapshot plan's knobs
inline bool plan(const char* fn, const tbc_ledger_rt_in* rin, Plan& P, std::string& err, uint32_t sort_chunks_cap = lgsn::kSnSortChunksMax, uint32_t scan_rows = lgsn::kSnScanRows) {
  const tbc_ledger_in* in = &rin->ledger;
  P = Plan{};
  if (!lgsn::plan(fn, in, P.sn, err, sort_chunks_cap, scan_rows)) return false;
  std::vector<uint32_t> partner;
  std::vector<uint8_t> status;
  lgrt::pair(rin, partner, status);
  for (uint32_t i = 0; i < in->n_ops; i++) {
    if (in->type[i] != TBC_LEDGER_T_OK || in->kind[i] != TBC_LEDGER_K_READ) continue;
    P.inv1.push_back(partner[i] == lgrt::kRtNone ? 0u : in->index[partner[i]] + 1u);     // (an index is below 2^32 - 1)
    P.ret1.push_back(in->index[i] + 1u);
  }
  CyArena& A = P.arena;
  oneshot::Cursor c;
  c.at = P.sn.arena.bytes;                                                        // (a multiple of 256)
  const size_t R = P.sn.n_reads;
  A.acc = c.take(sizeof(CyAcc)); A.inv1 = c.take(R * 4); A.ret1 = c.take(R * 4);
  A.summary = c.take(sizeof(tbc_ledger_cycles_summary));
  A.sumkey = c.take(R * 8); A.pmax = c.take(R * 8); A.state = c.take(R * 4); A.cls1 = c.take(R * 4); A.cls_rep = c.take(R * 4);
  A.core_list = c.take(R * 4); A.core_pos = c.take(R * 4);
  for (int k = 0; k < 2; k++) A.ikey[k] = c.take(R * 8);
  for (int k = 0; k < 2; k++) A.iperm[k] = c.take(R * 4);
  A.pcls = c.take(R * 4); A.scls = c.take(R * 4);
  for (Region* r : {&A.out_code, &A.in_code, &A.cinv, &A.cret, &A.rep, &A.k_lo_code, &A.k_lo_ret, &A.k_hi_code, &A.k_hi_inv, &A.k_size, &A.k_label, &A.rep_list, &A.member_of, &A.scc})
    *r = c.take(R * 4);
  A.cyc_flags = c.take((R + 3) / 4 * 4);
  A.bytes = c.at;
  return true;
}

inline CyAcc acc_start() {
  CyAcc a{};
  a.first = a.largest = kCyNone;
  return a;
}

// this checker's head as one image: the accumulators, inv1, ret1 (the snapshot plan's image is made by lgsn::image and copied first)
inline std::vector<unsigned char> head_image(const Plan& P) {
  const CyArena& A = P.arena;
  std::vector<unsigned char> img(A.head_bytes(), 0);
  const CyAcc a = acc_start();
  const auto put = [&](const Region& r, const void* src) { if (r.bytes) std::copy((const unsigned char*)src, (const unsigned char*)src + r.bytes, img.begin() + (r.at - A.head_at())); };
  put(A.acc, &a); put(A.inv1, P.inv1.data()); put(A.ret1, P.ret1.data());
  return img;
}

// the words of a row of the core's matrix, and the bytes of ONE matrix
inline uint32_t matrix_words(uint32_t n_core) { return (n_core + 31u) / 32u; }
inline size_t matrix_bytes(uint32_t n_core) { return (size_t)n_core * matrix_words(n_core) * 4u; }

// the kernels' arguments over an arena at `base` (mat, n_core, n_words: set by `with_matrix`)
inline CyArgs args(const tbc_ledger_rt_in* in, const Plan& P, char* base) {
  const CyArena& L = P.arena;
  const auto at = [&](const Region& r) { return base + r.at; };
  const auto u32 = [&](const Region& r) { return (uint32_t*)at(r); };
  CyArgs A{};
  A.sn = lgsn::args(&in->ledger, P.sn, base);
  A.acc = (CyAcc*)at(L.acc); A.summary = (tbc_ledger_cycles_summary*)at(L.summary);
  A.inv1 = u32(L.inv1); A.ret1 = u32(L.ret1); A.n_reads = P.sn.n_reads;
  A.sumkey = (unsigned long long*)at(L.sumkey); A.pmax = (unsigned long long*)at(L.pmax);
  A.state = u32(L.state); A.cls1 = u32(L.cls1); A.cls_rep = u32(L.cls_rep); A.core_list = u32(L.core_list); A.core_pos = u32(L.core_pos);
  for (int k = 0; k < 2; k++) { A.ikey[k] = (unsigned long long*)at(L.ikey[k]); A.iperm[k] = u32(L.iperm[k]); }
  A.pcls = u32(L.pcls); A.scls = u32(L.scls);
  A.out_code = u32(L.out_code); A.in_code = u32(L.in_code); A.cinv = u32(L.cinv); A.cret = u32(L.cret); A.rep = u32(L.rep);
  A.k_lo_code = u32(L.k_lo_code); A.k_lo_ret = u32(L.k_lo_ret); A.k_hi_code = u32(L.k_hi_code); A.k_hi_inv = u32(L.k_hi_inv);
  A.k_size = u32(L.k_size); A.k_label = u32(L.k_label); A.rep_list = u32(L.rep_list); A.member_of = u32(L.member_of);
  A.scc = u32(L.scc); A.cyc_flags = (uint8_t*)at(L.cyc_flags);
  return A;
}

inline CyArgs with_matrix(CyArgs A, uint32_t n_core, char* matrices) {
  A.n_core = n_core; A.n_words = matrix_words(n_core);
  A.mat[0] = (uint32_t*)matrices; A.mat[1] = (uint32_t*)(matrices + matrix_bytes(n_core));
  return A;
}

// The call from a finished plan to the filled `out`, over an open frame (oneshot_plan.h, "the frame interface"): the snapshot plan's
// image and this checker's head as two copies, the zeroed regions, the kernels that separate clean reads from the core --
// run.prepare(A) --, the accumulators back -- the core's size decides whether the call goes on (`max_core` at most), and how large the
// two bit matrices are, which are allocated only now --, the descriptors and the matrix -- run.describe(A) --, one squaring per round
// -- run.round(A, round) -- with the changed flag read back after each, the rest of the kernels -- run.finish(A, final_side, rounds)
// --, the summary back, and then one copy per array the caller asked for.  Every run of kernels is a timed section; ns_device is their
// sum.
template <class Frame, class Run>
tbc_status steps(const char* fn, Frame& C, Run&& run, const tbc_ledger_rt_in* in, const Plan& P, tbc_ledger_cycles_out* out, uint32_t max_core = TBC_LEDGER_CYCLES_MAX_CORE) {
  const lgsn::SnArena& S = P.sn.arena;
  const CyArena& L = P.arena;
  const std::vector<unsigned char> img = lgsn::image(&in->ledger, P.sn), head = head_image(P);
  lgsn::SnAcc sn_acc{};
  CyAcc acc{};
  uint32_t changed = 0;
  C.image(img);
  C.image(head, L.head_at());
  C.fill(S.val, 0, S.zero_bytes());
  CyArgs A = args(in, P, C.base());
  C.timed([&] { run.prepare(A); });
  C.get(&sn_acc, S.acc, sizeof sn_acc);
  C.get(&acc, L.acc, sizeof acc);
  if (C.sync() != TBC_OK) return C.status;
  tbc_ledger_cycles_summary& s = out->summary;
  s = tbc_ledger_cycles_summary{};
  s.read_count = P.sn.n_reads; s.n_partial = sn_acc.n_partial; s.n_core = acc.n_core; s.bad_values = sn_acc.bad_values; s.n_checked = sn_acc.n_checked;
  s.first = s.largest = kCyNone;
  oneshot::account(C, s);
  if (s.bad_values) return C.fail(TBC_ERR_UNSUPPORTED, "%s: %u reads hold counters whose magnitudes add up to 2^63 or more", fn, s.bad_values);
  if (s.n_core > max_core) return C.fail(TBC_ERR_UNSUPPORTED, "%s: %u reads are partial, skewed or contradicted by real time; the search takes %u at most", fn, s.n_core, max_core);
  uint32_t rounds = 0, final_side = 0;
  if (acc.n_core) {
    char* matrices = C.more(2 * matrix_bytes(acc.n_core));
    if (C.status != TBC_OK) return C.status;
    A = with_matrix(A, acc.n_core, matrices);
    for (;;) {
      C.timed([&] {
        if (!rounds) run.describe(A);
        run.round(A, rounds);
      });
      C.get(&changed, Region{L.acc.at + offsetof(CyAcc, changed) + 4u * rounds, 4u});
      if (C.sync() != TBC_OK) return C.status;
      final_side = (rounds & 1u) ^ 1u;
      rounds++;
      if (!changed) break;
      if (rounds == kCyMaxRounds) return C.fail(TBC_ERR_HIP, "%s: the closure did not settle in %u rounds", fn, rounds);
    }
  }
  C.timed([&] { run.finish(A, final_side, rounds); });
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_cycles_summary));
  if (C.sync() != TBC_OK) return C.status;
  oneshot::account(C, out->summary);
  const size_t R = P.sn.n_reads;
  C.get(out->scc, L.scc, R * 4); C.get(out->cyc_flags, L.cyc_flags, R);
  return C.sync();
}

}  // namespace lgcy
