// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  walk_harness.h: what every emulated run of the front walk (csrc/open_walk_impl.h, the very file
// hipcc compiles into libtbcheck.so) is set in, once -- emu_walk.cpp (walk_wave), emu_walk_runs.cpp (walk_run) and emu_walk_sparse.cpp (the
// count form) differ in how they drive the wavefronts and in the four choices named below, nothing else.
//   * the walk's INPUTS, built the way pack.hip and open_counts_kernel leave them: pack_kernel's per-slot record lists with their
//     sentinels (from a slot-of-op rule), the ranks, off[] / ret_slot / ret_op (host_tables.h);
//   * its OUTPUT arrays, poisoned, each with a guard entry behind it;
//   * the PackOpenArgs block;
//   * the comparison of EVERY WORD it writes -- the fronts' lists, the twin masks, the open-read rows / whole compact front records, the
//     lookahead records with their producer distances -- with the tables host_tables.h builds from the definitions.
// The choices: the slot rule and the tables' form (count_form), a mask on word 0 of a lookahead record, a status filter on the schedule counts.
#pragma once
#define TBC_EMU 1
#define __HIPCC__ 1          // tbc_internal.h's look_val / look_need / look_prod / rec_cls helpers
#include "wave_env_emu.h"
#include "../../jepsen-tigerbeetle_amd/csrc/open_walk_impl.h"

using namespace tbc;

#include "host_tables.h"

namespace {

// flags: 1 = twin masks, 2 = lookahead records, 4 = branch lists, 8 = front records (else plain rows), 16 = the compact form,
// 64 / 128 / bits 16 up = the list order (PackOpenArgs.list_order 1: a front's list in order of completion; 2: the writes last; 16 + W)
struct WalkFlags {
  bool want_twn, want_look, branch, records, compact;
  uint32_t by_ret;
  explicit WalkFlags(uint32_t flags)
      : want_twn(flags & 1u), want_look(flags & 2u), branch(flags & 4u), records(flags & 8u), compact((flags & 16u) && (flags & 8u)),
        by_ret((flags >> 16) ? (flags >> 16) : (flags & 128u) ? 2u : (flags & 64u) ? 1u : 0u) {}
};

struct WalkHarness {
  Tables T;                                   // what the walk must leave (host_tables.h), and the inputs it shares with the reference
  uint32_t nh = 0, vpad = 0, FS = 0, FW = 0;  // FS: the reference's u64 words per front (always front records); FW: the walk's
  const uint64_t* op_off = nullptr;
  bool want_twn = false, want_look = false;
  std::vector<Hist> hist;
  std::vector<Rec> rec;
  std::vector<uint32_t> seg, scratch, tmp;
  std::vector<OpRec> lst;
  std::vector<uint64_t> twn, rdm, look;
  PackOpenArgs A{};

  // The slot of each op of a history (-1: on no slot).  Plain forms: the process.  COUNT FORM (tbc_internal.h kHistCount): the live calls
  // sit on RE-USED slots -- a process takes the lowest free slot when it first invokes and hands it back when it crashes -- and a crashed
  // call holds no slot: it is in no slot's record list, so it is none of the walk's candidates.
  static std::vector<int32_t> slot_of_op(uint32_t n, uint32_t n_process, const int32_t* process, const uint32_t* ret_pos, bool count_form) {
    std::vector<int32_t> slot(n, -1);
    if (!count_form) {
      for (uint32_t i = 0; i < n; i++) slot[i] = process[i];
      return slot;
    }
    std::vector<int32_t> slot_of(n_process + 1, -1);
    std::vector<uint8_t> used(n_process + 2, 0);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t p = (uint32_t)process[i];
      if (ret_pos[i] == TBC_POS_CRASHED) { if (slot_of[p] >= 0) { used[slot_of[p]] = 0; slot_of[p] = -1; } continue; }
      if (slot_of[p] < 0) { uint32_t sl = 0; while (used[sl]) sl++; used[sl] = 1; slot_of[p] = (int32_t)sl; }
      slot[i] = slot_of[p];
    }
    return slot;
  }

  // false: bad input (or a history the count form refuses)
  bool build(uint32_t nh_, const uint64_t* op_off_, const uint32_t* n_process, const uint8_t* f, const int32_t* a, const int32_t* b,
             const int32_t* process, const uint32_t* inv_pos, const uint32_t* ret_pos, uint32_t vpad_, const WalkFlags& fl, bool count_form) {
    nh = nh_; op_off = op_off_; vpad = vpad_; want_twn = fl.want_twn; want_look = fl.want_look;
    if (!build_tables(nh, op_off, n_process, f, a, b, process, inv_pos, ret_pos, 1, vpad, 1, fl.branch, fl.compact, T, count_form, fl.by_ret)) return false;
    const uint64_t total = op_off[nh];
    FS = fl.compact ? kFrontCompactWords : front_stride(vpad, 1);
    FW = fl.records ? FS : vpad;
    // pack_kernel's record lists: per slot a head sentinel, the slot's calls in op order, a tail sentinel
    hist = T.hist;
    scratch.assign(2 * total + 2, 0);
    uint32_t max_ops = 1;
    for (uint32_t h = 0; h < nh; h++) {
      const uint64_t o = op_off[h];
      const uint32_t n = (uint32_t)(op_off[h + 1] - o), W = count_form ? T.hist[h].n_slots : n_process[h];
      max_ops = std::max(max_ops, n);
      const std::vector<int32_t> slot = slot_of_op(n, n_process[h], process + o, ret_pos + o, count_form);
      hist[h].rec_off = rec.size(); hist[h].seg_off = seg.size(); hist[h].frame_off = 2 * o;
      for (uint32_t i = 0; i < n; i++) { scratch[2 * o + i] = T.inv_rank[o + i]; scratch[2 * o + n + i] = T.ret_rank[o + i]; }
      const uint64_t r0 = rec.size();
      for (uint32_t p = 0; p < W; p++) {
        seg.push_back((uint32_t)(rec.size() - r0));
        Rec hd; hd.inv_rank = 0; hd.ret_rank = 0; hd.opidx = kInf; hd.f = kFNone; hd.a = 0; hd.b = 0; hd.cls = 0; hd.prod = kLookNone;
        rec.push_back(hd);
        for (uint32_t i = 0; i < n; i++) if (slot[i] == (int32_t)p) {
          Rec r; r.inv_rank = T.inv_rank[o + i]; r.ret_rank = T.ret_rank[o + i]; r.opidx = i; r.f = f[o + i]; r.a = a[o + i]; r.b = b[o + i];
          r.cls = rec_cls(r.f, r.a, !count_form && r.ret_rank == kInf);      // (count form: a call on a slot is live)
          r.prod = look_prod(r.f, r.a, r.b);
          rec.push_back(r);
        }
        Rec tl = hd; tl.inv_rank = kInf; tl.ret_rank = kInf;
        rec.push_back(tl);
      }
      seg.push_back((uint32_t)(rec.size() - r0));
    }
    const uint64_t kPoison = 0xA5A5A5A5A5A5A5A5ull;
    lst.assign(T.lst.size() + 1, OpRec{0xA5A5A5A5u, 0xA5A5A5A5u, (int32_t)0xA5A5A5A5, (int32_t)0xA5A5A5A5});
    twn.assign(T.twn.size() + 1, kPoison); rdm.assign(total * (FW ? FW : 1) + 1, kPoison); look.assign(T.look.size() + 1, kPoison);
    tmp.assign(total + 1, 0xA5A5A5A5u);
    A = PackOpenArgs{};
    A.hist = hist.data(); A.bh = T.bh.data(); A.f = f; A.a = a; A.b = b; A.process = process; A.scratch = scratch.data();
    A.rec = rec.data(); A.seg = seg.data(); A.chunks_per_hist = (max_ops + 63) / 64; A.branch_lists = fl.branch ? 1u : 0u;
    A.off = T.off.data(); A.ncr = T.ncr.data(); A.lst = lst.data(); A.crashed = nullptr; A.ret_slot = T.ret_slot.data(); A.ret_op = T.ret_op.data();
    A.look = want_look ? look.data() : nullptr; A.tmp = want_look ? tmp.data() : nullptr; A.slot8 = nullptr;
    A.front_words = fl.records ? FS : 0u; A.front_compact = fl.compact ? 1u : 0u; A.rk8 = nullptr; A.n_hist = nh; A.mask_words = 1;
    A.twn = want_twn ? twn.data() : nullptr; A.rdm = vpad ? rdm.data() : nullptr; A.vpad = vpad; A.h0 = 0; A.list_order = fl.by_ret;
    return true;
  }

  // a wavefront's LDS, filled with a pattern before each wavefront
  static std::vector<uint32_t> fresh_lds() { return std::vector<uint32_t>(walk::walk_lds_words() + 16); }
  static void poison_lds(std::vector<uint32_t>& lds) { std::fill(lds.begin(), lds.end(), 0xDEADBEEFu); }

  // counts[3], counts[4] = (history, run) pairs that have a front, chunks that have fronts.  live_only: not the histories the walk skips by
  // their status.
  void expected_counts(uint32_t run, bool live_only, uint64_t* counts) const {
    counts[3] = 0; counts[4] = 0;
    for (uint32_t h = 0; h < nh; h++) {
      if (live_only && (T.hist[h].status != 0 || T.bh[h].status != 0)) continue;
      const uint32_t chunks = (T.hist[h].n_ret + 63u) / 64u;
      counts[3] += (chunks + run - 1u) / run; counts[4] += chunks;
    }
  }

  // 0 when every word agrees; else a code (1 lst, 2 twn, 3 rdm, 4 look word 0, 5 look mask) with diag = {history, front, index, got, want}.
  // not_the_walks: bits of the reference's look word 0 that another kernel adds.
  int compare(uint64_t* diag, uint64_t not_the_walks = 0ull) const {
    auto fail = [&](int code, uint64_t h, uint64_t F, uint64_t i, uint64_t got, uint64_t want) { diag[0] = h; diag[1] = F; diag[2] = i; diag[3] = got; diag[4] = want; return code; };
    for (uint32_t h = 0; h < nh; h++) {
      const uint64_t o = op_off[h];
      const uint32_t R = T.hist[h].n_ret;
      const uint32_t* off = T.off.data() + T.bh[h].off_off;
      const uint64_t l0 = T.bh[h].lst_off;
      for (uint32_t F = 0; F < R; F++) {
        for (uint32_t i = off[F]; i < off[F + 1]; i++) {
          const OpRec &g = lst[l0 + i], &w = T.lst[l0 + i];
          if (g.op != w.op) return fail(1, h, F, i - off[F], g.op, w.op);
          if (g.f_slot != w.f_slot) return fail(1, h, F, i - off[F], g.f_slot, w.f_slot);
          if (g.a != w.a || g.b != w.b) return fail(1, h, F, i - off[F], (uint32_t)g.a, (uint32_t)w.a);
          if (want_twn && twn[l0 + i] != T.twn[l0 + i]) return fail(2, h, F, i - off[F], twn[l0 + i], T.twn[l0 + i]);
        }
        for (uint32_t v = 0; v < vpad; v++) {
          const uint64_t want = T.rdm[(o + F) * FS + v];      // (a compact record whole: words 6, 7 are the list location and the window of the next ranks)
          if (rdm[(o + F) * FW + v] != want) return fail(3, h, F, v, rdm[(o + F) * FW + v], want);
        }
        if (want_look) {
          const uint64_t lo = look_off(o, h, 1);
          const uint64_t want0 = T.look[lo + (uint64_t)F * 2] & ~not_the_walks;                // (with the producer distance)
          if (look[lo + (uint64_t)F * 2] != want0) return fail(4, h, F, 0, look[lo + (uint64_t)F * 2], want0);
          if (look[lo + (uint64_t)F * 2 + 1] != T.look[lo + (uint64_t)F * 2 + 1]) return fail(5, h, F, 0, look[lo + (uint64_t)F * 2 + 1], T.look[lo + (uint64_t)F * 2 + 1]);
        }
      }
      // nothing past the history's last list entry
      if (lst[l0 + off[R]].op != 0xA5A5A5A5u && (h + 1 == nh || T.bh[h + 1].lst_off != l0 + off[R])) return fail(1, h, R, 0, lst[l0 + off[R]].op, 0xA5A5A5A5u);
    }
    return 0;
  }
};

}  // namespace
