// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_walk_sparse.cpp: the run-form harness of emu_walk_runs.cpp once more, for the SPARSE form of
// the front walk's phase C (csrc/open_walk_impl.h: membership by prefix-XOR of toggle events, no loop over the candidates with lane =
// front).  It adds what that form's tests ask beyond the words: the schedule counts of the form (wv::stat: chunks that took it, chunks that
// took the dense loop, trips of the emission loop, steps down twin chains, value rounds, exact compares where the static twins are
// found) and a switch that sends every chunk through the dense loop.  tests/emu/walk_sparse.py builds it with g++, also with one of the
// planted mutations (-DTBC_WALK_OFF_AFTER=0u, -DTBC_WALK_TWIN_LE, -DTBC_WALK_NO_SELF_EXCLUSION), which the tests must see fail; with
// -DEMU_WALK_RUNS_MAIN it is a program of its own (for a sanitizer build) that reads the batch from a file, as emu_walk_runs.cpp's is.
#include "emu_walk_runs.cpp"

extern "C" {

// out[0 .. 10] = chunks on the sparse form, chunks on the dense loop, emission trips, twin-chain steps, value rounds, twin-find compares,
// chunks of at most 64 / of 65 .. walk::kSparseCand / of more candidates (the last keep the dense loop), the wavefront's steps of B2's
// bucket walk and of the twin chains (the longest lane's)
void emu_walk_sparse_stats(uint64_t* out, int reset) {
  for (int i = 0; i < 11; i++) {
    out[i] = wv::stats()[walk::kStatWalkSparse + i];
    if (reset) wv::stats()[walk::kStatWalkSparse + i] = 0;
  }
}

void emu_walk_force_dense(int on) { walk::emu_force_dense() = on != 0; }

// THE COUNT FORM (tbc_internal.h kHistCount; host_tables.h build_tables(count = true)): the live calls sit on RE-USED slots -- a process takes
// the lowest free slot when it first invokes and hands it back when it crashes -- and a crashed call holds no slot: it is in no slot's
// record list, so it is none of the walk's candidates.  This is the input under which the sparse form's "one bit per word and index"
// argument has to hold with slots handed from one process to the next inside a chunk.  Arguments and result as emu_walk_runs_check's
// (run: 0 = the kernel's kWalkRun); word 0 of a lookahead record is compared without the bit count_fronts_kernel adds (bit 48: a crashed
// call of a class producing `need` is invoked by this rank), which is not the walk's.  Returns 9 for a history the count form refuses.
int emu_walk_sparse_count_check(uint32_t nh, const uint64_t* op_off, const uint32_t* n_process, const uint8_t* f, const int32_t* a, const int32_t* b,
                                const int32_t* process, const uint32_t* inv_pos, const uint32_t* ret_pos, uint32_t vpad, uint32_t flags, uint32_t run,
                                uint64_t* diag, uint64_t* counts) {
  const bool want_twn = flags & 1u, want_look = flags & 2u, branch = flags & 4u, records = flags & 8u, compact = (flags & 16u) && records;
  const uint32_t by_ret = (flags >> 16) ? (flags >> 16) : (flags & 128u) ? 2u : (flags & 64u) ? 1u : 0u;
  if (run != 0u && run != walk::kWalkRun) return 9;
  Tables T;
  if (!build_tables(nh, op_off, n_process, f, a, b, process, inv_pos, ret_pos, 1, vpad, 1, branch, compact, T, true, by_ret)) return 9;
  const uint64_t total = op_off[nh];
  const uint32_t FS = compact ? kFrontCompactWords : front_stride(vpad, 1);
  const uint32_t FW = records ? FS : vpad;
  std::vector<Hist> hist = T.hist;
  std::vector<Rec> rec;
  std::vector<uint32_t> seg, scratch(2 * total + 2, 0);
  uint32_t max_ops = 1;
  for (uint32_t h = 0; h < nh; h++) {
    const uint64_t o = op_off[h];
    const uint32_t n = (uint32_t)(op_off[h + 1] - o), W = T.hist[h].n_slots;
    max_ops = std::max(max_ops, n);
    // the slots, from the definition once more: the lowest free one at a process's first invocation, handed back when the process crashes
    std::vector<int32_t> slot(n, -1), slot_of(n_process[h] + 1, -1);
    std::vector<uint8_t> used(n_process[h] + 2, 0);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t p = (uint32_t)process[o + i];
      if (ret_pos[o + i] == TBC_POS_CRASHED) { if (slot_of[p] >= 0) { used[slot_of[p]] = 0; slot_of[p] = -1; } continue; }
      if (slot_of[p] < 0) { uint32_t sl = 0; while (used[sl]) sl++; used[sl] = 1; slot_of[p] = (int32_t)sl; }
      slot[i] = slot_of[p];
    }
    hist[h].rec_off = rec.size(); hist[h].seg_off = seg.size(); hist[h].frame_off = 2 * o;
    for (uint32_t i = 0; i < n; i++) { scratch[2 * o + i] = T.inv_rank[o + i]; scratch[2 * o + n + i] = T.ret_rank[o + i]; }
    const uint64_t r0 = rec.size();
    for (uint32_t p = 0; p < W; p++) {
      seg.push_back((uint32_t)(rec.size() - r0));
      Rec hd; hd.inv_rank = 0; hd.ret_rank = 0; hd.opidx = kInf; hd.f = kFNone; hd.a = 0; hd.b = 0; hd.cls = 0; hd.prod = kLookNone;
      rec.push_back(hd);
      for (uint32_t i = 0; i < n; i++) if (slot[i] == (int32_t)p) {
        Rec r; r.inv_rank = T.inv_rank[o + i]; r.ret_rank = T.ret_rank[o + i]; r.opidx = i; r.f = f[o + i]; r.a = a[o + i]; r.b = b[o + i];
        r.cls = rec_cls(r.f, r.a, false); r.prod = look_prod(r.f, r.a, r.b);
        rec.push_back(r);
      }
      Rec tl = hd; tl.inv_rank = kInf; tl.ret_rank = kInf;
      rec.push_back(tl);
    }
    seg.push_back((uint32_t)(rec.size() - r0));
  }
  const uint64_t kPoison = 0xA5A5A5A5A5A5A5A5ull;
  std::vector<OpRec> lst(T.lst.size() + 1, OpRec{0xA5A5A5A5u, 0xA5A5A5A5u, (int32_t)0xA5A5A5A5, (int32_t)0xA5A5A5A5});
  std::vector<uint64_t> twn(T.twn.size() + 1, kPoison), rdm(total * (FW ? FW : 1) + 1, kPoison), look(T.look.size() + 1, kPoison);
  std::vector<uint32_t> tmp(total + 1, 0xA5A5A5A5u);
  PackOpenArgs A{};
  A.hist = hist.data(); A.bh = T.bh.data(); A.f = f; A.a = a; A.b = b; A.process = process; A.scratch = scratch.data();
  A.rec = rec.data(); A.seg = seg.data(); A.chunks_per_hist = (max_ops + 63) / 64; A.branch_lists = branch ? 1u : 0u;
  A.off = T.off.data(); A.ncr = T.ncr.data(); A.lst = lst.data(); A.crashed = nullptr; A.ret_slot = T.ret_slot.data(); A.ret_op = T.ret_op.data();
  A.look = want_look ? look.data() : nullptr; A.tmp = want_look ? tmp.data() : nullptr; A.slot8 = nullptr;
  A.front_words = records ? FS : 0u; A.front_compact = compact ? 1u : 0u; A.rk8 = nullptr; A.n_hist = nh; A.mask_words = 1;
  A.twn = want_twn ? twn.data() : nullptr; A.rdm = vpad ? rdm.data() : nullptr; A.vpad = vpad; A.h0 = 0; A.list_order = by_ret;
  std::vector<uint32_t> lds(walk::walk_lds_words() + 16);
  uint64_t before[3];
  for (int i = 0; i < 3; i++) before[i] = wv::stats()[walk::kStatWalkSearch + i];
  run_all<walk::kWalkRun>(A, nh, vpad, lds);
  for (int i = 0; i < 3; i++) counts[i] = wv::stats()[walk::kStatWalkSearch + i] - before[i];
  counts[3] = 0; counts[4] = 0;
  for (uint32_t h = 0; h < nh; h++) {
    const uint32_t chunks = (T.hist[h].n_ret + 63u) / 64u;
    counts[3] += (chunks + walk::kWalkRun - 1u) / walk::kWalkRun; counts[4] += chunks;
  }
  auto fail = [&](int code, uint64_t h, uint64_t F, uint64_t i, uint64_t got, uint64_t want) { diag[0] = h; diag[1] = F; diag[2] = i; diag[3] = got; diag[4] = want; return code; };
  const uint64_t kNotTheWalks = 1ull << 48;
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
        const uint64_t want = T.rdm[(o + F) * FS + v];
        if (rdm[(o + F) * FW + v] != want) return fail(3, h, F, v, rdm[(o + F) * FW + v], want);
      }
      if (want_look) {
        const uint64_t lo = look_off(o, h, 1);
        const uint64_t want0 = T.look[lo + (uint64_t)F * 2] & ~kNotTheWalks;
        if (look[lo + (uint64_t)F * 2] != want0) return fail(4, h, F, 0, look[lo + (uint64_t)F * 2], want0);
        if (look[lo + (uint64_t)F * 2 + 1] != T.look[lo + (uint64_t)F * 2 + 1]) return fail(5, h, F, 0, look[lo + (uint64_t)F * 2 + 1], T.look[lo + (uint64_t)F * 2 + 1]);
      }
    }
    if (lst[l0 + off[R]].op != 0xA5A5A5A5u && (h + 1 == nh || T.bh[h + 1].lst_off != l0 + off[R])) return fail(1, h, R, 0, lst[l0 + off[R]].op, 0xA5A5A5A5u);
  }
  return 0;
}

}  // extern "C"
