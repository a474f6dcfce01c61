// pair_kernels.h -- tbc_pair_events_batch on the MI355X (gfx950): the kernel bodies.  pair.hip compiles them into libtbcheck.so; their
// launches are pr::pair_sequence and pr::emit_sequence at the end of this file; the host plan (validation, the arena) is pair_plan.h.
// The specification is tbc_pair_events (tbc_host.cpp), history by history; the outputs are bit for bit its own.
//
// THE SPLIT.  ONE WAVEFRONT PER HISTORY (a wavefront-sized workgroup, grid-stride over the histories), which walks its history in
// chunks of 64 events, lane = event, twice.  Nothing of a history is shared between wavefronts, so nothing depends on how they are
// scheduled, no kernel holds a fence wider than the wavefront's, and a history of any length is carried by the one wavefront that owns
// it.  The state per process is in LDS, 32 KB + 16 B a workgroup: FOUR workgroups, i.e. four wavefronts, a compute unit (the word behind
// the table for INT32_MIN costs the fifth).  That is low residency for a walk that waits on memory every chunk, and it is accepted as
// such: measured, the kernels are ~5 % of a call whose time is its copies over PCIe (profiles/NOTES_pair_events.md).
//   s_key  4,096 process ids, open addressing from pr::table_hash, linear probing, claimed by a compare-and-swap.  INT32_MIN is the
//          empty word, so that one id has the entry behind the table (slot 4,096) to itself.  WHICH entry an id gets depends on the
//          order the lanes of a chunk arrive in; no output does.  A table that is full when a new id comes (or 4,096 ids and
//          INT32_MIN) is the history's TBC_ERR_UNSUPPORTED.
//   s_st   pass A: what the process's LAST event so far left -- the row of its open invocation, kPrRetired after an :info, kPrClosed;
//          pass B: the process's dense number once its first surviving op has been seen.
// In launch order -- the kernel boundary is the only ordering between them, none uses scratch:
//
//   pr_pair_kernel    PASS A, per chunk: the slot of every event's process; the lanes of the same slot by one ballot per bit of the
//                     slot number (the same-process count of pack_one_impl.h phase 4), so that an event's PREVIOUS event of its
//                     process is the nearest lower lane of its slot, else what s_st carries; from that alone whether the row is
//                     malformed (see there), the first such row of the chunk by one ballot, and the walk ends at the first chunk
//                     that has one.  A completion stores its row at its invocation's, comp_of (HBM, 0xFF before the launch); the
//                     last lane of a slot leaves the slot's state in s_st.
//                     PASS B (a well-formed history), per chunk again: an invocation reads its completion's row and type; it
//                     SURVIVES unless that is a :fail; its op index is the carried count plus the surviving lanes below it; the
//                     first surviving op of a process is the least lane that claims the slot (an LDS minimum) while the slot has no
//                     number, and the dense number is the carried count plus such lanes below -- tbc_pair_events' pass 2.  Invocation
//                     row, completion row (:ok only) and dense number go to the history's scratch at the op's index; with `word`
//                     asked for, an op the wire format cannot hold refuses the history.  Lane 0 leaves the history's descriptors.
//   pr_offsets_kernel ONE workgroup: the histories' op counts scanned, 256 a step with a carried base: op_off; the total and the
//                     histories that are not TBC_OK counted.
//   pr_emit_kernel    (launched once the host has held the total against ops_cap) a wavefront per history, lane = op: the op's
//                     columns gathered from the events through the scratch, stored at op_off[h] + op, and the wire word.
// Ballots, lane reads, the wavefront barrier and index / thread go through wave_env.h / wave_env_wg.h; the LDS atomics and the lane
// shuffle are plain HIP, which tests/emu/oneshot_emu.h and tests/emu/emu_pair.cpp state for the host emulator -- these very kernels
// run there lane by lane against tbc_pair_events (tests/test_pair_events_emu.py).  PR_MUTATION (1: a slot's carried state is not
// stored from lane 63; 2: dense numbers by first appearance among ALL invocations) exists for that test alone, which must see both.
//
// THE PACKED READER.  With PrArgs.ev_word set (a wavefront-uniform choice; tbc_pair_packed_batch, tbc_batch_submit_events) an event's
// type, f, a and b are the fields of its TBC_EVENT_WORD (include/tbcheck.h), one 4 B load where the columns take up to four; the
// process column is read as it is.  Pass A reads the word for the type; pass B reads the invocation's word once (its type, its f)
// and the completion's word for the completion's type; the wire check and the emit kernel read the word of the row whose values
// count.  The codes 7 / 16 / 256 decode to themselves -- an unknown type, an :f above 15, a value the wire format does not hold
// -- so every rule below decides as it does over the columns.  Null: the column loads are what they were.  PR_MUTATION 3 (the
// completion's type read from the INVOCATION's word) exists for tests/test_packed_events_emu.py alone.
#pragma once
#include "wave_env_wg.h"
#include "pair_plan.h"
#include "wg_scan.h"

namespace {

using pr::PrArgs;

constexpr uint32_t kPrEmpty = 0x80000000u;            // s_key: no id here (INT32_MIN itself lives at slot kPrTable)
constexpr uint32_t kPrClosed = 0xFFFFFFFFu;           // s_st, pass A: no op open (no event yet, or the last one was an :ok / :fail)
constexpr uint32_t kPrRetired = 0xFFFFFFFEu;          //               the last event was an :info
constexpr uint32_t kPrClaim = 0x10000u;               // s_st, pass B: kPrClaim + lane claims the slot's first surviving op; below: a dense number

// the slot of process id `k`: found, or claimed if `insert`.  kPrNone: the table is full of other ids (or, without insert, not there)
__device__ __forceinline__ uint32_t pr_slot(uint32_t* s_key, uint32_t k, bool insert, bool& fresh) {
  fresh = false;
  if (k == kPrEmpty) return pr::kPrTable;
  uint32_t idx = pr::table_hash(k);
  for (uint32_t t = 0; t < pr::kPrTable; t++, idx = (idx + 1u) & (pr::kPrTable - 1u)) {
    const uint32_t old = insert ? wv::lds_cas32(&s_key[idx], kPrEmpty, k) : s_key[idx];
    if (old == k) return idx;
    if (old == kPrEmpty) { fresh = insert; return insert ? idx : pr::kPrNone; }
  }
  return pr::kPrNone;
}

// the lanes that `act` and hold this lane's `slot` (13 bits): one ballot per bit
__device__ __forceinline__ unsigned long long pr_same_slot(bool act, uint32_t slot) {
  unsigned long long same = wv::ballot(act);
  for (uint32_t bit = 0; bit < 13u; bit++) {
    const bool one = ((slot >> bit) & 1u) != 0u;
    const unsigned long long m = wv::ballot(act && one);
    same &= one ? m : ~m;
  }
  return same;
}

__global__ __launch_bounds__(64) void pr_pair_kernel(PrArgs A) {
  __shared__ uint32_t s_key[pr::kPrTable];
  __shared__ uint32_t s_st[pr::kPrTable + 1u];
  const uint32_t lane = wv::wg_thread();
  const unsigned long long below = (1ull << lane) - 1ull;                   // the lanes below this one
  for (uint32_t h = wv::wg_index(); h < A.n_hist; h += A.grid) {
    const unsigned long long e0 = A.ev_off[h];
    const uint32_t n = (uint32_t)(A.ev_off[h + 1u] - e0);
    for (uint32_t i = lane; i <= pr::kPrTable; i += 64u) { if (i < pr::kPrTable) s_key[i] = kPrEmpty; s_st[i] = kPrClosed; }
    wv::barrier();
    // ---- pass A: pair, and the first malformed row.  (bad, overflow, n_distinct, special: uniform)
    uint32_t bad = pr::kPrNone, n_distinct = 0;
    bool overflow = false, special = false;
    for (uint32_t base = 0; base < n && bad == pr::kPrNone && !overflow; base += 64u) {
      const uint32_t i = base + lane;
      const bool in = i < n;
      uint32_t ty = 0, k = 0;
      if (in) { ty = A.ev_word ? TBC_EVW_TYPE(A.ev_word[e0 + i]) : (uint32_t)A.type[e0 + i]; k = (uint32_t)A.process[e0 + i]; }
      const bool known = in && ty <= TBC_INFO;
      bool fresh = false;
      const uint32_t slot = known ? pr_slot(s_key, k, true, fresh) : 0u;
      n_distinct += (uint32_t)__popcll(wv::ballot(fresh));
      if (!special && wv::ballot(known && k == kPrEmpty)) { special = true; n_distinct++; }
      overflow = wv::ballot(known && slot == pr::kPrNone) != 0ull || n_distinct > pr::kPrTable;
      if (overflow) break;                                                  // (uniform)
      const unsigned long long same = pr_same_slot(known, slot);
      // THE PREVIOUS EVENT OF THE SAME PROCESS decides the row: up to the first malformed row tbc_pair_events' open_of holds a
      // process exactly while its last event is an invocation, and `retired` holds it exactly once its last event is an :info (no
      // row after an :info of the process is well-formed, so the :info stays its last event).  So: an invocation is malformed iff
      // the previous event is an invocation (open) or an :info (retired); a completion iff there is none or it is no invocation.
      const unsigned long long lower = same & below;
      const int src = lower ? 63 - (int)__builtin_clzll(lower) : (int)lane;
      const uint32_t ty_prev = (uint32_t)__shfl((int)ty, src);
      uint32_t st = kPrClosed;
      if (known) st = lower ? (ty_prev == TBC_INVOKE ? base + (uint32_t)src : (ty_prev == TBC_INFO ? kPrRetired : kPrClosed)) : s_st[slot];
      const bool open = st < kPrRetired;
      const bool malformed = in && (!known || (ty == TBC_INVOKE ? st != kPrClosed : !open));
      const unsigned long long bm = wv::ballot(malformed);
      if (bm) { bad = base + (uint32_t)__builtin_ctzll(bm); break; }        // (uniform) the first one in history order: chunks in order, lanes in order
      if (known && ty != TBC_INVOKE) A.comp_of[e0 + st] = i;
      wv::barrier();                                                        // (every lane has read s_st)
      const bool last = known && (same >> lane) <= 1ull;                    // no higher lane of this slot
#if defined(PR_MUTATION) && PR_MUTATION == 1
      if (last && lane != 63u)
#else
      if (last)
#endif
        s_st[slot] = ty == TBC_INVOKE ? i : (ty == TBC_INFO ? kPrRetired : kPrClosed);
      wv::barrier();
    }
    int32_t status = overflow ? TBC_ERR_UNSUPPORTED : (bad != pr::kPrNone ? TBC_ERR_BAD_HISTORY : TBC_OK);
    uint32_t n_ops = 0, n_proc = 0;
    if (status == TBC_OK) {
      // ---- pass B: the surviving ops in order, their dense process numbers
      for (uint32_t i = lane; i <= pr::kPrTable; i += 64u) s_st[i] = 0xFFFFFFFFu;
      wv::barrier();
      bool wire_bad = false;
      for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t i = base + lane;
        uint32_t wi = 0;                                                    // (packed) this row's word
        if (A.ev_word && i < n) wi = A.ev_word[e0 + i];
        const bool inv = i < n && (A.ev_word ? TBC_EVW_TYPE(wi) : (uint32_t)A.type[e0 + i]) == TBC_INVOKE;
        uint32_t c = pr::kPrNone, cty = TBC_INVOKE, slot = 0;
        if (inv) {
          bool fresh;
          c = A.comp_of[e0 + i];
#if defined(PR_MUTATION) && PR_MUTATION == 3
          if (c != pr::kPrNone) cty = A.ev_word ? TBC_EVW_TYPE(wi) : (uint32_t)A.type[e0 + c];
#else
          if (c != pr::kPrNone) cty = A.ev_word ? TBC_EVW_TYPE(A.ev_word[e0 + c]) : (uint32_t)A.type[e0 + c];
#endif
          slot = pr_slot(s_key, (uint32_t)A.process[e0 + i], false, fresh);
          if (slot > pr::kPrTable) slot = pr::kPrTable;                     // (pass A entered every id: never)
        }
        const bool survives = inv && cty != TBC_FAIL;
        const uint32_t ret = cty == TBC_OK_ ? c : TBC_POS_CRASHED;
        const unsigned long long sm = wv::ballot(survives);
        const uint32_t op = n_ops + (uint32_t)__popcll(sm & below);
#if defined(PR_MUTATION) && PR_MUTATION == 2
        const bool numbered = inv;
#else
        const bool numbered = survives;
#endif
        if (numbered) atomicMin(&s_st[slot], kPrClaim + lane);              // (a slot that has its number keeps it: numbers are below kPrClaim)
        wv::barrier();
        const bool first = numbered && s_st[slot] == kPrClaim + lane;
        const unsigned long long fm = wv::ballot(first);
        wv::barrier();                                                      // (every lane has read the claims)
        if (first) s_st[slot] = n_proc + (uint32_t)__popcll(fm & below);
        wv::barrier();
        if (survives) {
          A.s_inv[e0 + op] = i; A.s_ret[e0 + op] = ret; A.s_proc[e0 + op] = s_st[slot];
        }
        if (A.want_word) {                                                  // (uniform) what tbc_batch_reload refuses
          bool unfit = false;
          if (survives) {
            const unsigned long long v = e0 + (ret != TBC_POS_CRASHED ? ret : i);
            uint32_t f;
            int32_t a, b;
            if (A.ev_word) {
              const uint32_t wv_ = ret != TBC_POS_CRASHED ? A.ev_word[v] : wi;
              f = TBC_EVW_F(wi); a = TBC_EVW_VALUE(TBC_EVW_A(wv_)); b = TBC_EVW_VALUE(TBC_EVW_B(wv_));
            } else {
              f = A.f[e0 + i]; a = A.a[v]; b = A.b[v];
            }
            const bool a_ok = a == TBC_NIL || (a >= 0 && a <= 254), b_ok = b == TBC_NIL || (b >= 0 && b <= 254);
            unfit = f > 15u || !a_ok || (f == TBC_F_CAS && !b_ok);
          }
          wire_bad = wire_bad || wv::ballot(unfit) != 0ull;
        }
        n_ops += (uint32_t)__popcll(sm); n_proc += (uint32_t)__popcll(fm);
        wv::barrier();                                                      // (the numbers are read before the next chunk's claims)
      }
      if (wire_bad) status = TBC_ERR_UNSUPPORTED;
    }
    if (status != TBC_OK) { n_ops = 0; n_proc = 0; }
    if (lane == 0u) {
      A.cnt[h] = n_ops; A.n_process[h] = n_proc; A.n_events[h] = n; A.status[h] = status;
      A.bad_row[h] = status == TBC_ERR_BAD_HISTORY ? bad : pr::kPrNone;
    }
    wv::barrier();                                                          // (the tables are reset only when every lane is done with them)
  }
}

__global__ __launch_bounds__(256) void pr_offsets_kernel(PrArgs A) {          // (one workgroup)
  __shared__ unsigned long long s_scan[256];
  __shared__ uint32_t s_bad;
  const uint32_t t = wv::wg_thread();
  if (t == 0u) { s_bad = 0u; A.op_off[0] = 0ull; }
  wv::wg_barrier();
  unsigned long long base = 0;
  uint32_t n_bad = 0;
  for (uint32_t h0 = 0; h0 < A.n_hist; h0 += 256u) {
    const uint32_t h = h0 + t;
    const bool in = h < A.n_hist;
    const unsigned long long v = in ? A.cnt[h] : 0u;
    unsigned long long total;
    const unsigned long long ex = wg_scan_excl(v, s_scan, t, 0ull, total, [](unsigned long long a, unsigned long long b) { return a + b; });
    if (in) { A.op_off[h + 1u] = base + ex + v; n_bad += A.status[h] != TBC_OK ? 1u : 0u; }
    base += total;
  }
  if (n_bad) atomicAdd(&s_bad, n_bad);
  wv::wg_barrier();
  if (t == 0u) { A.acc->total_ops = base; A.acc->n_bad = s_bad; }
}

__global__ __launch_bounds__(64) void pr_emit_kernel(PrArgs A) {
  const uint32_t lane = wv::wg_thread();
  for (uint32_t h = wv::wg_index(); h < A.n_hist; h += A.grid) {
    const unsigned long long e0 = A.ev_off[h], o0 = A.op_off[h];
    const uint32_t n = A.cnt[h];
    for (uint32_t k = lane; k < n; k += 64u) {
      const unsigned long long o = o0 + k;
      if (o >= A.out_cap) continue;                                         // (the host has held the total against the capacity: never)
      const uint32_t inv = A.s_inv[e0 + k], ret = A.s_ret[e0 + k], proc = A.s_proc[e0 + k];
      const unsigned long long v = e0 + (ret != TBC_POS_CRASHED ? ret : inv);   // an :ok completion's values replace the invocation's
      uint32_t f;
      int32_t a, b;
      if (A.ev_word) {                                                      // (uniform)
        const uint32_t wv_ = A.ev_word[v];
        f = TBC_EVW_F(ret != TBC_POS_CRASHED ? A.ev_word[e0 + inv] : wv_); a = TBC_EVW_VALUE(TBC_EVW_A(wv_)); b = TBC_EVW_VALUE(TBC_EVW_B(wv_));
      } else {
        f = A.f[e0 + inv]; a = A.a[v]; b = A.b[v];
      }
      if (A.o_f) A.o_f[o] = (uint8_t)f;
      if (A.o_a) A.o_a[o] = a;
      if (A.o_b) A.o_b[o] = b;
      if (A.o_process) A.o_process[o] = (int32_t)proc;
      if (A.o_inv) A.o_inv[o] = inv;
      if (A.o_ret) A.o_ret[o] = ret;
      if (A.o_word) {                                                       // as tbc_batch_reload encodes it (batch_stream.hip)
        const bool b_ok = b == TBC_NIL || (b >= 0 && b <= 254);
        const uint32_t a8 = a == TBC_NIL ? TBC_WIRE_NIL : (uint32_t)a, b8 = !b_ok ? 0u : (b == TBC_NIL ? TBC_WIRE_NIL : (uint32_t)b);
        A.o_word[o] = TBC_WIRE_WORD(f, a8, b8, proc);
      }
    }
  }
}

}  // namespace

namespace pr {

// The kernels of the call in order, over a launcher (oneshot_plan.h): THE statement of the launches -- the library runs them over a
// stream (pair.hip), the tests over the emulator.  The pairing and the scan of the op counts; then, once the host has read the total,
// the op columns.  A call without histories still has its op_off[0] and its (zero) total from the scan.
template <class Launcher>
void pair_sequence(Launcher& go, PrArgs A) {
  if (A.n_hist) {
    A.grid = go.grid(A.n_hist, 8192u);
    go.launch(pr_pair_kernel, A.grid, 64u, A);
  }
  A.grid = go.grid(1u, 1u);
  go.launch(pr_offsets_kernel, A.grid, 256u, A);
}

template <class Launcher>
void emit_sequence(Launcher& go, PrArgs A) {
  if (!A.n_hist) return;
  A.grid = go.grid(A.n_hist, 8192u);
  go.launch(pr_emit_kernel, A.grid, 64u, A);
}

}  // namespace pr
