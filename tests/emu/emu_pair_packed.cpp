// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_pair_packed.cpp: the PACKED reader of csrc/pair_kernels.h on the CPU (the very file
// hipcc compiles into libtbcheck.so; include/tbcheck.h, "the packed event word"), two ways:
//   emu_prp_batch   tbc_pair_packed_batch -- the validation, the plan and pr::steps of csrc/pair_plan.h, the list csrc/pair_host.hip
//                   runs -- over the emulator's call frame and launcher (oneshot_emu.h), grids capped at `grid_cap` workgroups;
//   emu_prp_stage   what tbc_batch_submit_events does on the device (csrc/batch_stream.hip): the arena laid out ONCE for the batch's
//                   capacities (pr::plan_batch), the three arrays of the slot copied in, the pairing, the descriptors read back,
//                   the all-or-nothing rule (pr::batch_refusal), and only then the wire columns emitted into a SEPARATE stage buffer
//                   of the caller's (pr::args_stage), which a refused call must leave as it was.
// Built as a shared object by tests/test_packed_events_emu.py (also with PR_MUTATION 3, which that test must see).  With
// EMU_PAIR_PACKED_MAIN it is a program of its own, linked with csrc/tbc_host.cpp: seeded histories packed by tbc_pack_events, through
// both entries and through tbc_pair_events over what the words decode to -- the form built with -fsanitize=address,undefined and run
// as a plain executable.  The lane shuffle the kernels use is stated here, as in emu_pair.cpp.
#include "oneshot_emu.h"

static inline uint64_t emu_shfl(uint64_t v, int src_of_me, int site) {
  const int me = (int)wv::lane_id();
  const uint64_t* s = wv::gather(v, site);
  return src_of_me >= 0 && src_of_me < 64 ? s[src_of_me] : s[me];
}
#define __shfl(v, src) ((decltype(v))emu_shfl((uint64_t)(uint32_t)(v), (int)(src), 400000 + __LINE__))

#include "pair_plan.h"
#include "pair_kernels.h"

namespace {
std::string g_err;
}  // namespace

extern "C" int emu_prp_batch(const tbc_packed_event_batch* in, tbc_pair_out* out, uint32_t grid_cap, uint64_t seed) {
  g_err.clear();
  if (!in || !out) { g_err = "emu_prp_batch: null argument"; return TBC_ERR_INVALID_ARG; }
  const tbc_status st = pr::validate("emu_prp_batch", in, out, g_err);
  if (st != TBC_OK) return st;
  pr::Plan P;
  pr::plan(in, out, P);
  struct Run {
    emu::Launcher go;
    void pair(const pr::PrArgs& A) { pr::pair_sequence(go, A); }
    void emit(const pr::PrArgs& A) { pr::emit_sequence(go, A); }
  };
  emu::Arena C(g_err);
  C.open(in->device, P.arena.bytes);
  pr::steps(C, Run{emu::Launcher(grid_cap, seed)}, "emu_prp_batch", in, P, out);
  return C.close();
}

// `in`: the slot's arrays.  The arena is that of a batch of n_hist_cap histories, events_cap events and ops_cap ops a third of the stage;
// stage: 3 * ops_cap words of the caller's.  out (op_off, n_events, n_process, status, bad_row, n_bad, n_ops): the descriptors that
// came back, whatever the call decides.
extern "C" int emu_prp_stage(const tbc_packed_event_batch* in, uint32_t n_hist_cap, uint64_t events_cap, uint64_t ops_cap, uint32_t* stage,
                             tbc_pair_out* out, uint32_t grid_cap, uint64_t seed) {
  g_err.clear();
  if (!in || !out || !stage) { g_err = "emu_prp_stage: null argument"; return TBC_ERR_INVALID_ARG; }
  tbc_status st = pr::validate_offsets("emu_prp_stage", in->n_hist, in->ev_off, nullptr, g_err);
  if (st != TBC_OK) return st;
  const uint32_t nh = in->n_hist;
  const uint64_t n = in->ev_off[nh];
  if (nh == 0 || nh > n_hist_cap || n > events_cap) { g_err = "emu_prp_stage: beyond the capacities"; return TBC_ERR_INVALID_ARG; }
  pr::Plan P;
  pr::plan_batch(n_hist_cap, events_cap, ops_cap, P);
  const pr::PrArena& L = P.arena;
  emu::Arena C(g_err);
  C.open(in->device, L.bytes);
  const pr::PrArgs A = pr::args_stage(P, nh, C.base(), stage);
  const auto part = [](const oneshot::Region& r, size_t bytes) { return oneshot::Region{r.at, bytes}; };
  C.put(part(L.ev_off, ((size_t)nh + 1) * 8), in->ev_off);
  C.put(part(L.ev_word, (size_t)n * 4), in->ev_word); C.put(part(L.process, (size_t)n * 4), in->process);
  C.fill(L.acc, 0, L.acc.bytes);
  C.fill(L.comp_of, 0xFF, (size_t)n * 4);
  emu::Launcher go(grid_cap, seed);
  pr::pair_sequence(go, A);
  pr::PrAcc acc{};
  C.get(&acc, L.acc);
  C.get(out->op_off, L.op_off, ((size_t)nh + 1) * 8); C.get(out->n_events, L.n_events, (size_t)nh * 4); C.get(out->n_process, L.n_process, (size_t)nh * 4);
  C.get(out->status, L.status, (size_t)nh * 4); C.get(out->bad_row, L.bad_row, (size_t)nh * 4);
  if (C.status != TBC_OK) return C.close();
  out->n_bad = acc.n_bad; out->n_ops = acc.total_ops;
  st = pr::batch_refusal("emu_prp_stage", nh, acc, out->status, out->bad_row, ops_cap, g_err);
  if (st != TBC_OK) { const tbc_status guard = C.close(); return guard != TBC_OK ? guard : st; }
  pr::emit_sequence(go, A);
  return C.close();
}
extern "C" const char* emu_prp_error() { return g_err.c_str(); }
extern "C" uint32_t emu_prp_mutation() {
#if defined(PR_MUTATION)
  return PR_MUTATION;
#else
  return 0u;
#endif
}

#if defined(EMU_PAIR_PACKED_MAIN)
namespace {

struct Events { std::vector<uint8_t> type, f; std::vector<int32_t> process, a, b; };

uint64_t g_rng = 0x13198A2E03707344ull;
uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }

void row(Events& e, uint32_t type, int32_t p, uint32_t f, int32_t a, int32_t b) {
  e.type.push_back((uint8_t)type); e.process.push_back(p); e.f.push_back((uint8_t)f); e.a.push_back(a); e.b.push_back(b);
}
// a value: mostly small, now and then nil, an edge of the wire format or something it does not hold
int32_t value() {
  static const int32_t edge[] = {254, 255, 256, -1, TBC_NIL, 100000};
  return rnd(10) == 0 ? edge[rnd(6)] : (int32_t)rnd(5);
}
// about `n` events over `procs` processes, well-formed unless `spoil` (one row's type made another, or a code that is none)
Events history(uint32_t n, uint32_t procs, uint32_t fail_pm, uint32_t info_pm, bool spoil, bool fits) {
  Events e;
  std::vector<int32_t> id(procs), open(procs, 0);
  for (uint32_t p = 0; p < procs; p++) id[p] = (int32_t)p * 5 - 2;
  while (e.type.size() < n) {
    const uint32_t p = rnd(procs);
    const uint32_t f = !fits && rnd(40) == 0 ? 15u + rnd(3) : rnd(3);
    if (!open[p]) { row(e, TBC_INVOKE, id[p], f, fits ? (int32_t)rnd(5) : value(), fits ? (int32_t)rnd(5) : value()); open[p] = 1; continue; }
    const uint32_t r = rnd(1000);
    if (r < fail_pm) row(e, TBC_FAIL, id[p], f, 0, 0);
    else if (r < fail_pm + info_pm) { row(e, TBC_INFO, id[p], f, 0, 0); id[p] += (int32_t)procs * 5; }
    else if (r < 900) row(e, TBC_OK_, id[p], f, fits ? (int32_t)rnd(5) : value(), fits ? (int32_t)rnd(5) : value());
    else continue;
    open[p] = 0;
  }
  if (spoil && !e.type.empty()) {
    const uint32_t at = rnd((uint32_t)e.type.size());
    e.type[at] = (uint8_t)(rnd(2) ? 4u + rnd(250) : (e.type[at] == TBC_INVOKE ? (uint32_t)TBC_OK_ : (uint32_t)TBC_INVOKE));
  }
  return e;
}

// what tbc_pair_events_batch gives with `word` asked for, from tbc_pair_events over one decoded history: the status, and the ops
struct Want { int32_t status; uint32_t n_process; std::vector<uint32_t> word, inv, ret; };
Want reference(const Events& d) {
  const uint32_t n = (uint32_t)d.type.size();
  tbc_events ev{n, d.type.data(), d.process.data(), d.f.data(), d.a.data(), d.b.data()};
  std::vector<uint8_t> f(n + 1); std::vector<int32_t> a(n + 1), b(n + 1), p(n + 1); std::vector<uint32_t> ip(n + 1), rp(n + 1);
  uint32_t k = 0, np = 0;
  Want w{};
  w.status = tbc_pair_events(&ev, f.data(), a.data(), b.data(), p.data(), ip.data(), rp.data(), &k, &np);
  if (w.status != TBC_OK) return w;
  for (uint32_t i = 0; i < k; i++) {
    const bool a_ok = a[i] == TBC_NIL || (a[i] >= 0 && a[i] <= 254), b_ok = b[i] == TBC_NIL || (b[i] >= 0 && b[i] <= 254);
    if (f[i] > 15u || !a_ok || (f[i] == TBC_F_CAS && !b_ok)) { w = Want{}; w.status = TBC_ERR_UNSUPPORTED; return w; }
    const uint32_t a8 = a[i] == TBC_NIL ? TBC_WIRE_NIL : (uint32_t)a[i], b8 = !b_ok ? 0u : (b[i] == TBC_NIL ? TBC_WIRE_NIL : (uint32_t)b[i]);
    w.word.push_back(TBC_WIRE_WORD(f[i], a8, b8, (uint32_t)p[i])); w.inv.push_back(ip[i]); w.ret.push_back(rp[i]);
  }
  w.n_process = np;
  return w;
}

}  // namespace

int main() {
  int wrong = 0;
  // round 0: histories among which some are refused (the one-shot entry answers each; the stage entry refuses the call and writes
  // nothing); round 1: histories a batch takes (the stage entry emits what the one-shot entry gives)
  for (int round = 0; round < 2; round++) {
    std::vector<Events> hs;
    for (uint32_t k = 0; k < 30; k++) hs.push_back(history(k < 8 ? k : 30u + rnd(400), 1u + rnd(k % 4 == 0 ? 80u : 9u), 100u * (k % 4), 30u * (k % 3), round == 0 && k % 5 == 4, round == 1));
    std::vector<uint32_t> words; std::vector<int32_t> process; std::vector<uint64_t> ev_off{0};
    std::vector<Want> want;
    for (const Events& e : hs) {
      const uint32_t n = (uint32_t)e.type.size();
      tbc_events ev{n, e.type.data(), e.process.data(), e.f.data(), e.a.data(), e.b.data()};
      std::vector<uint32_t> w(n + 1, 0xEEEEEEEEu);
      if (tbc_pack_events(&ev, w.data()) != TBC_OK || w[n] != 0xEEEEEEEEu) { std::printf("tbc_pack_events failed or wrote past the history\n"); return 1; }
      Events d;
      for (uint32_t i = 0; i < n; i++) row(d, TBC_EVW_TYPE(w[i]), e.process[i], TBC_EVW_F(w[i]), TBC_EVW_VALUE(TBC_EVW_A(w[i])), TBC_EVW_VALUE(TBC_EVW_B(w[i])));
      want.push_back(reference(d));
      words.insert(words.end(), w.begin(), w.begin() + n); process.insert(process.end(), e.process.begin(), e.process.end());
      ev_off.push_back(words.size());
    }
    const size_t nh = hs.size();
    std::vector<uint32_t> ww, wi, wr; std::vector<uint64_t> woff{0};
    uint32_t n_bad = 0;
    for (const Want& w : want) {
      ww.insert(ww.end(), w.word.begin(), w.word.end()); wi.insert(wi.end(), w.inv.begin(), w.inv.end()); wr.insert(wr.end(), w.ret.begin(), w.ret.end());
      woff.push_back(ww.size()); n_bad += w.status != TBC_OK;
    }
    const size_t T = ww.size();
    if ((round == 0) != (n_bad != 0)) { std::printf("round %d: %u histories refused: the generator does not make what the round is for\n", round, n_bad); return 1; }
    tbc_packed_event_batch in{(uint32_t)nh, 0, ev_off.data(), words.data(), process.data()};
    for (uint64_t seed = 1; seed <= 2; seed++) {
      std::vector<uint64_t> op_off(nh + 1); std::vector<uint32_t> n_events(nh), n_process(nh), bad_row(nh); std::vector<int32_t> status(nh);
      std::vector<uint32_t> ip(T + 1, 0xEEEEEEEEu), rp(T + 1, 0xEEEEEEEEu), word(T + 1, 0xEEEEEEEEu);
      tbc_pair_out out{};
      out.ops_cap = T; out.op_off = op_off.data(); out.n_events = n_events.data(); out.n_process = n_process.data();
      out.inv_pos = ip.data(); out.ret_pos = rp.data(); out.word = word.data(); out.status = status.data(); out.bad_row = bad_row.data();
      int st = emu_prp_batch(&in, &out, seed == 1 ? 3 : 1, seed);
      if (st != TBC_OK) { std::printf("emu_prp_batch: status %d: %s\n", st, emu_prp_error()); return 1; }
      if (out.n_ops != T || op_off != woff || out.n_bad != n_bad) { std::printf("round %d seed %llu: op_off differs (%llu ops, want %zu)\n", round, (unsigned long long)seed, (unsigned long long)out.n_ops, T); wrong++; }
      for (size_t h = 0; h < nh; h++)
        if (status[h] != want[h].status || n_process[h] != want[h].n_process || n_events[h] != hs[h].type.size() || (status[h] == TBC_ERR_BAD_HISTORY) != (bad_row[h] != TBC_PAIR_NO_ROW)) {
          std::printf("round %d seed %llu: history %zu: status %d (want %d), %u processes (want %u), bad row %u\n", round, (unsigned long long)seed, h, status[h], want[h].status, n_process[h], want[h].n_process, bad_row[h]);
          wrong++;
        }
      if (ip[T] != 0xEEEEEEEEu || rp[T] != 0xEEEEEEEEu || word[T] != 0xEEEEEEEEu) { std::printf("round %d: a word past the ops was written\n", round); wrong++; }
      ip.resize(T); rp.resize(T); word.resize(T);
      if (word != ww || ip != wi || rp != wr) { std::printf("round %d seed %llu: an op column differs\n", round, (unsigned long long)seed); wrong++; }
      // the batch's way: a larger arena, the stage of the caller's, three guard words behind it
      const uint64_t cap = T + (seed == 1 ? 0 : 5);
      std::vector<uint32_t> stage(3 * cap + 3, 0xA5A5A5A5u);
      std::vector<uint64_t> s_off(nh + 1); std::vector<uint32_t> s_ne(nh), s_np(nh), s_bad(nh); std::vector<int32_t> s_st(nh);
      tbc_pair_out so{};
      so.op_off = s_off.data(); so.n_events = s_ne.data(); so.n_process = s_np.data(); so.status = s_st.data(); so.bad_row = s_bad.data();
      st = emu_prp_stage(&in, (uint32_t)nh + 3, words.size() + 100, cap, stage.data(), &so, 3, seed);
      if (s_st != status || s_bad != bad_row || s_off != op_off || s_np != n_process) { std::printf("round %d: the stage entry's descriptors differ\n", round); wrong++; }
      bool same = true, clean = true;
      for (size_t k = 0; k < 3; k++) {
        const std::vector<uint32_t>& col = k == 0 ? ww : (k == 1 ? wi : wr);
        for (size_t i = 0; i < cap; i++) { if (i < T) same = same && stage[k * cap + i] == col[i]; else clean = clean && stage[k * cap + i] == 0xA5A5A5A5u; }
      }
      for (size_t i = 3 * cap; i < stage.size(); i++) clean = clean && stage[i] == 0xA5A5A5A5u;
      if (round == 0) {
        bool untouched = true;
        for (uint32_t x : stage) untouched = untouched && x == 0xA5A5A5A5u;
        if (st == TBC_OK || !untouched) { std::printf("round 0: a refused input was emitted (status %d)\n", st); wrong++; }
      } else if (st != TBC_OK || !same || !clean) { std::printf("round 1 seed %llu: status %d (%s), thirds %s, guards %s\n", (unsigned long long)seed, st, emu_prp_error(), same ? "equal" : "DIFFER", clean ? "intact" : "WRITTEN"); wrong++; }
    }
    std::printf("%s: round %d: %zu histories, %zu events, %zu ops, %u refused\n", wrong ? "WRONG" : "ok", round, nh, words.size(), T, n_bad);
  }
  return wrong ? 1 : 0;
}
#endif
