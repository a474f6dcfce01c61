// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_pair.cpp: tbc_pair_events_batch on the CPU -- the validation and the host plan of
// csrc/pair_plan.h, the steps of the call as pr::steps of that header states them -- the list csrc/pair_host.hip runs -- over the
// emulator's call frame, and the kernels of csrc/pair_kernels.h (the very file hipcc compiles into libtbcheck.so) under the wavefront /
// workgroup emulator, launched by pr::pair_sequence / pr::emit_sequence of that file over the emulator's launcher (oneshot_emu.h).
// Every grid that strides is capped at `grid_cap` workgroups, so that the strides run and a workgroup's tables are used again.
// Built as a shared object by tests/test_pair_events_emu.py (also with PR_MUTATION 1 and 2, which that test must see), which compares
// what comes back with tbc_pair_events history by history.  With EMU_PAIR_MAIN it is a program of its own (linked with
// csrc/tbc_host.cpp, the specification): seeded histories, well-formed and malformed, through the emulator and through
// tbc_pair_events, every array compared -- the form that is built with -fsanitize=address,undefined and run as a plain executable.
// The lane shuffle the kernels use is stated here.
#include "oneshot_emu.h"

// a lane shuffle is a rendezvous: every lane deposits, each reads its partner's deposit
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

// TBC_OK: done; otherwise the status the library gives (emu_pr_error says why)
extern "C" int emu_pr_batch(const tbc_event_batch* in, tbc_pair_out* out, uint32_t grid_cap, uint64_t seed) {
  g_err.clear();
  if (!in || !out) { g_err = "emu_pr_batch: null argument"; return TBC_ERR_INVALID_ARG; }
  const tbc_status st = pr::validate("emu_pr_batch", in, out, g_err);
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
  pr::steps(C, Run{emu::Launcher(grid_cap, seed)}, "emu_pr_batch", in, P, out);
  return C.close();
}
extern "C" const char* emu_pr_error() { return g_err.c_str(); }
extern "C" uint32_t emu_pr_hash(uint32_t k) { return pr::table_hash(k); }
extern "C" uint32_t emu_pr_mutation() {
#if defined(PR_MUTATION)
  return PR_MUTATION;
#else
  return 0u;
#endif
}

#if defined(EMU_PAIR_MAIN)
namespace {

struct Events { std::vector<uint8_t> type, f; std::vector<int32_t> process, a, b; };

uint64_t g_rng = 0x243F6A8885A308D3ull;
uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }

void row(Events& e, uint32_t type, int32_t p, uint32_t f, int32_t a, int32_t b) {
  e.type.push_back((uint8_t)type); e.process.push_back(p); e.f.push_back((uint8_t)f); e.a.push_back(a); e.b.push_back(b);
}

// a well-formed history of about `n` events over `procs` processes (a crashed one comes back as p + procs, as Jepsen numbers it);
// `spoil`: one row is made malformed
Events history(uint32_t n, uint32_t procs, uint32_t fail_pm, uint32_t info_pm, bool spoil) {
  Events e;
  std::vector<int32_t> id(procs), open(procs, 0);
  for (uint32_t p = 0; p < procs; p++) id[p] = (int32_t)p * 7 - 3;
  while (e.type.size() < n) {
    const uint32_t p = rnd(procs);
    if (!open[p]) { row(e, TBC_INVOKE, id[p], rnd(3), rnd(2) ? TBC_NIL : (int32_t)rnd(5), (int32_t)rnd(5)); open[p] = 1; continue; }
    const uint32_t r = rnd(1000);
    if (r < fail_pm) row(e, TBC_FAIL, id[p], rnd(3), 0, 0);
    else if (r < fail_pm + info_pm) { row(e, TBC_INFO, id[p], rnd(3), 0, 0); id[p] += (int32_t)procs * 7; }
    else if (r < 900) row(e, TBC_OK_, id[p], rnd(3), (int32_t)rnd(5), (int32_t)rnd(5));
    else continue;                                                          // (stays open a while)
    open[p] = 0;
  }
  if (spoil && !e.type.empty()) {
    const uint32_t at = rnd((uint32_t)e.type.size());
    e.type[at] = (uint8_t)(rnd(2) ? 9u : (e.type[at] == TBC_INVOKE ? (uint32_t)TBC_OK_ : (uint32_t)TBC_INVOKE));
  }
  return e;
}

}  // namespace

int main() {
  std::vector<Events> hs;
  for (uint32_t k = 0; k < 40; k++) hs.push_back(history(k < 10 ? k : 30u + rnd(500), 1u + rnd(k % 4 == 0 ? 90u : 9u), 100u * (k % 4), 30u * (k % 3), k % 5 == 4));
  hs.push_back(history(9000, 4096, 50, 0, false));
  Events cat;
  std::vector<uint64_t> ev_off{0};
  for (const Events& e : hs) {
    cat.type.insert(cat.type.end(), e.type.begin(), e.type.end()); cat.f.insert(cat.f.end(), e.f.begin(), e.f.end());
    cat.process.insert(cat.process.end(), e.process.begin(), e.process.end());
    cat.a.insert(cat.a.end(), e.a.begin(), e.a.end()); cat.b.insert(cat.b.end(), e.b.begin(), e.b.end());
    ev_off.push_back(cat.type.size());
  }
  // the specification, history by history
  const size_t nh = hs.size(), N = cat.type.size();
  std::vector<uint8_t> wf; std::vector<int32_t> wa, wb, wp; std::vector<uint32_t> wi, wr, wn(nh), wproc(nh); std::vector<int32_t> wst(nh);
  std::vector<uint64_t> woff{0};
  for (size_t h = 0; h < nh; h++) {
    const Events& e = hs[h];
    const uint32_t n = (uint32_t)e.type.size();
    tbc_events ev{n, e.type.data(), e.process.data(), e.f.data(), e.a.data(), e.b.data()};
    std::vector<uint8_t> f(n + 1); std::vector<int32_t> a(n + 1), b(n + 1), p(n + 1); std::vector<uint32_t> ip(n + 1), rp(n + 1);
    uint32_t k = 0, np = 0;
    wst[h] = tbc_pair_events(&ev, f.data(), a.data(), b.data(), p.data(), ip.data(), rp.data(), &k, &np);
    if (wst[h] != TBC_OK) { k = 0; np = 0; }
    wf.insert(wf.end(), f.begin(), f.begin() + k); wa.insert(wa.end(), a.begin(), a.begin() + k); wb.insert(wb.end(), b.begin(), b.begin() + k);
    wp.insert(wp.end(), p.begin(), p.begin() + k); wi.insert(wi.end(), ip.begin(), ip.begin() + k); wr.insert(wr.end(), rp.begin(), rp.begin() + k);
    wn[h] = k; wproc[h] = np; woff.push_back(wf.size());
  }
  const size_t T = wf.size();
  int wrong = 0;
  for (uint64_t seed = 1; seed <= 2; seed++) {
    tbc_event_batch in{(uint32_t)nh, 0, ev_off.data(), cat.type.data(), cat.process.data(), cat.f.data(), cat.a.data(), cat.b.data()};
    std::vector<uint64_t> op_off(nh + 1); std::vector<uint32_t> n_events(nh), n_process(nh), bad_row(nh); std::vector<int32_t> status(nh);
    std::vector<uint8_t> f(T + 1, 0xEE); std::vector<int32_t> a(T + 1), b(T + 1), p(T + 1); std::vector<uint32_t> ip(T + 1), rp(T + 1), word(T + 1, 0xEEEEEEEEu);
    tbc_pair_out out{};
    out.ops_cap = T; out.op_off = op_off.data(); out.n_events = n_events.data(); out.n_process = n_process.data();
    out.f = f.data(); out.a = a.data(); out.b = b.data(); out.process = p.data(); out.inv_pos = ip.data(); out.ret_pos = rp.data(); out.word = word.data();
    out.status = status.data(); out.bad_row = bad_row.data();
    const int st = emu_pr_batch(&in, &out, 3, seed);
    if (st != TBC_OK) { std::printf("emu_pr_batch: status %d: %s\n", st, emu_pr_error()); return 1; }
    if (out.n_ops != T || op_off != woff) { std::printf("seed %llu: op_off differs (%llu ops, want %zu)\n", (unsigned long long)seed, (unsigned long long)out.n_ops, T); wrong++; }
    for (size_t h = 0; h < nh; h++)
      if (status[h] != wst[h] || n_process[h] != wproc[h] || n_events[h] != hs[h].type.size() || (status[h] == TBC_OK) != (bad_row[h] == TBC_PAIR_NO_ROW)) {
        std::printf("seed %llu: history %zu: status %d (want %d), %u processes (want %u), bad row %u\n", (unsigned long long)seed, h, status[h], wst[h], n_process[h], wproc[h], bad_row[h]);
        wrong++;
      }
    f.resize(T); a.resize(T); b.resize(T); p.resize(T); ip.resize(T); rp.resize(T);
    if (f != wf || a != wa || b != wb || p != wp || ip != wi || rp != wr) { std::printf("seed %llu: an op column differs\n", (unsigned long long)seed); wrong++; }
    if (f.size() != T || word[T] != 0xEEEEEEEEu) { std::printf("seed %llu: a word past the ops was written\n", (unsigned long long)seed); wrong++; }
  }
  std::printf("%s: %zu histories, %zu events, %zu ops\n", wrong ? "WRONG" : "ok", nh, N, T);
  return wrong ? 1 : 0;
}
#endif
