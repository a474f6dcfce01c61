// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_split.cpp: tbc_pair_keyed_events on the CPU -- the validation, the plan and the steps
// of csrc/split_plan.h (the list csrc/split_host.hip runs) over the emulator's call frame, and the kernels of csrc/split_kernels.h
// followed by those of csrc/pair_kernels.h (the very files hipcc compiles into libtbcheck.so) under the wavefront / workgroup emulator.
// THE LAUNCHER IS THIS PROGRAM'S OWN: oneshot_emu.h runs a launch's workgroups one after the other in index order, which a kernel that
// takes a row's place from the order in which its atomics arrive would pass; here the workgroups of every launch run in a seeded
// PERMUTED order, so that such a place moves with the seed.  Grids that stride are capped at `grid_cap` workgroups.
// Built as a shared object by tests/test_keyed_events_emu.py (also with SPLIT_MUTATION 1 to 4, which that test must see).  With
// EMU_SPLIT_MAIN it is a program of its own (linked with csrc/tbc_host.cpp, the specification of the pairing): seeded keyed histories
// through the emulator, against a stable split on the host and tbc_pair_events per key, every array compared -- the form that is built
// with -fsanitize=address,undefined and run as a plain executable.
#include <numeric>
#include "oneshot_emu.h"

// a lane shuffle is a rendezvous: every lane deposits, each reads its partner's deposit
static inline uint64_t emu_shfl(uint64_t v, int src_of_me, int site) {
  const int me = (int)wv::lane_id();
  const uint64_t* s = wv::gather(v, site);
  return src_of_me >= 0 && src_of_me < 64 ? s[src_of_me] : s[me];
}
#define __shfl(v, src) ((decltype(v))emu_shfl((uint64_t)(uint32_t)(v), (int)(src), 400000 + __LINE__))
// the 64-bit compare-and-swap of the key table (between two rendezvous the emulator runs one lane at a time)
static inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long expected, unsigned long long desired) {
  const unsigned long long o = *p;
  if (o == expected) *p = desired;
  return o;
}

#include "split_plan.h"
#include "split_kernels.h"
#include "pair_kernels.h"

namespace {

std::string g_err;

// emu::Launcher with the workgroups of a launch in a seeded permuted order
struct PermutedLauncher {
  uint32_t grid_cap;
  uint64_t seed;
  uint32_t n_launches = 0;
  PermutedLauncher(uint32_t cap, uint64_t s) : grid_cap(cap ? cap : 1u), seed(s) {}
  uint32_t grid(uint64_t blocks, uint32_t cap) const { return oneshot::capped_grid(blocks, std::min(cap, grid_cap)); }
  template <class... P, class... A>
  void launch(void (*kernel)(P...), uint32_t grid, uint32_t threads, const A&... args) {
    std::function<void()> body = [&] { kernel(static_cast<P>(args)...); };
    std::vector<uint32_t> order(grid);
    std::iota(order.begin(), order.end(), 0u);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull * (n_launches + 1u);
    for (uint32_t k = grid; k > 1u; k--) {                                    // Fisher-Yates
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      std::swap(order[k - 1u], order[(size_t)(x % k)]);
    }
    for (uint32_t b : order) wv::run_workgroup(emu::Launcher::trampoline, &body, (int)((threads + 63u) / 64u), b, seed + 1000u * n_launches + b);
    n_launches++;
  }
};

}  // namespace

// TBC_OK: done; otherwise the status the library gives (emu_sp_error says why).  out: null for the split alone
extern "C" int emu_sp_keyed(const tbc_keyed_events* in, tbc_split_out* split, tbc_pair_out* out, uint32_t grid_cap, uint64_t seed) {
  g_err.clear();
  if (!in || !split) { g_err = "emu_sp_keyed: null argument"; return TBC_ERR_INVALID_ARG; }
  const tbc_status st = sp::validate("emu_sp_keyed", in, split, out, g_err);
  if (st != TBC_OK) return st;
  sp::Plan P;
  sp::plan(in, split, out, P);
  struct Run {
    PermutedLauncher go;
    void keys(const sp::SpArgs& A) { sp::keys_sequence(go, A); }
    void sort(const sp::SpArgs& A) { sp::sort_sequence(go, A); }
    void pair(const pr::PrArgs& A) { pr::pair_sequence(go, A); }
    void emit(const pr::PrArgs& A) { pr::emit_sequence(go, A); }
  };
  emu::Arena C(g_err);
  C.open(in->device, P.bytes);
  sp::steps(C, Run{PermutedLauncher(grid_cap, seed)}, "emu_sp_keyed", in, P, split, out);
  return C.close();
}
// THE BATCH FORM of the arena (sp::plan_batch / sp::args_batch, csrc/batch_stream.hip): every region laid out for `cap` rows and used by
// a call of in->n <= cap rows -- its own tile count, its own table size.  The caller's input arrays hold `cap` rows (the frame copies
// whole regions); only the first in->n count.
extern "C" int emu_sp_keyed_cap(const tbc_keyed_events* in, tbc_split_out* split, tbc_pair_out* out, uint32_t grid_cap, uint64_t seed, uint32_t cap) {
  g_err.clear();
  if (!in || !split || in->n > cap) { g_err = "emu_sp_keyed_cap: null argument, or more rows than the capacity"; return TBC_ERR_INVALID_ARG; }
  const tbc_status st = sp::validate("emu_sp_keyed_cap", in, split, out, g_err);
  if (st != TBC_OK) return st;
  tbc_keyed_events whole = *in;
  whole.n = cap;
  tbc_split_out wide = *split;
  wide.keys_cap = std::max(split->keys_cap, 1u);
  sp::Plan P;
  sp::plan(&whole, &wide, out, P);                                            // the regions of `cap` rows ...
  P.n = in->n; P.n_tiles = (in->n + sp::kTile - 1u) / sp::kTile; P.bits = sp::table_bits(in->n);   // ... used by a call of in->n, as sp::args_batch sets them
  struct Run {
    PermutedLauncher go;
    void keys(const sp::SpArgs& A) { sp::keys_sequence(go, A); }
    void sort(const sp::SpArgs& A) { sp::sort_sequence(go, A); }
    void pair(const pr::PrArgs& A) { pr::pair_sequence(go, A); }
    void emit(const pr::PrArgs& A) { pr::emit_sequence(go, A); }
  };
  emu::Arena C(g_err);
  C.open(in->device, P.bytes);
  sp::steps(C, Run{PermutedLauncher(grid_cap, seed)}, "emu_sp_keyed_cap", in, P, split, out);
  return C.close();
}
extern "C" const char* emu_sp_error() { return g_err.c_str(); }
extern "C" uint64_t emu_sp_hash(uint32_t key, uint32_t bits) { return sp::table_hash(key, bits); }
extern "C" uint32_t emu_sp_table_bits(uint64_t n) { return sp::table_bits(n); }
extern "C" uint32_t emu_sp_tile() { return sp::kTile; }
extern "C" uint32_t emu_sp_passes(uint32_t n_keys) { return sp::sort_passes(n_keys); }
extern "C" uint32_t emu_sp_mutation() {
#if defined(SPLIT_MUTATION)
  return SPLIT_MUTATION;
#else
  return 0u;
#endif
}

#if defined(EMU_SPLIT_MAIN)
#include <map>
namespace {

struct Events { std::vector<uint8_t> type, f; std::vector<int32_t> process, a, b, key; };

uint64_t g_rng = 0x243F6A8885A308D3ull;
uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }

// one interleaved history of about `n` rows over the keys `kv`, `procs` processes a key; a key in `spoil` gets one malformed row
Events history_over(uint32_t n, const std::vector<int32_t>& kv, uint32_t procs, uint32_t spoil_every) {
  Events e;
  const uint32_t n_keys = (uint32_t)kv.size();
  std::vector<std::vector<int>> open(n_keys, std::vector<int>(procs, 0));
  std::vector<std::vector<int32_t>> id(n_keys, std::vector<int32_t>(procs));
  for (uint32_t k = 0; k < n_keys; k++) for (uint32_t p = 0; p < procs; p++) id[k][p] = (int32_t)p;
  std::vector<int> spoiled(n_keys, 0);
  while (e.type.size() < n) {
    const uint32_t k = rnd(4) ? rnd(n_keys) : rnd(std::min(n_keys, 3u)), p = rnd(procs);           // (a few hot keys)
    const int32_t pid = id[k][p];
    uint32_t ty;
    if (!open[k][p]) { ty = TBC_INVOKE; open[k][p] = 1; }
    else { const uint32_t r = rnd(10); ty = r < 2 ? TBC_FAIL : (r < 3 ? TBC_INFO : TBC_OK_); open[k][p] = 0; }
    if (ty == TBC_INFO) id[k][p] += (int32_t)procs;                                                // (a crashed process comes back as p + procs, as Jepsen numbers it)
    if (spoil_every && k % spoil_every == spoil_every - 1u && !spoiled[k] && rnd(8) == 0) { ty = 9u; spoiled[k] = 1; }
    e.type.push_back((uint8_t)ty); e.process.push_back(pid); e.f.push_back((uint8_t)rnd(3));
    e.a.push_back(rnd(2) ? TBC_NIL : (int32_t)rnd(5)); e.b.push_back((int32_t)rnd(5)); e.key.push_back(kv[k]);
  }
  return e;
}
// ... over `n_keys` keys, their values spread over the int32 range, INT32_MIN and -1 among them
Events history(uint32_t n, uint32_t n_keys, uint32_t procs, uint32_t spoil_every) {
  std::vector<int32_t> kv(n_keys);
  for (uint32_t k = 0; k < n_keys; k++) kv[k] = k == 0 ? INT32_MIN : (k == 1 ? -1 : (int32_t)(0x7FFFFFFF - (int32_t)k * 40503));
  return history_over(n, kv, procs, spoil_every);
}
// keys whose probe run crosses the END of the table a history of n rows gets: 8 whose home is the last slot, 8 in the slot before it, 4
// in slot 0, a key of each in turn (the first three are the hot keys)
std::vector<int32_t> wrapping_keys(uint32_t n) {
  const uint32_t bits = sp::table_bits(n);
  const uint64_t last = (1ull << bits) - 1ull;
  std::vector<std::vector<int32_t>> g(3);
  const uint64_t home[3] = {last, last - 1ull, 0ull};
  const size_t count[3] = {8, 8, 4};
  for (uint32_t k = 1; k < 200000u; k++)
    for (int i = 0; i < 3; i++)
      if (sp::table_hash(k, bits) == home[i] && g[i].size() < count[i]) g[i].push_back((int32_t)k);
  std::vector<int32_t> kv;
  for (size_t j = 0; j < 8; j++)
    for (int i = 0; i < 3; i++)
      if (j < g[i].size()) kv.push_back(g[i][j]);
  return kv;
}

// want_keys: the distinct keys the history is there to have (0: any)
int check(const Events& e0, bool packed, uint32_t grid_cap, uint64_t seed, uint32_t cap = 0, size_t want_keys = 0) {
  const uint32_t n = (uint32_t)e0.type.size();
  Events e = e0;                                                              // (cap: the arrays hold `cap` rows, the first n count)
  if (cap) { e.type.resize(cap); e.f.resize(cap); e.process.resize(cap); e.a.resize(cap); e.b.resize(cap); e.key.resize(cap); }
  // the specification: a stable split by first appearance, tbc_pair_events per key
  std::vector<int32_t> wkeys;
  std::map<int32_t, uint32_t> id_of;
  std::vector<std::vector<uint32_t>> rows;
  for (uint32_t r = 0; r < n; r++) {
    auto it = id_of.find(e.key[r]);
    if (it == id_of.end()) { it = id_of.emplace(e.key[r], (uint32_t)wkeys.size()).first; wkeys.push_back(e.key[r]); rows.emplace_back(); }
    rows[it->second].push_back(r);
  }
  const size_t nk = wkeys.size();
  if (want_keys && nk != want_keys) { std::printf("seed %llu: the history has %zu keys, it is there for %zu\n", (unsigned long long)seed, nk, want_keys); return 1; }
  std::vector<uint64_t> wev_off{0}, woff{0};
  std::vector<uint32_t> wrow_of, wi, wr, wproc(nk);
  std::vector<uint8_t> wf; std::vector<int32_t> wa, wb, wp, wst(nk);
  for (size_t h = 0; h < nk; h++) {
    Events s;
    for (uint32_t r : rows[h]) { s.type.push_back(e.type[r]); s.process.push_back(e.process[r]); s.f.push_back(e.f[r]); s.a.push_back(e.a[r]); s.b.push_back(e.b[r]); wrow_of.push_back(r); }
    wev_off.push_back(wrow_of.size());
    const uint32_t m = (uint32_t)s.type.size();
    tbc_events ev{m, s.type.data(), s.process.data(), s.f.data(), s.a.data(), s.b.data()};
    std::vector<uint8_t> f(m + 1); std::vector<int32_t> a(m + 1), b(m + 1), p(m + 1); std::vector<uint32_t> ip(m + 1), rp(m + 1);
    uint32_t k = 0, np = 0;
    wst[h] = tbc_pair_events(&ev, f.data(), a.data(), b.data(), p.data(), ip.data(), rp.data(), &k, &np);
    if (wst[h] != TBC_OK) { k = 0; np = 0; }
    wf.insert(wf.end(), f.begin(), f.begin() + k); wa.insert(wa.end(), a.begin(), a.begin() + k); wb.insert(wb.end(), b.begin(), b.begin() + k);
    wp.insert(wp.end(), p.begin(), p.begin() + k); wi.insert(wi.end(), ip.begin(), ip.begin() + k); wr.insert(wr.end(), rp.begin(), rp.begin() + k);
    wproc[h] = np; woff.push_back(wf.size());
  }
  const size_t T = wf.size();
  std::vector<uint32_t> words(std::max(n, cap));
  if (packed) { tbc_events all{n, e.type.data(), e.process.data(), e.f.data(), e.a.data(), e.b.data()}; if (tbc_pack_events(&all, words.data()) != TBC_OK) return 1; }
  tbc_keyed_events in{};
  in.n = n; in.key = e.key.data(); in.process = e.process.data();
  if (packed) in.ev_word = words.data();
  else { in.type = e.type.data(); in.f = e.f.data(); in.a = e.a.data(); in.b = e.b.data(); }
  std::vector<int32_t> keys(nk + 1, 0x5A5A5A5A); std::vector<uint64_t> ev_off(nk + 1); std::vector<uint32_t> row_of(n + 1, 0xEEEEEEEEu);
  tbc_split_out split{};
  split.keys_cap = (uint32_t)nk; split.keys = keys.data(); split.ev_off = ev_off.data(); split.row_of = row_of.data();
  std::vector<uint64_t> op_off(nk + 1); std::vector<uint32_t> n_events(nk + 1), n_process(nk + 1), bad_row(nk + 1); std::vector<int32_t> status(nk + 1);
  std::vector<uint8_t> f(T + 1, 0xEE); std::vector<int32_t> a(T + 1), b(T + 1), p(T + 1); std::vector<uint32_t> ip(T + 1), rp(T + 1);
  tbc_pair_out out{};
  out.ops_cap = T; out.op_off = op_off.data(); out.n_events = n_events.data(); out.n_process = n_process.data();
  out.f = f.data(); out.a = a.data(); out.b = b.data(); out.process = p.data(); out.inv_pos = ip.data(); out.ret_pos = rp.data();
  out.status = status.data(); out.bad_row = bad_row.data();
  const int st = cap ? emu_sp_keyed_cap(&in, &split, &out, grid_cap, seed, cap) : emu_sp_keyed(&in, &split, &out, grid_cap, seed);
  if (st != TBC_OK) { std::printf("emu_sp_keyed: status %d: %s\n", st, emu_sp_error()); return 1; }
  int wrong = 0;
  keys.resize(nk); row_of.resize(n);
  if (split.n_keys != nk || keys != wkeys || ev_off != wev_off || row_of != wrow_of) { std::printf("seed %llu: the split differs (%u keys, want %zu)\n", (unsigned long long)seed, split.n_keys, nk); wrong++; }
  if (out.n_ops != T || op_off != woff) { std::printf("seed %llu: op_off differs (%llu ops, want %zu)\n", (unsigned long long)seed, (unsigned long long)out.n_ops, T); wrong++; }
  for (size_t h = 0; h < nk; h++)
    if (status[h] != wst[h] || n_process[h] != wproc[h] || n_events[h] != rows[h].size()) { std::printf("seed %llu: key %zu: status %d (want %d), %u processes (want %u)\n", (unsigned long long)seed, h, status[h], wst[h], n_process[h], wproc[h]); wrong++; }
  if (f[T] != 0xEE) { std::printf("seed %llu: an op past the total was written\n", (unsigned long long)seed); wrong++; }
  f.resize(T); a.resize(T); b.resize(T); p.resize(T); ip.resize(T); rp.resize(T);
  if (f != wf || a != wa || b != wb || p != wp || ip != wi || rp != wr) { std::printf("seed %llu: an op column differs\n", (unsigned long long)seed); wrong++; }
  return wrong;
}

}  // namespace

int main() {
  int wrong = 0;
  size_t rows = 0;
  const Events small = history(700, 5, 3, 0), wide = history(3 * sp::kTile + 77, 300, 2, 7), one = history(sp::kTile + 1, 1, 6, 0);
  for (const Events* e : {&small, &wide, &one})
    for (uint64_t seed = 1; seed <= 2; seed++) {
      wrong += check(*e, seed == 2, seed == 1 ? 3u : 1u, seed);
      rows += e->type.size();
    }
  // the batch form: regions for a capacity, a call of fewer rows (a tile more, and ten times the rows)
  wrong += check(small, true, 3u, 3, (uint32_t)small.type.size() + sp::kTile + 5u);
  wrong += check(wide, true, 1u, 4, 10u * (uint32_t)wide.type.size());
  // a probe run across the table's end (20 keys around the last slot of the 1,024 that 300 rows get), and several rows a key over two
  // passes of the sort (257 keys, each key's rows over the five tiles)
  const std::vector<int32_t> around_the_end = wrapping_keys(300);
  if (around_the_end.size() != 20u) { std::printf("WRONG: %zu keys around the table's end\n", around_the_end.size()); return 1; }
  const Events wraps = history_over(300, around_the_end, 2, 0), two_passes = history(4 * sp::kTile + 3, 257, 2, 0);
  for (uint64_t seed = 5; seed <= 6; seed++) {
    wrong += check(wraps, seed == 6, seed == 5 ? 3u : 1u, seed, 0, 20);
    wrong += check(two_passes, seed == 5, seed == 5 ? 3u : 1u, seed, 0, 257);
    rows += wraps.type.size() + two_passes.type.size();
  }
  std::printf("%s: %zu rows\n", wrong ? "WRONG" : "ok", rows);
  return wrong ? 1 : 0;
}
#endif
