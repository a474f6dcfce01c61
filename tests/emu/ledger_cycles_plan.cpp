// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  ledger_cycles_plan.cpp: tbc_ledger_cycles without a device, in a program of its own -- the
// one to build with -fsanitize=address,undefined (tests/test_ledger_cycles_plan.py does):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include -I tests/emu -I jepsen-tigerbeetle_amd/csrc tests/emu/ledger_cycles_plan.cpp -o ledger_cycles_plan && ./ledger_cycles_plan
// It builds ledgers of reads of many shapes (seeded): reads that overlap in time, reads without an invocation, partial reads, reads that
// check nothing, among transfers; it plans them (csrc/ledger_cycles_plan.h, the very functions ledger_cycles_host.hip runs every call
// through) and holds inv and ret to a plain restatement of pairing by process; and because it includes the emulator program of the
// kernels (emu_ledger_cycles.cpp) it runs every kernel of csrc/ledger_cycles_kernels.h on each ledger under the sanitizers -- an index
// past an array's end in a kernel is the sanitizer's to see -- under two grid caps and the plan's knobs, and holds scc, cyc_flags and
// the summary to a plain restatement of the rules: the explicit graph, its transitive closure by Warshall's algorithm, and the core by
// its quantifiers.  It breaks the input's rules and looks at the messages, and it holds the sequences' launches without a core to a
// list written out by hand.
#include <cstdio>
#include <cstdlib>
#include <map>
#include "emu_ledger_cycles.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

namespace {

struct Ledger {
  std::vector<uint32_t> index;
  std::vector<uint8_t> type, kind, flags, mop_flags;
  std::vector<int32_t> process;
  std::vector<uint64_t> mop_off{0};
  std::vector<int64_t> id, a, b, c, accounts;
  tbc_ledger_rt_in in() const {
    tbc_ledger_rt_in r{};
    tbc_ledger_in& s = r.ledger;
    s.n_ops = (uint32_t)index.size(); s.index = index.data(); s.type = type.data(); s.kind = kind.data(); s.flags = flags.data();
    s.mop_off = mop_off.data(); s.mop_id = id.data(); s.mop_a = a.data(); s.mop_b = b.data(); s.mop_c = c.data(); s.mop_flags = mop_flags.data();
    s.accounts = accounts.data(); s.n_accounts = (uint32_t)accounts.size();
    r.process = process.data(); r.ok_transfers_apply = 1;
    return r;
  }
  void op(uint8_t t, uint8_t k, int32_t p) {
    index.push_back(index.empty() ? 2u : index.back() + 1u + (uint32_t)(id.size() % 2));
    type.push_back(t); kind.push_back(k); flags.push_back(0); process.push_back(p);
  }
  void mop(int64_t ident, int64_t va, int64_t vb, uint8_t fl = 0) { id.push_back(ident); a.push_back(va); b.push_back(vb); c.push_back(77); mop_flags.push_back(fl); }
  void end() { mop_off.push_back(id.size()); }
};

uint64_t rng_state = 1;
uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

// `n_procs` processes take turns at random: an idle one invokes a read (or, now and then, a transfer), a busy one completes; some
// completions come without an invocation.  Counters grow slowly with time when `growing`, so that many reads stay clean.
Ledger make(uint32_t n_ops, uint32_t n_accounts, uint32_t n_procs, bool growing) {
  Ledger L;
  for (uint32_t k = 0; k < n_accounts; k++) L.accounts.push_back((int64_t)(n_accounts - k) * 3);                     // (unsorted)
  std::vector<int> busy(n_procs, 0);                                          // 0 idle, 1 reading, 2 transferring
  for (uint32_t i = 0; i < n_ops; i++) {
    const uint32_t p = rnd(n_procs);
    if (!busy[p] && rnd(10)) {
      const bool transfer = rnd(6) == 0;
      L.op(TBC_LEDGER_T_INVOKE, transfer ? TBC_LEDGER_K_TRANSFER : TBC_LEDGER_K_READ, (int32_t)p);
      if (transfer) L.mop(500 + (int64_t)i, L.accounts[0], L.accounts[n_accounts - 1]);
      else for (uint32_t j = 0; j < n_accounts; j++) L.mop(L.accounts[j], 0, 0, TBC_LEDGER_M_NIL);
      L.end();
      busy[p] = transfer ? 2 : 1;
      continue;
    }
    if (busy[p] == 2) { L.op(rnd(3) ? TBC_LEDGER_T_OK : TBC_LEDGER_T_INFO, TBC_LEDGER_K_TRANSFER, (int32_t)p); L.mop(500, 1, 2); L.end(); busy[p] = 0; continue; }
    // an :ok read (with no invocation when the process was idle), now and then a failed one
    L.op(rnd(9) ? TBC_LEDGER_T_OK : TBC_LEDGER_T_FAIL, TBC_LEDGER_K_READ, (int32_t)p);
    busy[p] = 0;
    const uint32_t how = rnd(7);
    const int64_t base = growing ? (int64_t)(i / 6) : 0;
    for (uint32_t j = 0; j < n_accounts; j++) {
      if (how == 0 && j == n_accounts / 2) continue;
      if (how == 1 && (j == 0 || rnd(2))) { L.mop(1000 + 64 * (int64_t)i + j, 1, 1); continue; }
      const bool jitter = !growing || rnd(8) == 0;
      L.mop(L.accounts[j], base + (jitter ? (int64_t)rnd(4) - 2 : 0), base + (jitter ? (int64_t)rnd(3) - 1 : 0), how == 2 && j + 1 == n_accounts ? TBC_LEDGER_M_NIL : 0);
    }
    L.end();
  }
  return L;
}

struct Want {
  std::vector<uint32_t> scc;
  std::vector<uint8_t> flags;
  uint32_t n_partial = 0, n_core = 0, n_on = 0, n_comp = 0, first = lgcy::kCyNone, largest = lgcy::kCyNone, largest_size = 0;
  uint64_t n_checked = 0;
};

// the rules, restated plainly from the columns
Want restate(const Ledger& L, std::vector<uint32_t>& inv1, std::vector<uint32_t>& ret1) {
  const uint32_t nA = (uint32_t)L.accounts.size(), C = 2 * nA;
  std::vector<std::map<uint32_t, int64_t>> vec;
  inv1.clear(); ret1.clear();
  std::map<int32_t, uint32_t> open;
  for (uint32_t i = 0; i < L.index.size(); i++) {
    if (L.type[i] == TBC_LEDGER_T_INVOKE) { open[L.process[i]] = i; continue; }
    uint32_t inv = lgcy::kCyNone;
    if (open.count(L.process[i])) { inv = open[L.process[i]]; open.erase(L.process[i]); }
    if (L.type[i] != TBC_LEDGER_T_OK || L.kind[i] != TBC_LEDGER_K_READ) continue;
    std::map<uint32_t, int64_t> v;
    for (uint64_t m = L.mop_off[i]; m < L.mop_off[i + 1]; m++)
      for (uint32_t k = 0; k < nA; k++)
        if (L.accounts[k] == L.id[m] && !(L.mop_flags[m] & TBC_LEDGER_M_NIL)) { v[2 * k] = L.a[m]; v[2 * k + 1] = L.b[m]; }
    vec.push_back(v);
    inv1.push_back(inv == lgcy::kCyNone ? 0u : L.index[inv] + 1u);
    ret1.push_back(L.index[i] + 1u);
  }
  const uint32_t R = (uint32_t)vec.size();
  const auto below = [&](uint32_t x, uint32_t y) {
    for (const auto& kv : vec[x]) { const auto it = vec[y].find(kv.first); if (it != vec[y].end() && kv.second < it->second) return true; }
    return false;
  };
  std::vector<std::vector<uint8_t>> reach(R, std::vector<uint8_t>(R, 0));
  for (uint32_t x = 0; x < R; x++) for (uint32_t y = 0; y < R; y++) reach[x][y] = x != y && (below(x, y) || ret1[x] < inv1[y]);
  for (uint32_t k = 0; k < R; k++) for (uint32_t x = 0; x < R; x++) if (reach[x][k]) for (uint32_t y = 0; y < R; y++) reach[x][y] |= reach[k][y];
  Want W;
  W.scc.assign(R, lgcy::kCyNone); W.flags.assign(R, 0);
  std::vector<uint8_t> complete(R), U(R);
  std::vector<int64_t> sum(R, 0);
  for (uint32_t x = 0; x < R; x++) { complete[x] = vec[x].size() == C; for (const auto& kv : vec[x]) sum[x] += kv.second; W.n_checked += vec[x].size() / 2; }
  for (uint32_t x = 0; x < R; x++) {
    U[x] = complete[x];
    for (uint32_t y = 0; y < R && U[x]; y++) if (complete[y] && below(x, y) && below(y, x)) U[x] = 0;
  }
  std::vector<uint32_t> size(R, 0);
  for (uint32_t x = 0; x < R; x++) {
    bool clean = U[x];
    for (uint32_t y = 0; y < R && clean; y++) if (U[y] && ret1[y] < inv1[x] && sum[y] > sum[x]) clean = false;
    uint32_t label = x, n = 1;
    for (uint32_t y = 0; y < R; y++) if (y != x && reach[x][y] && reach[y][x]) { label = std::min(label, y); n++; }
    W.flags[x] = (uint8_t)((complete[x] ? 0u : TBC_LEDGER_CYC_PARTIAL) | (n >= 2 ? TBC_LEDGER_CYC_ON_CYCLE : 0u) | (clean ? 0u : TBC_LEDGER_CYC_CORE));
    W.n_partial += !complete[x]; W.n_core += !clean;
    if (n >= 2) { W.scc[x] = label; W.n_on++; size[label]++; W.first = std::min(W.first, x); }
  }
  for (uint32_t x = 0; x < R; x++) {
    W.n_comp += size[x] != 0;
    if (size[x] > W.largest_size) { W.largest_size = size[x]; W.largest = x; }
  }
  return W;
}

void run_and_check(const Ledger& L, uint32_t grid_cap, uint64_t seed, uint32_t sort_chunks_cap, uint32_t scan_rows) {
  const tbc_ledger_rt_in in = L.in();
  std::vector<uint32_t> inv1, ret1;
  const Want W = restate(L, inv1, ret1);
  std::string err;
  lgcy::Plan P;
  if (!lgcy::validate("t", &in, err) || !lgcy::plan("t", &in, P, err)) { std::printf("%s\n", err.c_str()); CHECK(false); }
  CHECK(P.inv1 == inv1 && P.ret1 == ret1 && P.sn.n_reads == W.scc.size());
  CHECK(P.arena.acc.at == P.sn.arena.bytes && P.arena.bytes >= P.arena.cyc_flags.at && P.arena.head_bytes() % 256 == 0);
  const size_t R = W.scc.size();
  std::vector<uint32_t> scc(R + 1, 0x77777777u);
  std::vector<uint8_t> flags(R + 1, 0x77);
  tbc_ledger_cycles_out out{};
  out.scc = scc.data(); out.cyc_flags = flags.data();
  const int st = emu_cycles_check(&in, &out, grid_cap, seed, sort_chunks_cap, scan_rows, 0);
  if (st != 0) std::printf("%s\n", emu_cycles_error());
  CHECK(st == 0);
  CHECK(scc[R] == 0x77777777u && flags[R] == 0x77);
  for (size_t r = 0; r < R; r++) {
    if (scc[r] != W.scc[r] || flags[r] != W.flags[r]) std::printf("read %zu of %zu: scc %u want %u, flags %u want %u\n", r, R, scc[r], W.scc[r], flags[r], W.flags[r]);
    CHECK(scc[r] == W.scc[r] && flags[r] == W.flags[r]);
  }
  const tbc_ledger_cycles_summary& s = out.summary;
  CHECK(s.read_count == R && s.n_partial == W.n_partial && s.n_core == W.n_core && s.n_on_cycle == W.n_on && s.n_components == W.n_comp);
  CHECK(s.first == W.first && s.largest == W.largest && s.largest_size == W.largest_size && s.valid == (W.n_on == 0) && s.n_checked == W.n_checked && s.bad_values == 0);
  CHECK((s.closure_rounds == 0) == (W.n_core == 0));
  uint32_t bound = 1;
  while ((1u << (bound - 1)) < std::max(1u, W.n_core)) bound++;
  CHECK(s.closure_rounds <= bound);                                          // ceil(log2 m) + 1 at most
}

}  // namespace

int main() {
  uint32_t planned = 0, with_cycles = 0, with_clean_on_cycle = 0, without_core = 0;
  for (uint32_t trial = 0; trial < 60; trial++) {
    rng_state = 77 + trial;
    const uint32_t n_ops = 1 + rnd(trial < 40 ? 60 : 220), n_accounts = 1 + rnd(trial % 5 == 0 ? 40 : 4);
    const Ledger L = make(n_ops, n_accounts, 2 + rnd(5), trial % 2 == 0);
    run_and_check(L, 1 + trial % 3, trial, trial % 4 == 0 ? 1 : 0, trial % 3 == 0 ? 2 : 0);
    std::vector<uint32_t> i1, r1;
    const Want W = restate(L, i1, r1);
    planned++; with_cycles += W.n_on != 0; without_core += W.n_core == 0;
    for (size_t r = 0; r < W.flags.size(); r++) if ((W.flags[r] & 6u) == 2u) { with_clean_on_cycle++; break; }
  }
  CHECK(with_cycles >= 10 && with_clean_on_cycle >= 5 && without_core >= 3);
  // refusals: the rules of the input, with the entry point's name
  uint32_t refusals = 0;
  {
    rng_state = 5;
    Ledger L = make(40, 3, 3, true);
    std::string err;
    tbc_ledger_rt_in in = L.in();
    in.process = nullptr;
    CHECK(!lgcy::validate("tbc_ledger_cycles", &in, err) && err.find("tbc_ledger_cycles: null argument (process)") == 0); refusals++;
    in = L.in(); in.ok_transfers_apply = 2;
    CHECK(!lgcy::validate("tbc_ledger_cycles", &in, err) && err.find("ok_transfers_apply") != std::string::npos); refusals++;
    L.type[2] = 9; in = L.in();
    CHECK(!lgcy::validate("tbc_ledger_cycles", &in, err) && err.find("tbc_ledger_cycles: op 2 (index") == 0); refusals++;
  }
  // the launches without a core: the snapshot filter's, four of this checker's, then labels, largest and the summary -- and nothing between
  {
    Ledger L;
    L.accounts = {4, 9};
    for (uint32_t k = 0; k < 70; k++) {
      L.op(TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_READ, 1); L.mop(4, 0, 0, TBC_LEDGER_M_NIL); L.mop(9, 0, 0, TBC_LEDGER_M_NIL); L.end();
      L.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_READ, 1); L.mop(4, k, k); L.mop(9, k / 2, k); L.end();
    }
    const tbc_ledger_rt_in in = L.in();
    std::string err;
    lgcy::Plan P;
    CHECK(lgcy::validate("t", &in, err) && lgcy::plan("t", &in, P, err));
    emu::Arena C(err);
    C.open(0, P.arena.bytes);
    const lgcy::CyArgs A = lgcy::args(&in, P, C.base());
    emu::Recorder rec, snap;
    lgsn::filter_sequence(snap, A.sn);
    lgcy::prepare_sequence(rec, A);
    lgcy::describe_sequence(rec, A);
    lgcy::finish_sequence(rec, A, 0, 0);
    using E = emu::Recorder;
    std::vector<E::Launch> want = snap.launches;
    for (const E::Launch& l : std::vector<E::Launch>{{E::of(cy_sums_kernel), 1, 256}, {E::of(cy_pmax_kernel), 1, 256}, {E::of(cy_clean_kernel), 1, 256}, {E::of(cy_core_scan_kernel), 1, 256},
                                                      {E::of(cy_labels_kernel), 1, 256}, {E::of(cy_largest_kernel), 1, 256}, {E::of(cy_summary_kernel), 1, 64}})
      want.push_back(l);
    CHECK(rec.is(want));
    run_and_check(L, 2, 1, 0, 0);
  }
  std::printf("%u ledgers planned, run and checked, %u refusals, the launches of 1 shape\n", planned, refusals);
  return 0;
}
