// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  ledger_journal_plan.cpp: the host side of tbc_ledger_journal without a device -- the validation
// and the plan of csrc/ledger_journal_plan.h (the very functions ledger_journal_host.hip runs every call through) in a program of its own,
// the one to build with -fsanitize=address,undefined (tests/test_ledger_journal_plan.py does):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include -I tests/emu -I jepsen-tigerbeetle_amd/csrc tests/emu/ledger_journal_plan.cpp -o ledger_journal_plan && ./ledger_journal_plan
// It builds ledgers of many shapes (seeded), plans them and checks what can be checked without Python: the three groups of micro-ops the
// device gets (spans, image: the transfers' and the entries' five columns, the reads' four, never a read's c), the owner columns per
// transfer micro-op, the lookups' and the reads' inv and ret, the slices, the arena's regions; it shows that the plan reads no micro-op
// (the columns are not there); it looks at the plan's own refusals.  Because it includes the emulator program of the kernels
// (emu_ledger_journal.cpp), it runs every kernel of csrc/ledger_journal_kernels.h on each ledger under the sanitizers too, into output
// arrays of exactly the size the header states -- an index past an array's end is the sanitizer's to see -- and holds what comes back to
// the sums that need no restatement of the rules.  And it holds lgjn::sequence -- the launches the library makes -- to the list of
// (kernel, grid, threads) written out below by hand, under the device's caps: launch for launch, and no launch for an empty phase.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include "emu_ledger_journal.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

namespace {

struct Ledger {
  std::vector<uint32_t> index;
  std::vector<int32_t> process;
  std::vector<uint8_t> type, kind, flags, mop_flags;
  std::vector<uint64_t> mop_off{0};
  std::vector<int64_t> id, a, b, c, accounts, init_c, init_d;
  tbc_ledger_rt_in in() const {
    tbc_ledger_rt_in r{};
    tbc_ledger_in& s = r.ledger;
    s.n_ops = (uint32_t)index.size(); s.index = index.data(); s.type = type.data(); s.kind = kind.data(); s.flags = flags.data();
    s.mop_off = mop_off.data(); s.mop_id = id.data(); s.mop_a = a.data(); s.mop_b = b.data(); s.mop_c = c.data(); s.mop_flags = mop_flags.data();
    s.accounts = accounts.data(); s.n_accounts = (uint32_t)accounts.size();
    r.process = process.data(); r.init_credits = init_c.data(); r.init_debits = init_d.data(); r.ok_transfers_apply = 1;
    return r;
  }
  void op(uint8_t t, uint8_t k, int32_t p) {
    index.push_back(index.empty() ? 2u : index.back() + 1u + (uint32_t)(id.size() % 2));
    type.push_back(t); kind.push_back(k); flags.push_back(0); process.push_back(p);
  }
  void mop(int64_t ident, int64_t va, int64_t vb, int64_t vc, uint8_t fl = 0) { id.push_back(ident); a.push_back(va); b.push_back(vb); c.push_back(vc); mop_flags.push_back(fl); }
  void end() { mop_off.push_back(id.size()); }
};

uint64_t rng_state = 1;
uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

// transfers (ids repeat now and then, nil micro-ops, foreign accounts), lookups of entries drawn from the ids so far (some changed, some
// made up), reads, each invoked by a process of a few and completed -- or not -- later
Ledger make(uint32_t n_ops, uint32_t n_accounts) {
  Ledger L;
  for (uint32_t k = 0; k < n_accounts; k++) { L.accounts.push_back((int64_t)(n_accounts - k) * 3); L.init_c.push_back(100 + k); L.init_d.push_back(k); }
  const auto acct = [&] { return n_accounts && rnd(8) ? L.accounts[rnd(n_accounts)] : 1000 + (int64_t)rnd(5); };
  std::vector<std::array<int64_t, 4>> known;
  std::map<int32_t, uint8_t> open;
  for (uint32_t i = 0; i < n_ops; i++) {
    const int32_t p = (int32_t)rnd(6);
    if (open.count(p)) {
      const uint8_t k = open[p];
      open.erase(p);
      const uint8_t t = (uint8_t)(1 + rnd(3));
      L.op(t, k, p);
      if (t == TBC_LEDGER_T_OK && k == TBC_LEDGER_K_READ)
        for (uint32_t j = 0; j < n_accounts; j++) { if (rnd(9)) L.mop(L.accounts[j], rnd(50), rnd(50), 0, rnd(12) ? 0 : TBC_LEDGER_M_NIL); }
      if (t == TBC_LEDGER_T_OK && k == TBC_LEDGER_K_LOOKUP)
        for (uint32_t j = 0, n = rnd(3) ? rnd(90) : rnd(4); j < n && !known.empty(); j++) {
          const auto& e = known[rnd((uint32_t)known.size())];
          L.mop(rnd(15) ? e[0] : 7000 + e[0], e[1], e[2], rnd(15) ? e[3] : e[3] + 1, rnd(20) ? 0 : TBC_LEDGER_M_NIL);
        }
      L.end();
      continue;
    }
    const uint8_t k = (uint8_t)(1 + rnd(3));
    open[p] = k;
    L.op(TBC_LEDGER_T_INVOKE, k, p);
    if (k == TBC_LEDGER_K_TRANSFER)
      for (uint32_t j = 0, n = 1 + rnd(3); j < n; j++) {
        const int64_t ident = !known.empty() && !rnd(12) ? known[rnd((uint32_t)known.size())][0] : 5000 + (int64_t)L.id.size();
        known.push_back({ident, acct(), acct(), (int64_t)rnd(9)});
        L.mop(ident, known.back()[1], known.back()[2], known.back()[3], rnd(15) ? 0 : TBC_LEDGER_M_NIL);
      }
    if (rnd(10) == 0) open.erase(p);                                          // (the next op of the process is an invocation again: this one stays open)
    L.end();
  }
  return L;
}

void look(const Ledger& L, uint32_t grid_cap, uint32_t slice_entries, uint32_t chunk) {
  const tbc_ledger_rt_in rin = L.in();
  const tbc_ledger_in& in = rin.ledger;
  std::string err;
  CHECK(lgjn::validate("plan", &rin, err));
  lgjn::Plan P;
  CHECK(lgjn::plan("plan", &rin, P, err, slice_entries ? slice_entries : lgjn::kJnSliceEntries, chunk ? chunk : lgjn::kJnChunk));
  // the three groups, restated: which of the caller's micro-ops each holds, in order
  std::vector<uint64_t> xs, es, rs, lk_cum{0}, rd_cum{0};
  std::vector<uint32_t> x_owner, slice_cum{0};
  for (uint32_t i = 0; i < in.n_ops; i++) {
    std::vector<uint64_t>* into = in.type[i] == TBC_LEDGER_T_INVOKE && in.kind[i] == TBC_LEDGER_K_TRANSFER ? &xs
                                  : in.type[i] == TBC_LEDGER_T_OK && in.kind[i] == TBC_LEDGER_K_LOOKUP ? &es
                                  : in.type[i] == TBC_LEDGER_T_OK && in.kind[i] == TBC_LEDGER_K_READ ? &rs : nullptr;
    if (!into) continue;
    for (uint64_t m = in.mop_off[i]; m < in.mop_off[i + 1]; m++) { into->push_back(m); if (into == &xs) x_owner.push_back(i); }
    if (into == &es) { lk_cum.push_back(es.size()); slice_cum.push_back(slice_cum.back() + (uint32_t)((in.mop_off[i + 1] - in.mop_off[i] + P.slice_entries - 1) / P.slice_entries)); }
    if (into == &rs) rd_cum.push_back(rs.size());
  }
  const auto same = [&](const oneshot::Spans& S, const std::vector<uint64_t>& src) {
    uint64_t covered = 0;
    for (const oneshot::Span& s : S.spans) {
      CHECK(s.n > 0 && s.dst == covered);
      for (uint64_t j = 0; j < s.n; j++) CHECK(src[s.dst + j] == s.src + j);
      covered += s.n;
    }
    CHECK(covered == src.size() && S.n_mops == src.size());
  };
  same(P.xf, xs); same(P.lk, es); same(P.rd, rs);
  CHECK(P.lk_cum == lk_cum && P.rd_cum == rd_cum && P.slice_cum == slice_cum && P.n_slices == slice_cum.back());
  CHECK(P.n_lookups == lk_cum.size() - 1 && P.n_reads == rd_cum.size() - 1 && P.n_words == (xs.size() + 31) / 32 && P.n_class == 2 * in.n_accounts);
  CHECK(P.chunk % 64 == 0 && P.chunk >= 64 && P.chunk <= 256);
  // the owner columns: the invocation's index, and the completion's -- the next op of the same process, if that is a completion
  for (size_t m = 0; m < xs.size(); m++) {
    const uint32_t i = x_owner[m];
    uint32_t ret = lgjn::kJnNone; uint8_t status = TBC_LEDGER_T_INVOKE;
    for (uint32_t j = i + 1; j < in.n_ops; j++)
      if (rin.process[j] == rin.process[i]) { if (in.type[j] != TBC_LEDGER_T_INVOKE) { ret = in.index[j]; status = in.type[j]; } break; }
    CHECK(P.x_inv[m] == in.index[i] && P.x_ret[m] == ret && P.x_status[m] == status);
  }
  for (size_t k = 0; k < P.accounts.size(); k++) { if (k) CHECK(P.accounts[k - 1] < P.accounts[k]); CHECK(in.accounts[P.acct_pos[k]] == P.accounts[k]); }
  for (uint32_t k = 0; k < in.n_accounts; k++) CHECK(P.init[2 * k] == rin.init_credits[k] && P.init[2 * k + 1] == rin.init_debits[k]);
  // the arena: regions in order, 256 B starts, none overlapping
  const oneshot::Region* reg = reinterpret_cast<const oneshot::Region*>(&P.arena);
  const size_t n_reg = offsetof(lgjn::JnArena, bytes) / sizeof(oneshot::Region);
  for (size_t k = 0; k < n_reg; k++) CHECK(reg[k].at % 256 == 0 && reg[k].at + reg[k].bytes <= (k + 1 < n_reg ? reg[k + 1].at : P.arena.bytes));
  const lgjn::JnArena& A = P.arena;
  const std::vector<unsigned char> img = lgjn::image(&rin, P);
  CHECK(img.size() == A.image_bytes() && A.image_bytes() == A.slots.at && A.zero_bytes() == A.summary.at - A.slots.at);
  CHECK(img.size() <= 33 * (xs.size() + es.size()) + 25 * rs.size() + 9 * xs.size() + 20 * lk_cum.size() + 16 * rd_cum.size() + 28 * (size_t)in.n_accounts + 512 + 28 * 256);
  CHECK(A.r_id.bytes == rs.size() * 8 && A.r_flags.bytes == rs.size() && A.r_flags.at + A.r_flags.bytes <= A.slots.at);      // (no region for a read's c)
  const auto col = [&](const oneshot::Region& r, size_t m) { int64_t v; std::memcpy(&v, img.data() + r.at + m * 8, 8); return v; };
  for (size_t m = 0; m < xs.size(); m++) CHECK(col(A.x_id, m) == in.mop_id[xs[m]] && col(A.x_a, m) == in.mop_a[xs[m]] && col(A.x_b, m) == in.mop_b[xs[m]] && col(A.x_c, m) == in.mop_c[xs[m]] && img[A.x_flags.at + m] == in.mop_flags[xs[m]]);
  for (size_t m = 0; m < es.size(); m++) CHECK(col(A.e_id, m) == in.mop_id[es[m]] && col(A.e_a, m) == in.mop_a[es[m]] && col(A.e_b, m) == in.mop_b[es[m]] && col(A.e_c, m) == in.mop_c[es[m]] && img[A.e_flags.at + m] == in.mop_flags[es[m]]);
  for (size_t m = 0; m < rs.size(); m++) CHECK(col(A.r_id, m) == in.mop_id[rs[m]] && col(A.r_a, m) == in.mop_a[rs[m]] && col(A.r_b, m) == in.mop_b[rs[m]] && img[A.r_flags.at + m] == in.mop_flags[rs[m]]);
  // ---- the kernels, under the emulator and the sanitizers, into arrays of exactly the stated sizes
  const size_t M = xs.size(), E = es.size(), NL = P.n_lookups, R = P.n_reads, C = P.n_class;
  std::vector<uint8_t> entry_bits(E, 7), rd_bits(R, 7), xfer_flags(M, 7);
  std::vector<uint32_t> lk_counts(NL * 9, 7), lk_present(NL, 7), rd_first(R * 2, 7), xp(M, 7), xe(M, 7), xl(M, 7), xv(M, 7);
  std::vector<int64_t> lk_vector(NL * C, 7);
  tbc_ledger_journal_out out{};
  out.entry_bits = entry_bits.data(); out.lk_counts = lk_counts.data(); out.lk_present = lk_present.data(); out.lk_vector = lk_vector.data();
  out.rd_bits = rd_bits.data(); out.rd_first = rd_first.data(); out.xfer_present = xp.data(); out.xfer_early = xe.data(); out.xfer_lost = xl.data();
  out.xfer_vanished = xv.data(); out.xfer_flags = xfer_flags.data();
  CHECK(emu_journal_check(&rin, &out, grid_cap, 3 + M, slice_entries, chunk) == 0);
  const tbc_ledger_journal_summary& s = out.summary;
  std::map<int64_t, size_t> first_of;
  for (size_t m = 0; m < M; m++) first_of.emplace(in.mop_id[xs[m]], m);
  CHECK(s.n_xfer_mops == M && s.n_entries == E && s.n_lookups == NL && s.read_count == R && s.n_records == first_of.size() && s.n_reinvoked == M - first_of.size());
  uint64_t present = 0, per_record = 0, totals[9] = {0};
  for (size_t l = 0; l < NL; l++) { present += lk_present[l]; for (int k = 0; k < 9; k++) totals[k] += lk_counts[l * 9 + k]; }
  for (size_t m = 0; m < M; m++) {
    const bool record = first_of[in.mop_id[xs[m]]] == m;
    CHECK(xfer_flags[m] == ((record ? 0 : 1) | ((in.mop_flags[xs[m]] & 1) ? 2 : 0)) && (record || (xp[m] | xe[m] | xl[m] | xv[m]) == 0));
    per_record += xp[m];
  }
  CHECK(present == per_record);                                               // the lookups' present records are the records' lookups
  uint64_t unknown = 0, known = 0;
  for (size_t e = 0; e < E; e++) { CHECK(entry_bits[e] <= 2); unknown += entry_bits[e] == 1; known += first_of.count(in.mop_id[es[e]]); }
  CHECK(unknown == E - known && totals[TBC_LEDGER_JN_UNKNOWN] == unknown && totals[TBC_LEDGER_JN_REPEATED] == known - present);
  for (int k = 0; k < 9; k++) CHECK(s.totals[k] == totals[k]);
  CHECK(s.bytes_in == img.size());
}

// ---- the launches: the sequence over the recorder (it reads the plan's numbers alone, so the arguments are made directly)
lgjn::JnArgs shape(uint32_t n_xfer, uint32_t n_slices, uint32_t n_lookups, uint32_t n_reads, uint32_t n_class, uint32_t chunk = 256) {
  lgjn::JnArgs A{};
  A.n_xfer = n_xfer; A.n_slices = n_slices; A.n_lookups = n_lookups; A.n_reads = n_reads; A.n_class = n_class; A.chunk = chunk;
  return A;
}

void launches() {
  using R = emu::Recorder;
  constexpr uint32_t W = lgjn::kJnWindowWords;
  const R::Kernel claim = R::of(jn_claim_kernel), records = R::of(jn_records_kernel), entries = R::of(jn_entries_kernel<W>), members = R::of(jn_members_kernel),
                  books = R::of(jn_books_kernel), reads = R::of(jn_reads_kernel), count = R::of(jn_count_kernel), worst = R::of(jn_worst_kernel), summary = R::of(jn_summary_kernel);
  const auto seq = [](const lgjn::JnArgs& A) { R go; lgjn::sequence<W>(go, A); return go; };
  // nothing at all: only the summary
  CHECK(seq(shape(0, 0, 0, 0, 16)).is({{summary, 1, 64}}));
  // transfers alone: the table, the records, the members (they store the records' zeros); reads alone: the reads kernel (it counts what they check)
  CHECK(seq(shape(300, 0, 0, 0, 16)).is({{claim, 2, 256}, {records, 2, 256}, {members, 2, 256}, {summary, 1, 64}}));
  CHECK(seq(shape(0, 0, 0, 9, 16)).is({{reads, 3, 256}, {summary, 1, 64}}));
  // lookups without transfers: every entry is unknown; lookups without entries: no entries kernel; no accounts: a thread per lookup of the books
  CHECK(seq(shape(0, 2, 2, 0, 16)).is({{entries, 2, 256}, {books, 1, 256}, {count, 1, 256}, {worst, 1, 256}, {summary, 1, 64}}));
  CHECK(seq(shape(5, 0, 3, 0, 0)).is({{claim, 1, 256}, {records, 1, 256}, {members, 1, 256}, {books, 1, 256}, {count, 1, 256}, {worst, 1, 256}, {summary, 1, 64}}));
  // everything, chunks of 64: 300 micro-ops are 5 chunks; 80 lookups x 16 counters are 5 blocks of the books
  CHECK(seq(shape(300, 7, 80, 1000, 16, 64)).is({{claim, 2, 256}, {records, 2, 256}, {entries, 7, 256}, {members, 5, 256}, {books, 5, 256}, {reads, 250, 256},
                                                   {count, 1, 256}, {worst, 1, 256}, {summary, 1, 64}}));
  // one past each cap
  const lgjn::JnArgs big = shape(2049u * 256u, 2049, 4097u * 256u, 2049u * 4u, 2);
  CHECK(seq(big).is({{claim, 2048, 256}, {records, 2048, 256}, {entries, 2048, 256}, {members, 2048, 256}, {books, 8194, 256}, {reads, 2048, 256},
                     {count, 4096, 256}, {worst, 4096, 256}, {summary, 1, 64}}));
}

void refuse(const tbc_ledger_rt_in& in, const char* needle, bool by_plan = false) {
  std::string err;
  lgjn::Plan P;
  if (by_plan) CHECK(!lgjn::plan("tbc_ledger_journal", &in, P, err));
  else CHECK(!lgjn::validate("tbc_ledger_journal", &in, err));
  if (err.find(needle) == std::string::npos || err.find("tbc_ledger_journal") != 0) { std::printf("FAILED: message '%s' lacks '%s'\n", err.c_str(), needle); std::exit(1); }
}

}  // namespace

int main() {
  int planned = 0;
  for (uint32_t n_ops : {0u, 1u, 2u, 17u, 200u, 900u})
    for (uint32_t n_acc : {0u, 1u, 3u, 20u})
      for (uint32_t knobs : {0u, 1u}) {
        rng_state = 77 + n_ops * 31 + n_acc * 7 + knobs;
        look(make(n_ops, n_acc), knobs ? 2u : 3u, knobs ? 5u : 0u, knobs ? 64u : 0u);
        planned++;
      }
  // ---- the plan reads no micro-op: the columns are not there
  {
    Ledger L = make(400, 4);
    tbc_ledger_rt_in s = L.in();
    s.ledger.mop_id = s.ledger.mop_a = s.ledger.mop_b = s.ledger.mop_c = reinterpret_cast<const int64_t*>(8);      // (never dereferenced)
    s.ledger.mop_flags = reinterpret_cast<const uint8_t*>(8);
    std::string err;
    lgjn::Plan P;
    CHECK(lgjn::plan("plan", &s, P, err) && P.xf.n_mops > 0 && P.lk.n_mops > 0 && P.rd.n_mops > 0);
    planned++;
  }
  // ---- refusals: realtime's rules under this entry point's name, then the plan's own
  int refusals = 0;
  Ledger L = make(60, 3);
  { tbc_ledger_rt_in s = L.in(); s.process = nullptr; refuse(s, "null argument (process)"); refusals++; }
  { tbc_ledger_rt_in s = L.in(); s.ok_transfers_apply = 2; refuse(s, "ok_transfers_apply is 0 or 1"); refusals++; }
  { Ledger M = L; M.init_d[1] = -(1ll << 61); refuse(M.in(), "2^61"); refusals++; }
  { Ledger M = L; M.type[1] = 4; refuse(M.in(), "op 1 (index"); refusals++; }
  const auto hollow = [](Ledger& M) {                                          // (micro-ops that are counted and never read)
    tbc_ledger_rt_in s = M.in();
    s.ledger.mop_id = s.ledger.mop_a = s.ledger.mop_b = s.ledger.mop_c = reinterpret_cast<const int64_t*>(8);
    s.ledger.mop_flags = reinterpret_cast<const uint8_t*>(8);
    return s;
  };
  {                                                                           // (2^31 transfer micro-ops: refused before anything is sized by them)
    Ledger X; X.op(TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_TRANSFER, 0); X.end(); X.mop_off[1] = 1ull << 31;
    refuse(hollow(X), "2^31 or more transfer micro-ops", true); refusals++;
  }
  for (const uint64_t n : {(1ull << 31) - 1ull, 1ull << 31}) {
    std::string err;
    lgjn::Plan P;
    Ledger E; E.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_LOOKUP, 0); E.end(); E.mop_off[1] = n;
    if (n < (1ull << 31)) { const tbc_ledger_rt_in s = hollow(E); CHECK(lgjn::plan("x", &s, P, err) && P.lk.n_mops == n && P.n_slices == 524288); }
    else { refuse(hollow(E), "a lookup of 2^31 or more entries", true); refuse(hollow(E), "op 0 (index 2)", true); refusals++; }
  }
  for (const uint32_t lookups : {65535u, 65536u}) {                           // lookups x words of 2^31: 2^20 micro-ops are 2^15 words
    Ledger X; X.op(TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_TRANSFER, 0); X.end(); X.mop_off[1] = 1ull << 20;
    for (uint32_t l = 0; l < lookups; l++) { X.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_LOOKUP, 1); X.mop_off.push_back(1ull << 20); }
    std::string err;
    lgjn::Plan P;
    if (lookups == 65535u) { const tbc_ledger_rt_in s = hollow(X); CHECK(lgjn::plan("x", &s, P, err) && P.arena.bitmap.bytes == (size_t)65535 * (1u << 15) * 4); }
    else { refuse(hollow(X), "lookups x words of transfer micro-ops (65536 x 32768) is 2^31 or more", true); refusals++; }
  }
  {
    Ledger X;
    for (uint32_t k = 0; k < 32768u; k++) { X.accounts.push_back(k); X.init_c.push_back(0); X.init_d.push_back(0); }
    for (uint32_t i = 0; i < 32768u; i++) { X.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_READ, 0); X.end(); }
    refuse(X.in(), "reads x counters or lookups x counters", true); refusals++;
  }
  launches();
  std::printf("%d ledgers planned, run and checked, %d refusals, the launches of 7 shapes\n", planned, refusals);
  return 0;
}
