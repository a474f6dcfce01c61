// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  ledger_rt_plan.cpp: the host side of tbc_ledger_realtime without a device -- the validation
// and the plan of csrc/ledger_rt_plan.h (the very functions ledger_rt_host.hip runs every call through) in a program of its own, the one
// to build with -fsanitize=address,undefined (tests/test_ledger_realtime_plan.py does):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include -I tests/emu -I jepsen-tigerbeetle_amd/csrc tests/emu/ledger_rt_plan.cpp -o ledger_rt_plan && ./ledger_rt_plan
// It builds ledgers of many shapes (seeded), plans them and checks what can be checked without Python: pairing and statuses against a
// plain restatement, the three streams (order, positions, running lengths), the reads' invocations, the gathered micro-ops (spans, image), the sorted accounts
// with init permuted, the chunks, the arena's regions; then it breaks each rule in turn and looks at the message.  The columns are exactly as
// long as the struct says, so a read past an end is the sanitizer's to see -- and the transfers' micro-op columns are NOT THERE AT ALL
// where only transfers have micro-ops (null pointers behind a fence of the reads' own), so the plan cannot have read one.  And because
// it includes the emulator program of the kernels (emu_ledger_rt.cpp), it holds lgrt::sequence -- the launches the library makes -- to
// the list of (kernel, grid, threads) written out below by hand, under the device's caps, on the edge shapes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "emu_ledger_rt.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

namespace {

struct Ledger {
  std::vector<uint32_t> index;
  std::vector<uint8_t> type, kind, flags, mop_flags;
  std::vector<int32_t> process;
  std::vector<uint64_t> mop_off{0};
  std::vector<int64_t> id, a, b, c, accounts, init_c, init_d;
  uint32_t apply = 1;
  tbc_ledger_rt_in in() const {
    tbc_ledger_rt_in r{};
    tbc_ledger_in& s = r.ledger;
    s.n_ops = (uint32_t)index.size(); s.index = index.data(); s.type = type.data(); s.kind = kind.data(); s.flags = flags.data();
    s.mop_off = mop_off.data(); s.mop_id = id.data(); s.mop_a = a.data(); s.mop_b = b.data(); s.mop_c = c.data(); s.mop_flags = mop_flags.data();
    s.accounts = accounts.data(); s.n_accounts = (uint32_t)accounts.size();
    r.process = process.data(); r.init_credits = init_c.empty() ? nullptr : init_c.data(); r.init_debits = init_d.empty() ? nullptr : init_d.data();
    r.ok_transfers_apply = apply;
    return r;
  }
  void op(int32_t p, uint8_t t, uint8_t k, uint32_t n_mops) {
    index.push_back(index.empty() ? 2u : index.back() + 1u + (uint32_t)(n_mops % 2));
    process.push_back(p); type.push_back(t); kind.push_back(k); flags.push_back(0);
    for (uint32_t m = 0; m < n_mops; m++) { id.push_back(k == TBC_LEDGER_K_READ ? (int64_t)(m + 1) * 3 : (int64_t)id.size() + 1000); a.push_back(1); b.push_back(2); c.push_back(1); mop_flags.push_back(0); }
    mop_off.push_back(id.size());
  }
};

uint64_t rng_state = 1;
uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

Ledger make(uint32_t n_ops, uint32_t n_accounts, uint32_t n_procs) {
  Ledger L;
  for (uint32_t k = 0; k < n_accounts; k++) { L.accounts.push_back((int64_t)(n_accounts - k) * 3); L.init_c.push_back(100 + k); L.init_d.push_back(-(int64_t)k); }   // (unsorted)
  for (uint32_t i = 0; i < n_ops; i++) {
    const uint8_t t = (uint8_t)rnd(4), k = (uint8_t)rnd(4);
    const bool copied = (t == TBC_LEDGER_T_INVOKE && k == TBC_LEDGER_K_TRANSFER) || (t == TBC_LEDGER_T_OK && k >= TBC_LEDGER_K_READ);
    L.op((int32_t)rnd(n_procs) - 1, t, k, copied ? (k == TBC_LEDGER_K_READ ? rnd(6) : 1 + rnd(3)) : 0);
  }
  return L;
}

void look(const Ledger& L) {
  const tbc_ledger_rt_in rin = L.in();
  const tbc_ledger_in& in = rin.ledger;
  std::string err;
  CHECK(lgrt::validate("plan", &rin, err));
  lgrt::Plan P;
  CHECK(lgrt::plan("plan", &rin, P, err));
  // pairing and statuses, restated: a map from process to its open invocation
  std::map<int32_t, uint32_t> open;
  std::vector<uint32_t> partner(in.n_ops, lgrt::kRtNone);
  for (uint32_t i = 0; i < in.n_ops; i++) {
    if (in.type[i] == TBC_LEDGER_T_INVOKE) { open[rin.process[i]] = i; continue; }
    if (open.count(rin.process[i])) { const uint32_t j = open[rin.process[i]]; partner[j] = i; partner[i] = j; open.erase(rin.process[i]); }
  }
  CHECK(partner == P.partner);
  // the possible stream: invocation order; the definite stream: completion order; the reads
  // the micro-ops the device gets: those of the :ok reads and of the transfers that did not fail, numbered in the caller's order
  std::vector<uint64_t> at(in.n_ops, 0), src;
  for (uint32_t i = 0; i < in.n_ops; i++) {
    const bool failed = partner[i] != lgrt::kRtNone && in.type[partner[i]] == TBC_LEDGER_T_FAIL;
    if (!((in.type[i] == TBC_LEDGER_T_INVOKE && in.kind[i] == TBC_LEDGER_K_TRANSFER && !failed) || (in.type[i] == TBC_LEDGER_T_OK && in.kind[i] == TBC_LEDGER_K_READ))) continue;
    at[i] = src.size();
    for (uint64_t m = in.mop_off[i]; m < in.mop_off[i + 1]; m++) src.push_back(m);
  }
  CHECK(P.n_mops == src.size());
  {
    uint64_t covered = 0;
    for (size_t k = 0; k < P.spans.size(); k++) {
      const oneshot::Span& s = P.spans[k];
      CHECK(s.n > 0 && s.dst == covered && (k == 0 || P.spans[k - 1].src + P.spans[k - 1].n < s.src));       // (neighbours are merged)
      for (uint64_t j = 0; j < s.n; j++) CHECK(src[s.dst + j] == s.src + j);
      covered += s.n;
    }
    CHECK(covered == src.size());
  }
  size_t np = 0, nd = 0, nr = 0;
  for (uint32_t i = 0; i < in.n_ops; i++) {
    const uint64_t lo = at[i], n = in.mop_off[i + 1] - in.mop_off[i];
    if (in.type[i] == TBC_LEDGER_T_INVOKE && in.kind[i] == TBC_LEDGER_K_TRANSFER) {
      const uint8_t status = partner[i] == lgrt::kRtNone ? (uint8_t)TBC_LEDGER_T_INVOKE : in.type[partner[i]];
      CHECK(P.status[i] == status);
      if (status != TBC_LEDGER_T_FAIL) {
        const lgrt::Rows& R = P.rows[lgrt::kPossible];
        CHECK(np < R.lo.size() && R.lo[np] == lo && R.cum[np + 1] - R.cum[np] == n && R.pos[np] == in.index[i]); np++;
      }
    }
    if (in.type[i] == TBC_LEDGER_T_OK && partner[i] != lgrt::kRtNone && in.kind[partner[i]] == TBC_LEDGER_K_TRANSFER) {
      const uint32_t j = partner[i];
      const lgrt::Rows& R = P.rows[lgrt::kDefinite];
      CHECK(nd < R.lo.size() && R.lo[nd] == at[j] && R.cum[nd + 1] - R.cum[nd] == in.mop_off[j + 1] - in.mop_off[j] && R.pos[nd] == in.index[i]); nd++;
    }
    if (in.type[i] == TBC_LEDGER_T_OK && in.kind[i] == TBC_LEDGER_K_READ) {
      const lgrt::Rows& R = P.rows[lgrt::kReads];
      CHECK(nr < R.lo.size() && R.lo[nr] == lo && R.cum[nr + 1] - R.cum[nr] == n && R.pos[nr] == in.index[i]);
      CHECK(P.read_inv[nr] == (partner[i] == lgrt::kRtNone ? 0u : in.index[partner[i]])); nr++;
    }
  }
  CHECK(np == P.rows[lgrt::kPossible].lo.size() && nd == P.rows[lgrt::kDefinite].lo.size() && nr == P.n_reads && nr == P.read_inv.size());
  for (const lgrt::Rows& R : P.rows) {
    for (size_t k = 1; k < R.pos.size(); k++) CHECK(R.pos[k - 1] < R.pos[k]);                       // ascending position order
    CHECK(R.chunk_entries % 64 == 0 && R.chunk_entries >= 64 && (uint64_t)R.n_chunks * R.chunk_entries >= 2 * R.mops());
    CHECK(R.n_chunks == (2 * R.mops() + R.chunk_entries - 1) / R.chunk_entries && (uint64_t)R.n_chunks * P.n_class <= std::max<uint64_t>(lgrt::kRtCarryWords, P.n_class));
  }
  // the accounts sorted, init permuted to match
  CHECK(P.n_class == 2 * in.n_accounts && P.init.size() == 2 * (size_t)in.n_accounts);
  for (size_t k = 0; k < P.accounts.size(); k++) {
    if (k) CHECK(P.accounts[k - 1] < P.accounts[k]);
    size_t src = 0;
    while (in.accounts[src] != P.accounts[k]) src++;
    CHECK(P.init[k] == (rin.init_credits ? rin.init_credits[src] : 0) && P.init[in.n_accounts + k] == (rin.init_debits ? rin.init_debits[src] : 0));
  }
  // the arena: regions in order, 256 B starts, none overlapping, sized for what they hold
  const oneshot::Region* reg = reinterpret_cast<const oneshot::Region*>(&P.arena);
  const size_t n_reg = offsetof(lgrt::RtArena, bytes) / sizeof(oneshot::Region);
  for (size_t k = 0; k < n_reg; k++) CHECK(reg[k].at % 256 == 0 && reg[k].at + reg[k].bytes <= (k + 1 < n_reg ? reg[k + 1].at : P.arena.bytes));
  const lgrt::RtArena& A = P.arena;
  CHECK(A.mop_id.bytes == P.n_mops * 8 && A.mop_flags.bytes == P.n_mops && A.rt_bits.bytes % 4 == 0 && A.rt_bits.bytes >= P.n_reads && A.rt_miss.bytes == (size_t)P.n_reads * 24);
  for (int k = 0; k < lgrt::kStreams; k++) {
    const size_t E = 2 * (size_t)P.rows[k].mops();
    CHECK(A.ent_cls[k].bytes == E * 4 && A.ent_val[k].bytes == E * 8 && A.list_pos[k].bytes == E * 4 && A.list_val[k].bytes == E * 8);
    CHECK(A.carry_cnt[k].bytes == (size_t)P.rows[k].n_chunks * P.n_class * 4 && A.carry_val[k].bytes == 2 * A.carry_cnt[k].bytes && A.off[k].bytes == (P.n_class + 1) * 4);
  }
  CHECK(A.mop_lo.bytes == P.rows[lgrt::kReads].mops() * 16 && A.zero_bytes() == A.summary.at - A.carry_cnt[0].at && A.image_bytes() == A.carry_cnt[0].at);
  const std::vector<unsigned char> img = lgrt::image(&rin, P);
  CHECK(img.size() == A.image_bytes());
  for (size_t m = 0; m < src.size(); m++) {                                                         // the columns, gathered
    int64_t v[4];
    std::memcpy(&v[0], img.data() + A.mop_id.at + m * 8, 8); std::memcpy(&v[1], img.data() + A.mop_a.at + m * 8, 8);
    std::memcpy(&v[2], img.data() + A.mop_b.at + m * 8, 8); std::memcpy(&v[3], img.data() + A.mop_c.at + m * 8, 8);
    CHECK(v[0] == in.mop_id[src[m]] && v[1] == in.mop_a[src[m]] && v[2] == in.mop_b[src[m]] && v[3] == in.mop_c[src[m]] && img[A.mop_flags.at + m] == in.mop_flags[src[m]]);
  }
  lgrt::RtAcc acc;
  std::memcpy(&acc, img.data() + A.acc.at, sizeof acc);
  CHECK(acc.first[2] == lgrt::kRtNone && acc.worst[0] == lgrt::kRtNone && acc.first_error == lgrt::kRtNone && acc.count[1] == 0 && acc.worst_miss[2] == 0);
  if (P.n_reads) CHECK(std::memcmp(img.data() + A.read_inv.at, P.read_inv.data(), P.n_reads * 4) == 0);
  // the kernels' arguments point into the arena
  std::vector<char> fake(16);
  const lgrt::RtArgs K = lgrt::args(&rin, P, fake.data());
  CHECK((const char*)K.mop_floor == fake.data() + A.mop_floor.at && K.s[lgrt::kReads].n_entries == 2 * P.rows[lgrt::kReads].mops() && K.n_read_mops == P.rows[lgrt::kReads].mops());
}

// ---- the launches: lgrt::sequence over the recorder (it reads the plan's numbers alone, so the arguments are made directly)
struct StreamShape { uint64_t entries; uint32_t chunks; };
lgrt::RtArgs shape(StreamShape definite, StreamShape possible, StreamShape reads, uint32_t n_class, uint64_t read_mops, uint32_t n_reads) {
  lgrt::RtArgs A{};
  const StreamShape s[lgrt::kStreams] = {definite, possible, reads};
  for (int k = 0; k < lgrt::kStreams; k++) { A.s[k].n_entries = s[k].entries; A.s[k].n_chunks = s[k].chunks; }
  A.n_class = n_class; A.n_read_mops = read_mops; A.n_reads = n_reads;
  return A;
}

void launches() {
  using R = emu::Recorder;
  const R::Kernel number = R::of(rt_number_kernel<false>), carry = R::of(rt_carry_kernel<false>), scan = R::of(rt_scan_kernel<false>),
                  number_r = R::of(rt_number_kernel<true>), carry_r = R::of(rt_carry_kernel<true>), scan_r = R::of(rt_scan_kernel<true>),
                  offsets = R::of(rt_offsets_kernel), query = R::of(rt_query_kernel), count = R::of(rt_count_kernel), worst = R::of(rt_worst_kernel),
                  summary = R::of(rt_summary_kernel);
  const auto record = [](const lgrt::RtArgs& A) { R go; lgrt::sequence(go, A); return go; };
  // no ops: only the summary
  CHECK(record(shape({0, 0}, {0, 0}, {0, 0}, 0, 0, 0)).is({{summary, 1, 64}}));
  // no accounts: of a stream the numbering only (it counts the sides and the amounts); reads without a micro-op are counted still
  CHECK(record(shape({10, 1}, {200, 4}, {0, 0}, 0, 0, 3)).is({{number, 1, 64}, {number, 4, 64}, {count, 1, 256}, {worst, 1, 256}, {summary, 1, 64}}));
  // all of it: three streams of four kernels, the query, the counts
  CHECK(record(shape({200, 2}, {300, 3}, {600, 5}, 6, 300, 40)).is(
      {{number, 2, 64}, {carry, 6, 256}, {offsets, 1, 256}, {scan, 2, 64}, {number, 3, 64}, {carry, 6, 256}, {offsets, 1, 256}, {scan, 3, 64},
       {number_r, 5, 64}, {carry_r, 6, 256}, {offsets, 1, 256}, {scan_r, 5, 64}, {query, 2, 256}, {count, 1, 256}, {worst, 1, 256}, {summary, 1, 64}}));
  // transfers but no read: two streams, no query, no counts
  CHECK(record(shape({128, 2}, {128, 2}, {0, 0}, 2, 0, 0)).is(
      {{number, 2, 64}, {carry, 2, 256}, {offsets, 1, 256}, {scan, 2, 64}, {number, 2, 64}, {carry, 2, 256}, {offsets, 1, 256}, {scan, 2, 64}, {summary, 1, 64}}));
  // one past each cap: 8,193 chunks, 4,097 classes, 16,385 x 256 read micro-ops, 16,385 x 256 reads
  CHECK(record(shape({0, 0}, {0, 0}, {8193ull * 64, 8193}, 4097, 16385ull * 256, 16385u * 256u)).is(
      {{number_r, 8192, 64}, {carry_r, 4096, 256}, {offsets, 1, 256}, {scan_r, 8192, 64}, {query, 16384, 256}, {count, 16384, 256}, {worst, 16384, 256}, {summary, 1, 64}}));
}

void refuse(tbc_ledger_rt_in in, const char* needle) {
  std::string err;
  CHECK(!lgrt::validate("tbc_ledger_realtime", &in, err));
  if (err.find(needle) == std::string::npos || err.find("tbc_ledger_realtime") != 0) { std::printf("FAILED: message '%s' lacks '%s'\n", err.c_str(), needle); std::exit(1); }
}

}  // namespace

int main() {
  int planned = 0;
  for (uint32_t n_ops : {0u, 1u, 2u, 17u, 300u, 3000u})
    for (uint32_t n_acc : {0u, 1u, 8u, 70u})
      for (uint32_t n_procs : {1u, 3u, 40u}) { rng_state = 91 + n_ops * 31 + n_acc * 7 + n_procs; look(make(n_ops, n_acc, n_procs)); planned++; }
  // ---- the plan never reads a transfer's micro-ops: a ledger of transfers alone, its micro-op columns absent
  {
    Ledger L;
    L.accounts = {3, 6};
    for (int i = 0; i < 40; i++) { L.op(i % 5, TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_TRANSFER, 2); if (i % 3) L.op(i % 5, (uint8_t)(1 + i % 3), TBC_LEDGER_K_TRANSFER, 0); }
    tbc_ledger_rt_in s = L.in();
    std::string err;
    lgrt::Plan P;
    std::vector<int64_t> none;
    s.ledger.mop_id = s.ledger.mop_a = s.ledger.mop_b = s.ledger.mop_c = reinterpret_cast<const int64_t*>(8);      // (never dereferenced)
    CHECK(lgrt::validate("plan", &s, err) && lgrt::plan("plan", &s, P, err) && P.rows[lgrt::kPossible].mops() > 0);
    planned++;
  }
  // ---- every rule, broken in turn
  Ledger L;
  L.accounts = {3, 6, 9}; L.init_c = {1, 2, 3}; L.init_d = {0, 0, 0};
  for (int i = 0; i < 4; i++) { L.op(i, TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_TRANSFER, 1); L.op(i, TBC_LEDGER_T_OK, TBC_LEDGER_K_TRANSFER, 0); }
  L.op(7, TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_READ, 0);
  L.op(7, TBC_LEDGER_T_OK, TBC_LEDGER_K_READ, 3);
  look(L);
  { tbc_ledger_rt_in s = L.in(); s.process = nullptr; refuse(s, "null argument (process)"); }
  { tbc_ledger_rt_in s = L.in(); s.ok_transfers_apply = 2; refuse(s, "ok_transfers_apply is 0 or 1"); }
  { Ledger M = L; M.init_c[1] = (int64_t)1 << 61; refuse(M.in(), "initial value of account 6"); }
  { Ledger M = L; M.init_d[2] = -((int64_t)1 << 61); refuse(M.in(), "initial value of account 9"); }
  { Ledger M = L; M.init_d[2] = -((int64_t)1 << 61) + 1; std::string e; const tbc_ledger_rt_in s = M.in(); CHECK(lgrt::validate("x", &s, e)); }
  // ... and the rules of tbc_ledger_in, which it shares (ledger_plan.h states them; here: they are checked under this entry point's name)
  { tbc_ledger_rt_in s = L.in(); s.ledger.mop_off = nullptr; refuse(s, "null argument"); }
  { tbc_ledger_rt_in s = L.in(); s.ledger.accounts = nullptr; refuse(s, "null argument (accounts)"); }
  { Ledger M = L; M.index[4] = M.index[3]; refuse(M.in(), "op 4 (index"); refuse(M.in(), "strictly ascending"); }
  { Ledger M = L; M.type[1] = 4; refuse(M.in(), "type is not"); }
  { Ledger M = L; M.kind[1] = 4; refuse(M.in(), "kind is not"); }
  { Ledger M = L; M.accounts = {3, 6, 3}; refuse(M.in(), "account 3 is listed twice"); }
  { Ledger M = L; M.id[5] = M.id[4]; refuse(M.in(), "names an id twice"); }
  { Ledger M = L; M.mop_flags[5] = 2; refuse(M.in(), "unknown micro-op flags"); }
  // ---- the one refusal the plan itself makes: 2^31 micro-ops of transfers, or of reads, in one call (the device's entry and list
  // numbers are 32 bits, two entries a micro-op).  The plan reads no micro-op, so the columns need not be there.
  for (const uint8_t kind : {(uint8_t)TBC_LEDGER_K_TRANSFER, (uint8_t)TBC_LEDGER_K_READ})
    for (const uint64_t n : {(1ull << 31) - 1ull, 1ull << 31}) {
      Ledger M;
      M.accounts = {3};
      M.op(0, kind == TBC_LEDGER_K_TRANSFER ? TBC_LEDGER_T_INVOKE : TBC_LEDGER_T_OK, kind, 0);
      M.mop_off[1] = n;
      tbc_ledger_rt_in s = M.in();
      s.ledger.mop_id = s.ledger.mop_a = s.ledger.mop_b = s.ledger.mop_c = reinterpret_cast<const int64_t*>(8);      // (never dereferenced)
      s.ledger.mop_flags = reinterpret_cast<const uint8_t*>(8);
      std::string err;
      lgrt::Plan P;
      const bool ok = lgrt::plan("tbc_ledger_realtime", &s, P, err);
      if (n < (1ull << 31)) { CHECK(ok && P.n_mops == n && P.rows[kind == TBC_LEDGER_K_TRANSFER ? lgrt::kPossible : lgrt::kReads].mops() == n); continue; }
      CHECK(!ok);
      if (err.find("2^31 or more micro-ops of transfers, or of reads, in one call") == std::string::npos || err.find("tbc_ledger_realtime") != 0) { std::printf("FAILED: message '%s'\n", err.c_str()); std::exit(1); }
    }
  // ---- a cap on the chunks makes them longer, never fewer entries than the stream has
  {
    const Ledger B = make(3000, 8, 40);
    const tbc_ledger_rt_in s = B.in();
    std::string err;
    lgrt::Plan P;
    CHECK(lgrt::plan("plan", &s, P, err, 2));
    for (const lgrt::Rows& R : P.rows) CHECK(R.n_chunks <= 2 && R.chunk_entries % 64 == 0 && (uint64_t)R.n_chunks * R.chunk_entries >= 2 * R.mops());
    CHECK(P.rows[lgrt::kReads].chunk_entries > 64);
  }
  launches();
  std::printf("%d ledgers planned and checked, 15 refusals, the launches of 5 shapes\n", planned + 1);
  return 0;
}
