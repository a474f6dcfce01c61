// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  ledger_snap_plan.cpp: the host side of tbc_ledger_snapshots without a device -- the validation
// and the plan of csrc/ledger_snap_plan.h (the very functions ledger_snap_host.hip runs every call through) in a program of its own, the
// one to build with -fsanitize=address,undefined (tests/test_ledger_snapshots_plan.py does):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include -I tests/emu -I jepsen-tigerbeetle_amd/csrc tests/emu/ledger_snap_plan.cpp -o ledger_snap_plan && ./ledger_snap_plan
// It builds ledgers of many shapes (seeded), plans them and checks what can be checked without Python: the reads' rows, the gathered
// micro-ops (spans, image: id, a, b and flags, never c), the sorted accounts with their positions, the chunks of the sort and of the
// scan, the arena's regions; it shows that the plan reads no micro-op (the columns are not there); it breaks each rule in turn and looks
// at the message, the plan's own two refusals included.  And because it includes the emulator program of the kernels
// (emu_ledger_snap.cpp), it runs every kernel of csrc/ledger_snap_kernels.h on each ledger under the sanitizers too -- an index past an
// array's end in a kernel is the sanitizer's to see -- and holds the result to a plain pair-by-pair restatement of the rules; and it
// holds lgsn::filter_sequence and lgsn::rest_sequence -- the launches the library makes -- to the list of (kernel, grid, threads) written
// out below by hand, under the device's caps, on the edge shapes.
#include <cstdio>
#include <cstdlib>
#include <map>
#include "emu_ledger_snap.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

namespace {

struct Ledger {
  std::vector<uint32_t> index;
  std::vector<uint8_t> type, kind, flags, mop_flags;
  std::vector<uint64_t> mop_off{0};
  std::vector<int64_t> id, a, b, c, accounts;
  tbc_ledger_in in() const {
    tbc_ledger_in s{};
    s.n_ops = (uint32_t)index.size(); s.index = index.data(); s.type = type.data(); s.kind = kind.data(); s.flags = flags.data();
    s.mop_off = mop_off.data(); s.mop_id = id.data(); s.mop_a = a.data(); s.mop_b = b.data(); s.mop_c = c.data(); s.mop_flags = mop_flags.data();
    s.accounts = accounts.data(); s.n_accounts = (uint32_t)accounts.size();
    return s;
  }
  void op(uint8_t t, uint8_t k) {
    index.push_back(index.empty() ? 2u : index.back() + 1u + (uint32_t)(id.size() % 2));
    type.push_back(t); kind.push_back(k); flags.push_back(0);
  }
  void mop(int64_t ident, int64_t va, int64_t vb, uint8_t fl = 0) { id.push_back(ident); a.push_back(va); b.push_back(vb); c.push_back(77); mop_flags.push_back(fl); }
  void end() { mop_off.push_back(id.size()); }
};

uint64_t rng_state = 1;
uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

// reads of small random counters (so that sums tie and reads are skewed), some lacking an account, holding a nil micro-op or a foreign
// id, among ops of every other type and kind
Ledger make(uint32_t n_ops, uint32_t n_accounts) {
  Ledger L;
  for (uint32_t k = 0; k < n_accounts; k++) L.accounts.push_back((int64_t)(n_accounts - k) * 3);                     // (unsorted)
  for (uint32_t i = 0; i < n_ops; i++) {
    const uint8_t t = (uint8_t)rnd(4), k = (uint8_t)(rnd(3) ? (uint32_t)TBC_LEDGER_K_READ : rnd(4));
    L.op(t, k);
    if (t == TBC_LEDGER_T_OK && k == TBC_LEDGER_K_READ) {
      const uint32_t how = rnd(8);
      for (uint32_t j = 0; j < n_accounts; j++) {
        if (how == 0 && j == n_accounts / 2) continue;
        if (how == 1 && j == 0) { L.mop(1000 + (int64_t)i, 1, 1); continue; }
        L.mop(L.accounts[j], (int64_t)rnd(4) - 1, (int64_t)rnd(4) - 1, how == 2 && j + 1 == n_accounts ? TBC_LEDGER_M_NIL : 0);
      }
    } else if ((t == TBC_LEDGER_T_INVOKE && k == TBC_LEDGER_K_TRANSFER) || (t == TBC_LEDGER_T_OK && k == TBC_LEDGER_K_LOOKUP)) {
      for (uint32_t j = 0; j < 1 + rnd(3); j++) L.mop(5000 + (int64_t)L.id.size(), 3, 6);
    }
    L.end();
  }
  return L;
}

void look(const Ledger& L, uint32_t grid_cap, uint32_t sort_cap, uint32_t scan_rows) {
  const tbc_ledger_in in = L.in();
  std::string err;
  CHECK(lgsn::validate("plan", &in, err));
  lgsn::Plan P;
  CHECK(lgsn::plan("plan", &in, P, err));
  // the reads' rows and the micro-ops the device gets, restated
  std::vector<uint64_t> src, cum{0};
  for (uint32_t i = 0; i < in.n_ops; i++) {
    if (in.type[i] != TBC_LEDGER_T_OK || in.kind[i] != TBC_LEDGER_K_READ) continue;
    for (uint64_t m = in.mop_off[i]; m < in.mop_off[i + 1]; m++) src.push_back(m);
    cum.push_back(src.size());
  }
  CHECK(P.n_mops == src.size() && P.row_cum == cum && P.n_reads == cum.size() - 1);
  uint64_t covered = 0;
  for (size_t k = 0; k < P.spans.size(); k++) {
    const oneshot::Span& s = P.spans[k];
    CHECK(s.n > 0 && s.dst == covered && (k == 0 || P.spans[k - 1].src + P.spans[k - 1].n < s.src));       // (neighbours are merged)
    for (uint64_t j = 0; j < s.n; j++) CHECK(src[s.dst + j] == s.src + j);
    covered += s.n;
  }
  CHECK(covered == src.size());
  // the accounts sorted, each with its position in the caller's list
  CHECK(P.n_class == 2 * in.n_accounts && P.n_words == (P.n_class + 31) / 32 && P.accounts.size() == in.n_accounts && P.acct_pos.size() == in.n_accounts);
  for (size_t k = 0; k < P.accounts.size(); k++) {
    if (k) CHECK(P.accounts[k - 1] < P.accounts[k]);
    CHECK(in.accounts[P.acct_pos[k]] == P.accounts[k]);
  }
  // the chunks
  const uint64_t R = P.n_reads;
  CHECK(P.sort_chunk_entries % 64 == 0 && P.sort_chunk_entries >= 64 && P.sort_chunks <= lgsn::kSnSortChunksMax);
  CHECK(P.sort_chunks == (R + P.sort_chunk_entries - 1) / P.sort_chunk_entries && P.scan_rows == lgsn::kSnScanRows && P.scan_chunks == (R + 63) / 64);
  // the arena: regions in order, 256 B starts, none overlapping, sized for what they hold
  const oneshot::Region* reg = reinterpret_cast<const oneshot::Region*>(&P.arena);
  const size_t n_reg = offsetof(lgsn::SnArena, bytes) / sizeof(oneshot::Region);
  for (size_t k = 0; k < n_reg; k++) CHECK(reg[k].at % 256 == 0 && reg[k].at + reg[k].bytes <= (k + 1 < n_reg ? reg[k + 1].at : P.arena.bytes));
  const lgsn::SnArena& A = P.arena;
  CHECK(A.mop_id.bytes == P.n_mops * 8 && A.mop_flags.bytes == P.n_mops && A.val.bytes == R * P.n_class * 8 && A.chk.bytes == R * P.n_words * 4);
  CHECK(A.skew_count.bytes == R * 4 && A.skew_first.bytes == R * 4 && A.skew_key.bytes == R * 8 && A.snap_flags.bytes >= R && A.snap_flags.bytes % 4 == 0);
  CHECK(A.hist.bytes == (size_t)P.sort_chunks * 1024 && A.off.bytes == 1024 && A.cmax.bytes == (size_t)P.scan_chunks * P.n_class * 8 && A.cmin.bytes == A.cmax.bytes);
  CHECK(A.image_bytes() == A.val.at && A.zero_bytes() == A.skew_first.at - A.val.at && A.ones_bytes() == A.summary.at - A.skew_first.at);
  const std::vector<unsigned char> img = lgsn::image(&in, P);
  CHECK(img.size() == A.image_bytes());
  CHECK(img.size() <= 25 * src.size() + 8 * (R + 1) + 12 * (size_t)in.n_accounts + 8 * 256);       // 25 bytes a read micro-op: c is not copied
  for (size_t m = 0; m < src.size(); m++) {
    int64_t v[3];
    std::memcpy(&v[0], img.data() + A.mop_id.at + m * 8, 8); std::memcpy(&v[1], img.data() + A.mop_a.at + m * 8, 8); std::memcpy(&v[2], img.data() + A.mop_b.at + m * 8, 8);
    CHECK(v[0] == in.mop_id[src[m]] && v[1] == in.mop_a[src[m]] && v[2] == in.mop_b[src[m]] && img[A.mop_flags.at + m] == in.mop_flags[src[m]]);
  }
  lgsn::SnAcc acc;
  std::memcpy(&acc, img.data() + A.acc.at, sizeof acc);
  CHECK(acc.first == lgsn::kSnNone && acc.worst == lgsn::kSnNone && acc.count == 0 && acc.n_candidates == 0 && acc.sum_counts == 0);
  std::vector<char> fake(16);
  const lgsn::SnArgs K = lgsn::args(&in, P, fake.data());
  CHECK((const char*)K.snap_flags == fake.data() + A.snap_flags.at && K.n_reads == P.n_reads && K.sort_chunks == P.sort_chunks && (const char*)K.row_cum == fake.data() + A.row_cum.at);
  // ---- the kernels, under the emulator and the sanitizers, against the rules restated pair by pair
  std::vector<std::map<uint32_t, int64_t>> vec(R);
  uint64_t n_checked = 0;
  {
    size_t r = 0;
    for (uint32_t i = 0; i < in.n_ops; i++) {
      if (in.type[i] != TBC_LEDGER_T_OK || in.kind[i] != TBC_LEDGER_K_READ) continue;
      for (uint64_t m = in.mop_off[i]; m < in.mop_off[i + 1]; m++)
        for (uint32_t k = 0; k < in.n_accounts; k++)
          if (!(in.mop_flags[m] & TBC_LEDGER_M_NIL) && in.accounts[k] == in.mop_id[m]) { vec[r][2 * k] = in.mop_a[m]; vec[r][2 * k + 1] = in.mop_b[m]; n_checked++; }
      r++;
    }
  }
  const auto below = [&](size_t x, size_t y) {                                // the least counter on which x is below y
    for (const auto& kv : vec[x]) { const auto it = vec[y].find(kv.first); if (it != vec[y].end() && kv.second < it->second) return kv.first; }
    return lgsn::kSnNone;
  };
  std::vector<uint32_t> count(R, 0), first(R, lgsn::kSnNone), key(2 * R, lgsn::kSnNone);
  std::vector<uint8_t> fl(R, 0), with_complete(R, 0);
  uint32_t n_partial = 0, n_cand = 0, n_skewed = 0;
  uint64_t sum = 0;
  for (size_t x = 0; x < R; x++) {
    for (size_t y = 0; y < R; y++) {
      if (x == y || below(x, y) == lgsn::kSnNone || below(y, x) == lgsn::kSnNone) continue;
      if (!count[x]++) { first[x] = (uint32_t)y; key[2 * x] = below(x, y); key[2 * x + 1] = below(y, x); }
      if (vec[y].size() == P.n_class) with_complete[x] = 1;
    }
    const bool partial = vec[x].size() != P.n_class;
    fl[x] = (uint8_t)((partial ? TBC_LEDGER_SNAP_PARTIAL : 0u) | (count[x] ? TBC_LEDGER_SNAP_SKEWED : 0u));
    n_partial += partial; n_cand += partial || with_complete[x]; n_skewed += count[x] != 0; sum += count[x];
  }
  std::vector<uint32_t> g_count(R + 1, 7), g_first(R + 1, 7), g_key(2 * R + 1, 7);
  std::vector<uint8_t> g_fl(R + 1, 7);
  tbc_ledger_snap_out out{};
  out.skew_count = g_count.data(); out.skew_first = g_first.data(); out.skew_key = g_key.data(); out.snap_flags = g_fl.data();
  CHECK(emu_snap_check(&in, &out, grid_cap, 1 + n_reg, sort_cap, scan_rows) == 0);
  g_count.resize(R); g_first.resize(R); g_key.resize(2 * R); g_fl.resize(R);
  CHECK(g_count == count && g_first == first && g_key == key && g_fl == fl);
  const tbc_ledger_snap_summary& s = out.summary;
  CHECK(s.read_count == R && s.n_partial == n_partial && s.valid == (n_skewed == 0) && s.bad_values == 0 && s.n_candidates == n_cand);
  CHECK(s.n_checked == n_checked && s.n_pairs == sum / 2 && s.skewed.count == n_skewed && s.bytes_in == img.size());
}

// ---- the launches: the two sequences over the recorder (they read the plan's numbers alone, so the arguments are made directly)
lgsn::SnArgs shape(uint32_t reads, uint32_t n_class, uint32_t sort_chunks, uint32_t scan_chunks) {
  lgsn::SnArgs A{};
  A.n_reads = reads; A.n_class = n_class; A.sort_chunks = sort_chunks; A.scan_chunks = scan_chunks;
  return A;
}

void launches() {
  using R = emu::Recorder;
  const R::Kernel layout = R::of(sn_layout_kernel), hist = R::of(sn_hist_kernel), carry = R::of(sn_carry_kernel), scatter = R::of(sn_scatter_kernel),
                  extremes = R::of(sn_extremes_kernel), scan_carry = R::of(sn_scan_carry_kernel), flag = R::of(sn_flag_kernel), compact = R::of(sn_compact_kernel),
                  pair = R::of(sn_pair_kernel), keys = R::of(sn_keys_kernel), count = R::of(sn_count_kernel), worst = R::of(sn_worst_kernel), summary = R::of(sn_summary_kernel);
  const auto filter = [](const lgsn::SnArgs& A) { R go; lgsn::filter_sequence(go, A); return go; };
  const auto rest = [](const lgsn::SnArgs& A, uint32_t n_candidates) { R go; lgsn::rest_sequence(go, A, n_candidates); return go; };
  // the sort: eight passes of three kernels over `chunks` chunks
  const auto with_sort = [&](R::Launch first, uint32_t chunks, std::vector<R::Launch> then) {
    std::vector<R::Launch> all{first};
    for (int pass = 0; pass < 8; pass++) { all.push_back({hist, chunks, 64}); all.push_back({carry, 1, 256}); all.push_back({scatter, chunks, 64}); }
    all.insert(all.end(), then.begin(), then.end());
    return all;
  };
  // no reads: only the summary
  CHECK(filter(shape(0, 6, 0, 0)).is({}));
  CHECK(rest(shape(0, 6, 0, 0), 0).is({{summary, 1, 64}}));
  // no accounts: the layout only (it counts the partial reads); no sort, no scan, no candidate
  CHECK(filter(shape(10, 0, 1, 1)).is({{layout, 3, 256}}));
  CHECK(rest(shape(10, 0, 1, 1), 0).is({{keys, 1, 256}, {count, 1, 256}, {worst, 1, 256}, {summary, 1, 64}}));
  // reads and accounts: the whole filter; then no candidate -- no pair kernel --, and one candidate: a slice per tile of 64 reads
  CHECK(filter(shape(130, 4, 3, 3)).is(with_sort({layout, 33, 256}, 3, {{extremes, 1, 256}, {scan_carry, 4, 256}, {flag, 1, 256}, {compact, 1, 256}})));
  CHECK(rest(shape(130, 4, 3, 3), 0).is({{keys, 1, 256}, {count, 1, 256}, {worst, 1, 256}, {summary, 1, 64}}));
  CHECK(rest(shape(130, 4, 3, 3), 1).is({{pair, 3, 256}, {keys, 1, 256}, {count, 1, 256}, {worst, 1, 256}, {summary, 1, 64}}));
  // one past each cap: 16,385 x 256 reads (the layout's 4,096 workgroups of four reads too), 4,097 counters, chunks x counters past
  // 16,384 x 256; the sort's chunks are the plan's 256 at most
  const lgsn::SnArgs big = shape(16385u * 256u, 4097, 256, 65540);
  CHECK(filter(big).is(with_sort({layout, 4096, 256}, 256, {{extremes, 16384, 256}, {scan_carry, 4096, 256}, {flag, 16384, 256}, {compact, 16384, 256}})));
  // ... the pairs: 4 blocks of candidates x 512 slices = 2,048 workgroups; 2,049 blocks and more take one slice each
  CHECK(rest(big, 1000).is({{pair, 2048, 256}, {keys, 16384, 256}, {count, 16384, 256}, {worst, 16384, 256}, {summary, 1, 64}}));
  CHECK(rest(big, 2049u * 256u).is({{pair, 2049, 256}, {keys, 16384, 256}, {count, 16384, 256}, {worst, 16384, 256}, {summary, 1, 64}}));
}

void refuse(const tbc_ledger_in& in, const char* needle, bool by_plan = false) {
  std::string err;
  lgsn::Plan P;
  if (by_plan) CHECK(!lgsn::plan("tbc_ledger_snapshots", &in, P, err));
  else CHECK(!lgsn::validate("tbc_ledger_snapshots", &in, err));
  if (err.find(needle) == std::string::npos || err.find("tbc_ledger_snapshots") != 0) { std::printf("FAILED: message '%s' lacks '%s'\n", err.c_str(), needle); std::exit(1); }
}

}  // namespace

int main() {
  int planned = 0;
  for (uint32_t n_ops : {0u, 1u, 2u, 17u, 200u, 700u})
    for (uint32_t n_acc : {0u, 1u, 3u, 20u})
      for (uint32_t knobs : {0u, 1u}) {
        rng_state = 91 + n_ops * 31 + n_acc * 7 + knobs;
        look(make(n_ops, n_acc), knobs ? 2u : 3u, knobs ? 1u + n_acc % 2u : 0u, knobs ? 1u : 0u);
        planned++;
      }
  // ---- the plan reads no micro-op: the columns are not there
  {
    Ledger L = make(300, 4);
    tbc_ledger_in s = L.in();
    s.mop_id = s.mop_a = s.mop_b = s.mop_c = reinterpret_cast<const int64_t*>(8);      // (never dereferenced)
    s.mop_flags = reinterpret_cast<const uint8_t*>(8);
    std::string err;
    lgsn::Plan P;
    CHECK(lgsn::plan("plan", &s, P, err) && P.n_mops > 0 && P.n_reads > 0);
    planned++;
  }
  // ---- every rule of tbc_ledger_in, broken in turn: checked under this entry point's name
  int refusals = 0;
  Ledger L;
  L.accounts = {3, 6, 9};
  for (int i = 0; i < 4; i++) { L.op(TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_TRANSFER); L.mop(100 + i, 3, 6); L.end(); L.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_TRANSFER); L.end(); }
  L.op(TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_READ); L.end();
  L.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_READ); L.mop(3, 1, 1); L.mop(6, 1, 1); L.mop(9, 1, 1); L.end();
  look(L, 1, 0, 0);
  { tbc_ledger_in s = L.in(); s.mop_off = nullptr; refuse(s, "null argument"); refusals++; }
  { tbc_ledger_in s = L.in(); s.accounts = nullptr; refuse(s, "null argument (accounts)"); refusals++; }
  { tbc_ledger_in s = L.in(); s.negative_balances = 2; refuse(s, "negative_balances is 0 or 1"); refusals++; }
  { Ledger M = L; M.index[4] = M.index[3]; refuse(M.in(), "op 4 (index"); refuse(M.in(), "strictly ascending"); refusals++; }
  { Ledger M = L; M.type[1] = 4; refuse(M.in(), "type is not"); refusals++; }
  { Ledger M = L; M.kind[1] = 4; refuse(M.in(), "kind is not"); refusals++; }
  { Ledger M = L; M.accounts = {3, 6, 3}; refuse(M.in(), "account 3 is listed twice"); refusals++; }
  { Ledger M = L; M.id[5] = M.id[4]; refuse(M.in(), "names an id twice"); refusals++; }
  { Ledger M = L; M.mop_flags[5] = 2; refuse(M.in(), "unknown micro-op flags"); refusals++; }
  // ---- the plan's own refusals: reads x counters of 2^31 (the dense rows are indexed in 32 bits' reach), 2^31 micro-ops of reads
  for (const uint32_t reads : {32767u, 32768u}) {
    Ledger M;
    for (uint32_t k = 0; k < 32768u; k++) M.accounts.push_back(k);
    for (uint32_t i = 0; i < reads; i++) { M.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_READ); M.end(); }
    const tbc_ledger_in s = M.in();
    std::string err;
    lgsn::Plan P;
    if (reads == 32767u) { CHECK(lgsn::plan("x", &s, P, err) && P.arena.val.bytes == (size_t)32767 * 65536 * 8); continue; }
    refuse(s, "reads x counters (32768 x 65536) is 2^31 or more", true); refusals++;
  }
  for (const uint64_t n : {(1ull << 31) - 1ull, 1ull << 31}) {
    Ledger M;
    M.accounts = {3};
    M.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_READ); M.end();
    M.mop_off[1] = n;
    tbc_ledger_in s = M.in();
    s.mop_id = s.mop_a = s.mop_b = s.mop_c = reinterpret_cast<const int64_t*>(8);      // (never dereferenced)
    s.mop_flags = reinterpret_cast<const uint8_t*>(8);
    std::string err;
    lgsn::Plan P;
    if (n < (1ull << 31)) { CHECK(lgsn::plan("x", &s, P, err) && P.n_mops == n); continue; }
    refuse(s, "2^31 or more micro-ops of reads in one call", true); refusals++;
  }
  // ---- a cap on the sort's chunks makes them longer, never fewer entries than there are reads
  {
    Ledger B;
    B.accounts = {1};
    for (uint32_t i = 0; i < 40000u; i++) { B.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_READ); B.end(); }
    const tbc_ledger_in s = B.in();
    std::string err;
    lgsn::Plan P;
    CHECK(lgsn::plan("plan", &s, P, err) && P.sort_chunk_entries == 192 && P.sort_chunks == 209 && P.scan_chunks == 625);
    CHECK(lgsn::plan("plan", &s, P, err, 2, 1) && P.sort_chunks == 2 && P.sort_chunk_entries == 20032 && P.scan_chunks == 40000);
  }
  launches();
  std::printf("%d ledgers planned, run and checked, %d refusals, the launches of 4 shapes\n", planned + 1, refusals);
  return 0;
}
