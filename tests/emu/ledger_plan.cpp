// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  ledger_plan.cpp: the host side of tbc_ledger_check without a device -- the validation and
// the plan of csrc/ledger_plan.h (the very functions ledger_host.hip runs every call through) in a program of its own, the one to build
// with -fsanitize=address,undefined (tests/test_ledger_columns.py does):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include -I tests/emu -I jepsen-tigerbeetle_amd/csrc tests/emu/ledger_plan.cpp -o ledger_plan && ./ledger_plan
// It builds ledgers of many shapes (seeded), plans them and checks what can be checked without Python: the row tables against a plain
// walk of the ops, the runs, the transfer ids, the arena's regions; then it breaks each rule of tbc_ledger_in in turn and looks at
// the message.  The columns are exactly as long as the struct says, so a read past an end is the sanitizer's to see.  And because it
// includes the emulator program of the kernels (emu_ledger.cpp), it holds lg::sequence -- the launches the library makes -- to the list
// of (kernel, grid, threads) written out below by hand, under the device's caps, on the edge shapes; and it runs lg::steps -- the
// steps the library takes -- over the emulator's call frame into output arrays of exactly the size the header states, and sees that
// the frame's own checks fire: a get longer than its region, a fill past the arena, a byte written behind it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "emu_ledger.cpp"

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
    s.accounts = accounts.data(); s.n_accounts = (uint32_t)accounts.size(); s.negative_balances = 0; s.total_amount = 100;
    return s;
  }
  void op(uint8_t t, uint8_t k, uint8_t f, const std::vector<int64_t>& ids) {
    index.push_back(index.empty() ? 3u : index.back() + 1u + (uint32_t)(ids.size() % 3));
    type.push_back(t); kind.push_back(k); flags.push_back(f);
    for (int64_t v : ids) { id.push_back(v); a.push_back(v * 2); b.push_back(v); c.push_back(1); mop_flags.push_back((uint8_t)(v % 11 == 0)); }
    mop_off.push_back(id.size());
  }
};

uint64_t rng_state = 1;
uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

Ledger make(uint32_t n_ops, uint32_t n_accounts, uint32_t long_read) {
  Ledger L;
  for (uint32_t k = 0; k < n_accounts; k++) L.accounts.push_back((int64_t)(n_accounts - k) * 5);          // (unsorted)
  int64_t next = 1;
  for (uint32_t i = 0; i < n_ops; i++) {
    const uint8_t t = (uint8_t)rnd(4), k = (uint8_t)rnd(4), f = (uint8_t)(rnd(3) == 0);
    std::vector<int64_t> ids;
    uint32_t n = k == TBC_LEDGER_K_READ ? rnd(12) : k == TBC_LEDGER_K_LOOKUP ? rnd(40) : k == TBC_LEDGER_K_TRANSFER ? 1 + rnd(2) : 0;
    if (k == TBC_LEDGER_K_READ && long_read && i == n_ops / 2) n = long_read;
    for (uint32_t m = 0; m < n; m++) ids.push_back(k == TBC_LEDGER_K_READ ? (int64_t)(n - m) * 5 : k == TBC_LEDGER_K_TRANSFER ? (rnd(4) ? next++ : 1) : (int64_t)rnd(50));
    L.op(t, k, f, ids);
  }
  return L;
}

void look(const Ledger& L) {
  const tbc_ledger_in in = L.in();
  std::string err;
  CHECK(lg::validate("plan", &in, err));
  lg::Plan P;
  CHECK(lg::plan("plan", &in, P, err));
  // the row tables against a plain walk
  uint32_t r = 0, fr = 0, fl = 0;
  std::set<int64_t> T;
  for (uint32_t i = 0; i < in.n_ops; i++) {
    const uint64_t lo = in.mop_off[i], n = in.mop_off[i + 1] - lo;
    const bool ok = in.type[i] == TBC_LEDGER_T_OK, fin = in.flags[i] & TBC_LEDGER_F_FINAL;
    if (in.type[i] == TBC_LEDGER_T_INVOKE && in.kind[i] == TBC_LEDGER_K_TRANSFER) for (uint64_t m = lo; m < lo + n; m++) T.insert(in.mop_id[m]);
    if (ok && in.kind[i] == TBC_LEDGER_K_READ) {
      CHECK(P.read_lo[r] == lo && P.read_cum[r + 1] - P.read_cum[r] == n); r++;
      if (fin) { CHECK(P.fr_lo[fr] == lo && P.fr_cum[fr + 1] - P.fr_cum[fr] == n); fr++; }
    }
    if (ok && in.kind[i] == TBC_LEDGER_K_LOOKUP && fin) { CHECK(P.fl_lo[fl] == lo && P.fl_cum[fl + 1] - P.fl_cum[fl] == n); fl++; }
  }
  CHECK(r == P.n_reads && fr == P.n_final_reads && fl == P.n_final_lookups && P.read_cum.size() == r + 1u);
  CHECK(std::set<int64_t>(P.transfer.begin(), P.transfer.end()) == T && P.transfer.size() == T.size() && P.n_transfers == T.size());
  CHECK(P.tab_slots == 0 ? T.empty() : (P.tab_slots >= 2 * T.size() && (P.tab_slots & (P.tab_slots - 1)) == 0 && P.tab_mask == P.tab_slots - 1));
  // the runs cover the reads in order; a run of several reads stays within a step, and no run has more reads than LDS words
  CHECK(P.run_first.size() == P.n_runs + 1u && P.run_first[0] == 0 && P.run_first[P.n_runs] == P.n_reads);
  for (uint32_t k = 0; k < P.n_runs; k++) {
    const uint32_t a = P.run_first[k], b = P.run_first[k + 1];
    CHECK(b > a && b - a <= lg::kLgRunReads);
    if (b - a > 1) CHECK(P.read_cum[b] - P.read_cum[a] <= lg::kLgRunMops);
    if (b < P.n_reads && b - a < lg::kLgRunReads) CHECK(P.read_cum[b + 1] - P.read_cum[a] > lg::kLgRunMops);     // (it could not have taken one more)
  }
  for (size_t k = 1; k < P.accounts.size(); k++) CHECK(P.accounts[k - 1] < P.accounts[k]);
  // the arena: regions in order, 256 B starts, none overlapping, sized for what they hold
  const oneshot::Region* reg = reinterpret_cast<const oneshot::Region*>(&P.arena);
  const size_t n_reg = offsetof(lg::LgArena, bytes) / sizeof(oneshot::Region);
  for (size_t k = 0; k < n_reg; k++) CHECK(reg[k].at % 256 == 0 && reg[k].at + reg[k].bytes <= (k + 1 < n_reg ? reg[k + 1].at : P.arena.bytes));
  CHECK(P.arena.mop_id.bytes == P.n_mops * 8 && P.arena.mop_flags.bytes == P.n_mops && P.arena.slots.bytes == P.tab_slots * 16);
  CHECK(P.arena.fr_unlike.bytes % 4 == 0 && P.arena.fr_unlike.bytes >= P.n_final_reads && P.arena.fl_unlike.bytes % 4 == 0 && P.arena.fl_unlike.bytes >= P.n_final_lookups);
  CHECK(P.arena.zero_bytes() == P.arena.read_error.at - P.arena.slots.at && P.arena.head_bytes() == P.arena.mop_id.at);
  const std::vector<unsigned char> img = lg::head_image(P);
  CHECK(img.size() == P.arena.head_bytes());
  lg::LgAcc acc;
  std::memcpy(&acc, img.data() + P.arena.acc.at, sizeof acc);
  CHECK(acc.first[3] == 0xFFFFFFFFu && acc.lowest_key == ~0ull && acc.highest_key == 0 && acc.count[1] == 0);
  if (P.n_reads) CHECK(std::memcmp(img.data() + P.arena.read_lo.at, P.read_lo.data(), P.n_reads * 8) == 0);
}

// ---- the launches: lg::sequence over the recorder (it reads the plan's numbers alone, so the arguments are made directly)
lg::LgArgs shape(uint32_t reads, uint32_t runs, uint32_t transfers, uint32_t final_reads, uint32_t final_lookups) {
  lg::LgArgs A{};
  A.n_reads = reads; A.n_runs = runs; A.n_transfers = transfers; A.n_final_reads = final_reads; A.n_final_lookups = final_lookups;
  return A;
}

void launches() {
  using R = emu::Recorder;
  const R::Kernel si = R::of(lg_si_kernel), build = R::of(lg_table_build_kernel), lookup = R::of(lg_lookup_kernel<EMU_W>), rows = R::of(lg_rows_equal_kernel),
                  finish = R::of(lg_finish_kernel), summary = R::of(lg_summary_kernel);
  const auto record = [](const lg::LgArgs& A, uint64_t fr_mops, uint64_t fl_mops) { R go; lg::sequence<EMU_W>(go, A, fr_mops, fl_mops); return go; };
  // no ops: only the summary
  CHECK(record(shape(0, 0, 0, 0, 0), 0, 0).is({{summary, 1, 64}}));
  // reads and nothing else; invoked transfers and nothing else (the table is built, nobody looks anything up)
  CHECK(record(shape(5, 2, 0, 0, 0), 0, 0).is({{si, 2, 256}, {finish, 1, 256}, {summary, 1, 64}}));
  CHECK(record(shape(0, 0, 300, 0, 0), 0, 0).is({{build, 2, 256}, {summary, 1, 64}}));
  // fewer than two final rows of either kind: no comparison; one final lookup is still looked up
  CHECK(record(shape(1, 1, 300, 1, 1), 8, 300).is({{si, 1, 256}, {build, 2, 256}, {lookup, 1, 256}, {finish, 1, 256}, {summary, 1, 64}}));
  // two final rows of each kind, the reads' without a micro-op (one workgroup all the same); no invoked transfer: no lookup kernel
  CHECK(record(shape(2, 1, 0, 2, 2), 0, 600).is({{si, 1, 256}, {rows, 1, 256}, {rows, 3, 256}, {finish, 1, 256}, {summary, 1, 64}}));
  // one past each cap: 16,385 runs, 4,097 final lookups, 8,193 x 256 - 255 micro-ops of final lookups; 8,192 x 256 of final reads are at it
  CHECK(record(shape(20000, 16385, 70000, 2, 4097), 8192ull * 256, 8192ull * 256 + 1).is(
      {{si, 16384, 256}, {build, 274, 256}, {lookup, 4096, 256}, {rows, 8192, 256}, {rows, 8192, 256}, {finish, 79, 256}, {summary, 1, 64}}));
}

// ---- the call frame: lg::steps into exact arrays, then each of the frame's checks broken in turn
void frame(const Ledger& L) {
  const tbc_ledger_in in = L.in();
  uint64_t n[6];
  CHECK(emu_lg_shape(&in, n) == 0);
  std::vector<uint8_t> read_error(n[0]), fr_unlike(n[2]), fl_unlike(n[3]);
  std::vector<int64_t> read_total(n[0]), read_badness(n[0]);
  std::vector<uint32_t> missing(n[3]);
  tbc_ledger_out out{};
  out.read_error = read_error.data(); out.read_total = read_total.data(); out.read_badness = read_badness.data();
  out.lookup_missing = missing.data(); out.final_read_unlike = fr_unlike.data(); out.final_lookup_unlike = fl_unlike.data();
  CHECK(emu_lg_check(&in, &out, 2, 1) == 0);
  CHECK(out.summary.ns_device == 0 && out.summary.bytes_in >= 33 * in.mop_off[in.n_ops]);
  std::string err;
  const oneshot::Region r{256, 64};
  unsigned char buf[128];
  { emu::Arena C(err); C.open(0, 1024); CHECK(C.get(buf, r, 64) == TBC_OK && C.get(nullptr, r, 64) == TBC_OK && C.close() == TBC_OK && err.empty()); }
  { emu::Arena C(err); C.open(0, 1024); CHECK(C.get(buf, r, 65) == TBC_ERR_HIP && err.find("a get of 65 bytes") != std::string::npos && C.put(r, buf) == TBC_ERR_HIP && C.close() == TBC_ERR_HIP); }
  { emu::Arena C(err); C.open(0, 1024); CHECK(C.fill(r, 0, 768) == TBC_OK && C.fill(r, 0, 769) == TBC_ERR_HIP && err.find("a fill of 769 bytes") != std::string::npos && (unsigned char)C.base()[1024] == 0xA5); }
  { emu::Arena C(err); C.open(0, 1024); CHECK(C.put(oneshot::Region{1024, 1}, buf) == TBC_ERR_HIP && err.find("a put of 1 bytes at 1024") != std::string::npos && C.bytes_in == 0); }
  { emu::Arena C(err); C.open(0, 1024); C.base()[1024 + 7] = 0; CHECK(C.status == TBC_OK && C.close() == TBC_ERR_HIP && err.find("byte 7 behind the arena") != std::string::npos); }
  { emu::Arena C(err); C.open(0, 1024); C.more(40)[40] = 0; CHECK(C.close() == TBC_ERR_HIP && err.find("byte 0 behind the second allocation") != std::string::npos); }
}

void refuse(tbc_ledger_in in, const char* needle) {
  std::string err;
  CHECK(!lg::validate("tbc_ledger_check", &in, err));
  if (err.find(needle) == std::string::npos || err.find("tbc_ledger_check") != 0) { std::printf("FAILED: message '%s' lacks '%s'\n", err.c_str(), needle); std::exit(1); }
}

}  // namespace

int main() {
  int planned = 0;
  for (uint32_t n_ops : {0u, 1u, 2u, 17u, 300u, 3000u})
    for (uint32_t n_acc : {0u, 1u, 8u, 70u})
      for (uint32_t long_read : {0u, 257u, 700u}) { rng_state = 77 + n_ops * 31 + n_acc * 7 + long_read; look(make(n_ops, n_acc, long_read)); planned++; }
  // ---- every rule, broken in turn (op 5 of a small valid ledger: an :ok read of ids 15 10 5)
  Ledger L;
  L.accounts = {5, 10, 15};
  for (int i = 0; i < 5; i++) L.op(TBC_LEDGER_T_INVOKE, TBC_LEDGER_K_TRANSFER, 0, {100 + i});
  L.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_READ, TBC_LEDGER_F_FINAL, {15, 10, 5});
  L.op(TBC_LEDGER_T_OK, TBC_LEDGER_K_LOOKUP, TBC_LEDGER_F_FINAL, {100, 101, 101});
  look(L);
  frame(L);
  rng_state = 9; frame(make(300, 8, 257));
  { tbc_ledger_in s = L.in(); s.mop_off = nullptr; refuse(s, "null argument"); }
  { tbc_ledger_in s = L.in(); s.kind = nullptr; refuse(s, "null argument"); }
  { tbc_ledger_in s = L.in(); s.mop_b = nullptr; refuse(s, "null argument"); }
  { tbc_ledger_in s = L.in(); s.accounts = nullptr; refuse(s, "null argument"); }
  { tbc_ledger_in s = L.in(); s.negative_balances = 2; refuse(s, "negative_balances"); }
  { Ledger M = L; M.mop_off[0] = 1; refuse(M.in(), "mop_off[0] must be 0"); }
  { Ledger M = L; M.mop_off[3] = M.mop_off[2] - 1; refuse(M.in(), "op 2 (index"); }
  { Ledger M = L; M.index[4] = M.index[3]; refuse(M.in(), "op 4 (index"); refuse(M.in(), "strictly ascending"); }
  { Ledger M = L; M.index[6] = 0xFFFFFFFFu; refuse(M.in(), "TBC_NO_OP"); }
  { Ledger M = L; M.type[1] = 4; refuse(M.in(), "type is not"); }
  { Ledger M = L; M.kind[1] = 4; refuse(M.in(), "kind is not"); }
  { Ledger M = L; M.flags[1] = 2; refuse(M.in(), "unknown op flags"); }
  { Ledger M = L; M.mop_flags[5] = 2; refuse(M.in(), "unknown micro-op flags"); }
  { Ledger M = L; M.accounts = {5, 10, 5}; refuse(M.in(), "account 5 is listed twice"); }
  { Ledger M = L; M.id[7] = 15; refuse(M.in(), "op 5 (index"); refuse(M.in(), "names an id twice"); }
  launches();
  std::printf("%d ledgers planned and checked, 16 refusals, the launches of 6 shapes\n", planned + 1);
  return 0;
}
