// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  perf_plan.cpp: the host side of tbc_perf_series without a device -- the validation and the
// plan of csrc/perf_plan.h (the very functions perf_host.hip runs every call through) in a program of its own, the one to build with
// -fsanitize=address,undefined (tests/test_perf_host.py does):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include -I tests/emu -I jepsen-tigerbeetle_amd/csrc tests/emu/perf_plan.cpp -o perf_plan && ./perf_plan
// It builds histories of many shapes (seeded), plans them and checks what can be checked without Python: the partner column against a
// plain quadratic pairing, t_max / nb_all / n_plot at the bucket edges, the chunks, the arena's regions; then it breaks each rule of
// tbc_perf_in in turn and looks at the status and the message.  The columns are exactly as long as the struct says, so a read past an
// end is the sanitizer's to see.  And because it includes the emulator program of the kernels (emu_perf.cpp), it holds pf::sequence --
// the launches the library makes -- to the list of (kernel, grid, threads) written out below by hand, under the device's caps, on the
// edge shapes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>
#include "emu_perf.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

namespace {

struct History {
  std::vector<int64_t> time;
  std::vector<int32_t> process;
  std::vector<uint8_t> type, flags;
  std::vector<uint16_t> f;
  uint32_t n_f = 0;
  tbc_perf_in in() const {
    tbc_perf_in s{};
    s.n_ops = (uint32_t)time.size(); s.time = time.data(); s.process = process.data(); s.type = type.data(); s.flags = flags.data(); s.f = f.data();
    s.n_f = n_f;
    return s;
  }
  void op(int64_t t, int32_t p, uint8_t ty, uint16_t fi) {
    time.push_back(t); process.push_back(p); type.push_back(ty); flags.push_back(p == TBC_PERF_NO_PROCESS ? 0 : TBC_PERF_F_CLIENT); f.push_back(fi);
    if (p != TBC_PERF_NO_PROCESS && fi >= n_f) n_f = fi + 1u;
  }
};

uint64_t rng_state = 1;
uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

History make(uint32_t n_ops, uint32_t n_procs, uint32_t n_f, int64_t gap) {
  History H;
  int64_t t = 0;
  for (uint32_t i = 0; i < n_ops; i++) {
    t += 1 + rnd((uint32_t)gap);
    if (rnd(20) == 0) { H.op(t, TBC_PERF_NO_PROCESS, TBC_PERF_T_INFO, 0); continue; }
    // (invocations and completions at random: second invocations and completions of nothing open both occur)
    H.op(rnd(4) ? t : t / 2, (int32_t)rnd(n_procs) - 2, (uint8_t)rnd(4), (uint16_t)rnd(n_f));
  }
  return H;
}

void look(const History& H) {
  const tbc_perf_in in = H.in();
  std::string err;
  CHECK(pf::validate("plan", &in, err) == TBC_OK);
  pf::Plan P;
  CHECK(pf::plan("plan", &in, P, err) == TBC_OK);
  const uint32_t n = in.n_ops;
  // pairing, stated again: an invocation's partner is its process's next client op if that is a completion
  std::vector<uint32_t> partner(n, pf::kPfNone);
  uint32_t matched = 0, client = 0;
  int64_t t_max = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (in.time[i] > t_max) t_max = in.time[i];
    if (!(in.flags[i] & TBC_PERF_F_CLIENT)) continue;
    client++;
    if (in.type[i] != TBC_PERF_T_INVOKE) continue;
    for (uint32_t j = i + 1; j < n; j++) {
      if (!(in.flags[j] & TBC_PERF_F_CLIENT) || in.process[j] != in.process[i]) continue;
      if (in.type[j] != TBC_PERF_T_INVOKE) { partner[i] = j; partner[j] = i; matched++; }
      break;
    }
  }
  CHECK(P.partner == partner && P.n_matched == matched && P.n_client == client && P.t_max == t_max);
  CHECK(P.nb_all == (uint32_t)(t_max / 1000000000ll) + 1u && (P.n_plot == P.nb_all || P.n_plot + 1u == P.nb_all));
  CHECK(P.n_cells == in.n_f * P.nb_all && P.n_class == in.n_f * 3u && P.n_scan_tiles == (P.n_cells + 255u) / 256u);
  // the chunks: whole wavefronts, covering the ops, their carried totals within bounds (or one chunk)
  CHECK(P.chunk_ops % 64u == 0u && P.chunk_ops >= 64u && (uint64_t)P.n_chunks * P.chunk_ops >= n && (P.n_chunks == 0 ? n == 0 : (uint64_t)(P.n_chunks - 1u) * P.chunk_ops < n));
  CHECK(P.n_chunks <= 1u || (uint64_t)P.n_chunks * P.n_class <= pf::kPfCarryWords);
  CHECK(P.n_chunks <= pf::kPfChunksMax);
  // the arena: regions in order, 256 B starts, none overlapping, sized for what they hold
  const oneshot::Region* reg = reinterpret_cast<const oneshot::Region*>(&P.arena);
  const size_t n_reg = offsetof(pf::PfArena, bytes) / sizeof(oneshot::Region);
  for (size_t k = 0; k < n_reg; k++) CHECK(reg[k].at % 256 == 0 && reg[k].at + reg[k].bytes <= (k + 1 < n_reg ? reg[k + 1].at : P.arena.bytes));
  const pf::PfArena& A = P.arena;
  CHECK(A.time.bytes == (size_t)n * 8 && A.partner.bytes == (size_t)n * 4 && A.f.bytes == (size_t)n * 2 && A.op_outcome.bytes == n);
  CHECK(A.q_value.bytes == (size_t)P.n_cells * 32 && A.lat_cell.bytes == (size_t)matched * 8 && A.open_word.bytes == (size_t)P.n_class * P.nb_all * 8);
  CHECK(A.open_fill.bytes == (size_t)P.n_class * P.n_plot * 4 && A.carry.bytes == (size_t)P.n_chunks * P.n_class * 4);
  CHECK(A.zero_bytes() == A.summary.at && A.acc.at == 0);
  tbc_perf_sizes z{};
  CHECK(pf::sizes("plan", &in, z, err) == TBC_OK && z.n_ops == n && z.n_f == in.n_f && z.nb_all == P.nb_all && z.n_plot == P.n_plot && z.t_max == t_max);
}

// ---- the launches: pf::sequence over the recorder (it reads the plan's numbers alone, so the arguments are made directly)
pf::PfArgs shape(uint32_t n_ops, uint32_t n_class, uint32_t n_chunks, uint32_t n_cells, uint32_t n_scan_tiles) {
  pf::PfArgs A{};
  A.n_ops = n_ops; A.n_class = n_class; A.n_chunks = n_chunks; A.n_cells = n_cells; A.n_scan_tiles = n_scan_tiles;
  return A;
}

void launches() {
  using R = emu::Recorder;
  const R::Kernel classify = R::of(pf_classify_kernel), totals = R::of(pf_open_totals_kernel), carry = R::of(pf_open_carry_kernel), scan = R::of(pf_open_scan_kernel),
                  cell_sum = R::of(pf_cell_sum_kernel), tile_scan = R::of(pf_tile_scan_kernel), offsets = R::of(pf_cell_offsets_kernel), gather = R::of(pf_gather_kernel),
                  select = R::of(pf_select_kernel), fill = R::of(pf_fill_kernel), summary = R::of(pf_summary_kernel);
  const auto record = [](const pf::PfArgs& A) { R go; pf::sequence(go, A); return go; };
  // no ops: only the summary
  CHECK(record(shape(0, 0, 0, 0, 0)).is({{summary, 1, 64}}));
  // ops but no f (no client op): no cells and no classes; the open scan still writes the zeros of op_open_after
  CHECK(record(shape(300, 0, 5, 0, 0)).is({{classify, 2, 256}, {scan, 5, 64}, {summary, 1, 64}}));
  // all of it: 300 ops of 2 f's over 3 seconds
  CHECK(record(shape(300, 6, 5, 6, 1)).is({{classify, 2, 256}, {totals, 5, 64}, {carry, 6, 256}, {scan, 5, 64}, {cell_sum, 1, 256}, {tile_scan, 1, 256},
                                           {offsets, 1, 256}, {gather, 2, 256}, {select, 6, 256}, {fill, 6, 64}, {summary, 1, 64}}));
  // one past each cap: 8,193 x 256 ops, 4,097 chunks, 16,385 classes, 16,385 cells, 8,193 tiles of cells
  CHECK(record(shape(8193u * 256u, 16385, 4097, 16385, 8193)).is(
      {{classify, 8192, 256}, {totals, 4096, 64}, {carry, 16384, 256}, {scan, 4096, 64}, {cell_sum, 8192, 256}, {tile_scan, 1, 256},
       {offsets, 8192, 256}, {gather, 8192, 256}, {select, 16384, 256}, {fill, 16384, 64}, {summary, 1, 64}}));
}

void refuse(const tbc_perf_in& in, tbc_status want, const char* needle) {
  std::string err;
  tbc_status st = pf::validate("tbc_perf_series", &in, err);
  if (st == TBC_OK) { pf::Plan P; st = pf::plan("tbc_perf_series", &in, P, err); }
  if (st != want || err.find(needle) == std::string::npos || err.find("tbc_perf_series") != 0) {
    std::printf("FAILED: status %d (want %d), message '%s' lacks '%s'\n", (int)st, (int)want, err.c_str(), needle);
    std::exit(1);
  }
}

}  // namespace

int main() {
  int planned = 0;
  for (uint32_t n_ops : {0u, 1u, 2u, 63u, 64u, 65u, 300u, 5000u})
    for (uint32_t n_procs : {3u, 40u})
      for (uint32_t n_f : {1u, 9u, 300u})
        for (int64_t gap : std::initializer_list<int64_t>{1000, 40000000}) { rng_state = 99 + n_ops * 31 + n_procs * 7 + n_f + (uint64_t)gap; look(make(n_ops, n_procs, n_f, gap)); planned++; }
  // ---- t_max on the bucket edges: both values of n_plot, and the integer bucket against the reference's long(double(t) / 1e9)
  const int64_t S = 1000000000ll;
  for (int64_t k : std::initializer_list<int64_t>{1, 3, 1000, 4503598})
    for (int64_t d : std::initializer_list<int64_t>{-1, 0, S / 2 - 1, S / 2, S / 2 + 1}) {
      const int64_t t = k * S + d;
      History H;
      H.op(5, 0, TBC_PERF_T_INVOKE, 0); H.op(t, TBC_PERF_NO_PROCESS, TBC_PERF_T_INFO, 0);
      const tbc_perf_in in = H.in();
      tbc_perf_sizes z{};
      std::string err;
      CHECK(pf::validate("plan", &in, err) == TBC_OK && pf::sizes("plan", &in, z, err) == TBC_OK);
      CHECK(z.t_max == t && z.nb_all == (uint32_t)(t / S) + 1u && (int64_t)((double)t / 1e9) == t / S);
      CHECK(z.n_plot == (d < 0 || d >= S / 2 ? z.nb_all : z.nb_all - 1u));   // (k S - 1 is in bucket k - 1, past its midpoint)
      planned++;
    }
  // ---- every rule, broken in turn
  History L;
  for (int i = 0; i < 6; i++) { L.op(1000 * i, i % 3, TBC_PERF_T_INVOKE, (uint16_t)(i % 2)); L.op(1000 * i + 500, i % 3, TBC_PERF_T_OK, (uint16_t)(i % 2)); }
  L.op(7000, TBC_PERF_NO_PROCESS, TBC_PERF_T_INFO, 0);
  look(L);
  { tbc_perf_in s = L.in(); s.time = nullptr; refuse(s, TBC_ERR_INVALID_ARG, "null argument"); }
  { tbc_perf_in s = L.in(); s.f = nullptr; refuse(s, TBC_ERR_INVALID_ARG, "null argument"); }
  { tbc_perf_in s = L.in(); s.n_f = 65537; refuse(s, TBC_ERR_INVALID_ARG, "n_f is at most"); }
  { History M = L; M.type[3] = 4; refuse(M.in(), TBC_ERR_INVALID_ARG, "op 3: type is not"); }
  { History M = L; M.flags[3] = 2; refuse(M.in(), TBC_ERR_INVALID_ARG, "op 3: unknown op flags"); }
  { History M = L; M.flags[12] = 1; refuse(M.in(), TBC_ERR_INVALID_ARG, "op 12: TBC_PERF_F_CLIENT"); }
  { History M = L; M.process[2] = TBC_PERF_NO_PROCESS; refuse(M.in(), TBC_ERR_INVALID_ARG, "op 2: TBC_PERF_F_CLIENT"); }
  { History M = L; M.f[5] = 2; refuse(M.in(), TBC_ERR_INVALID_ARG, "op 5: f is not below n_f"); }
  { History M = L; M.time[4] = INT64_MIN; refuse(M.in(), TBC_ERR_BAD_HISTORY, "op 4: the op has no :time"); }
  { History M = L; M.time[12] = -1; refuse(M.in(), TBC_ERR_BAD_HISTORY, "op 12: negative :time"); }
  { History M = L; M.time[1] = 1ll << 52; refuse(M.in(), TBC_ERR_BAD_HISTORY, "op 1: :time is 2^52 ns or more"); }
  { History M = L; M.time[1] = (1ll << 52) - 1; M.n_f = 200; refuse(M.in(), TBC_ERR_UNSUPPORTED, "2^31 cells or more"); }
  { History M = L; M.time[1] = (1ll << 52) - 1; M.n_f = 2; std::string err; tbc_perf_sizes z{}; const tbc_perf_in s = M.in();
    CHECK(pf::validate("p", &s, err) == TBC_OK && pf::sizes("p", &s, z, err) == TBC_OK && z.nb_all == 4503600u); }
  launches();
  std::printf("%d histories planned and checked, 12 refusals, the launches of 4 shapes\n", planned + 1);
  return 0;
}
