// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  setfull_plan.cpp: the planner of a set-full object (csrc/set_full_plan.h, sf_make_layout: the
// very function set_full_host.hip builds an object from) behind a few C functions.  Built as a shared object by
// tests/test_set_full_plan.py, which looks at what the planner returns.  The planner is plain host code, so no emulator header is needed.
//
// With -DSFP_MAIN the file is a program of its own that plans the same shapes and checks what can be checked without Python -- the one to
// build with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -DSFP_MAIN -I jepsen-tigerbeetle_amd/csrc tests/emu/setfull_plan.cpp -o setfull_plan && ./setfull_plan
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "set_full_plan.h"

namespace {
SfLayout g;
constexpr size_t kRegions = offsetof(SfArena, bytes) / sizeof(SfRegion);          // SfArena: its regions in order, then the total
static_assert(offsetof(SfArena, bytes) % sizeof(SfRegion) == 0 && sizeof(SfRegion) == 2 * sizeof(size_t), "SfArena is an array of regions and a total");
const SfRegion* regions(const SfLayout& L) { return reinterpret_cast<const SfRegion*>(&L.arena); }
}  // namespace

extern "C" uint32_t sfp_regions() { return (uint32_t)kRegions; }
extern "C" uint32_t sfp_sizeof_key_plan() { return (uint32_t)sizeof(SfKeyPlan); }

// source: 0 Dense, 1 Rows, 2 Ops.  Returns fits()
extern "C" int sfp_make(uint32_t n_keys, const uint32_t* E, const uint32_t* R, uint32_t source, uint32_t words_per_row, uint64_t n_exceptions) {
  g = sf_make_layout(n_keys, E, R, (SfSource)source, words_per_row, n_exceptions);
  return g.fits() ? 1 : 0;
}

// plan [n_keys], first [kFirsts][n_keys + 1], tiles [kFirsts], the regions' starts and sizes [sfp_regions()], enc (tab_off, mask per key; Ops), and
// totals: arena bytes, head_bytes, enc_zero_bytes, m_words, sum_words, pmax_words, tab_slots, bytes_matrix, sumE, sumR, enc_keys
extern "C" void sfp_get(void* plan, uint32_t* first, uint64_t* tiles, uint64_t* at, uint64_t* bytes, uint64_t* enc, uint64_t* totals) {
  std::memcpy(plan, g.plan.data(), g.plan.size() * sizeof(SfKeyPlan));
  std::memcpy(first, g.first.data(), g.first.size() * 4);
  for (int i = 0; i < kFirsts; i++) tiles[i] = g.tiles[i];
  for (size_t i = 0; i < kRegions; i++) { at[i] = regions(g)[i].at; bytes[i] = regions(g)[i].bytes; }
  for (size_t k = 0; k < g.enc_keys.size(); k++) { enc[2 * k] = g.enc_keys[k].tab_off; enc[2 * k + 1] = g.enc_keys[k].mask; }
  const uint64_t t[] = {g.arena.bytes, g.arena.head_bytes(), g.arena.enc_zero_bytes(), g.m_words, g.sum_words, g.pmax_words, g.tab_slots, g.bytes_matrix,
                        g.sumE, g.sumR, g.enc_keys.size()};
  std::memcpy(totals, t, sizeof t);
}

#ifdef SFP_MAIN
#include <cstdio>
#include <cstdlib>
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)
int main() {
  // tests/test_set_full_plan.py's two objects under every source, then its single keys (tests/test_set_full_timing.py's shapes)
  const uint32_t E1[] = {129}, R1[] = {130}, E4[] = {33, 0, 4100, 1024}, R4[] = {130, 5, 0, 2049};
  const uint32_t shapes[][2] = {{33, 130}, {33, 2049}, {33, 5000}, {129, 130}, {129, 2049}, {129, 5000}, {4100, 130}, {4100, 2049}, {4100, 5000},
                                {33000, 130}, {33000, 5000}, {64, 2048 * 4 + 100}, {64, 2048 * 256 + 100}, {96, 256 * 130}, {0, 130}, {129, 0}, {0, 0}};
  int planned = 0;
  const auto look = [&](const SfLayout& L) {
    const uint32_t n = L.n_keys;
    CHECK(L.fits() && L.plan.size() == n && L.first.size() == (size_t)kFirsts * (n + 1));
    const SfRegion* r = regions(L);
    for (size_t i = 0; i < kRegions; i++) CHECK(r[i].at % 256 == 0 && r[i].at + r[i].bytes <= (i + 1 < kRegions ? r[i + 1].at : L.arena.bytes));
    for (uint32_t k = 0; k < n; k++) CHECK(L.plan[k].m_off % 64 == 0 && L.plan[k].sum_off % 64 == 0 && L.plan[k].PITCH % 4 == 0);
    for (int gi = 0; gi < kFirsts; gi++) {
      const uint32_t* f = L.first.data() + (size_t)gi * (n + 1);
      for (uint32_t k = 0; k < n; k++) CHECK(f[k] <= f[k + 1]);
      CHECK(f[n] == L.tiles[gi]);
    }
    CHECK(L.tiles[kFirstRows] == L.sumR);
    planned++;
  };
  for (int s = 0; s < 3; s++) {
    look(sf_make_layout(1, E1, R1, (SfSource)s, s == 0 ? 5u : 0u, s == 1 ? 7u : 0u));
    look(sf_make_layout(4, E4, R4, (SfSource)s, s == 0 ? 130u : 0u, s == 1 ? 7u : 0u));
  }
  for (const auto& sh : shapes) look(sf_make_layout(1, &sh[0], &sh[1], SfSource::Rows, 0u, 0u));
  std::printf("%d layouts planned and checked\n", planned);
  return 0;
}
#endif
