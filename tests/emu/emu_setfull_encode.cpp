// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_setfull_encode.cpp: tbc_setfull_keys_create_ops's encoding on the CPU -- the host plan of
// csrc/set_full_encode_plan.h, the layout of csrc/set_full_plan.h (sf_make_layout, as set_full_host.hip calls it for an object made from
// ops) and the kernels of csrc/set_full_encode.h (the very files hipcc compiles into libtbcheck.so) under the
// wavefront / workgroup emulator, in the library's order: plan, table build, values kernel, and the dups kernel if the repeat counter is
// not zero.  The window of the values kernel is EMU_W words here (the library's is TBC_SETFULL_ENCODE_WINDOW_WORDS), so that rows of a
// few hundred elements span several windows.  Built as a shared object by tests/test_set_full_encode_emu.py, which compares what it
// returns with jepsen/set_full.py `Encoded`.  The emulator headers have ballots and the workgroup barrier; the atomics the kernels use
// are stated here (between two rendezvous the emulator runs one lane at a time).
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "tbcheck.h"
#define TBC_EMU 1
#include "wave_env_emu.h"
#include "wave_env_wg_emu.h"

#define __global__
#define __launch_bounds__(...)
#define __forceinline__ inline
#define __shared__ static
#define __popcll(x) __builtin_popcountll(x)
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
static inline uint32_t atomicCAS(uint32_t* p, uint32_t expected, uint32_t desired) { const uint32_t o = *p; if (o == expected) *p = desired; return o; }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p |= v; return o; }
static inline uint32_t atomicAnd(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p &= v; return o; }
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v > o) *p = v; return o; }

#include "set_full_encode_plan.h"
#include "set_full_encode.h"

#ifndef EMU_W
#define EMU_W 8u
#endif

namespace {
struct Call { void (*k)(SfEncArgs); SfEncArgs A; };
void trampoline(void* arg, uint32_t) { Call* c = (Call*)arg; c->k(c->A); }
void launch(void (*k)(SfEncArgs), const SfEncArgs& A, uint32_t grid, uint64_t seed) {
  Call c{k, A};
  for (uint32_t b = 0; b < grid; b++) wv::run_workgroup(trampoline, &c, 4, b, seed + b);
}

struct State {
  sfenc::Plan P;
  std::vector<SfKeyPlan> plan;
  std::vector<uint32_t> M, dup_max, dup_count;
  std::vector<uint64_t> unknown;
  uint32_t repeats = 0, dups_ran = 0;
  std::string err;
} g;
}  // namespace

// 0: encoded; 1: refused (emu_sfe_error says why).  grid: the values kernel's workgroups (fewer than rows: the grid stride runs)
extern "C" int emu_sfe_encode(const tbc_setfull_ops_in* in, uint32_t grid, uint64_t seed) {
  g = State{};
  if (!sfenc::validate("emu_sfe_encode", in, g.err)) return 1;
  sfenc::plan(in, g.P);
  const sfenc::Plan& P = g.P;
  const uint32_t n = in->n_keys, sumE = (uint32_t)P.element.size(), sumR = (uint32_t)P.read_ok.size();
  // the library's own plan (csrc/set_full_plan.h): the plan table, the first rows, the keys' tables
  const SfLayout L = sf_make_layout(n, P.n_elements.data(), P.n_reads.data(), SfSource::Ops, 0u, 0u);
  g.plan = L.plan;
  const std::vector<uint32_t>& first = L.first;
  const std::vector<SfEncKey>& enc = L.enc_keys;
  g.M.assign(L.m_words + 4, 0xA5A5A5A5u);                     // (what the kernel does not write shows)
  std::vector<SfEncSlot> tab(L.tab_slots + 1, SfEncSlot{0, 0u, 0u});
  std::vector<uint8_t> row_flag(sumR + 1, 0);
  std::vector<uint32_t> key_flag(n, 0u), cnt(sumE + 1, 0u);
  g.dup_max.assign(sumE + 1, 0u); g.dup_count.assign(n, 0u); g.unknown.assign(n, 0ull);
  std::vector<unsigned long long> lo(P.val_lo.begin(), P.val_lo.end()), hi(P.val_hi.begin(), P.val_hi.end()), unk(n, 0ull);
  lo.push_back(0); hi.push_back(0);
  SfEncArgs A;
  A.plan = g.plan.data(); A.first = first.data(); A.enc = enc.data(); A.n_keys = n; A.R_all = sumR; A.E_all = sumE;
  A.grid = grid < 1u ? 1u : (grid < sumR ? grid : (sumR ? sumR : 1u));
  A.element = (const long long*)P.element.data(); A.slots = tab.data(); A.vals = (const long long*)in->vals;
  A.val_lo = lo.data(); A.val_hi = hi.data(); A.M = g.M.data(); A.row_flag = row_flag.data(); A.key_flag = key_flag.data();
  A.unknown = unk.data(); A.repeats = &g.repeats; A.cnt = cnt.data(); A.dup_max = g.dup_max.data(); A.dup_count = g.dup_count.data();
  if (sumE) launch(sf_table_build_kernel, A, (sumE + 255u) / 256u, seed);
  if (sumR) launch(sf_values_kernel<EMU_W>, A, A.grid, seed + 1000);
  if (g.repeats) { launch(sf_dups_kernel, A, n, seed + 2000); g.dups_ran = 1; }
  for (uint32_t k = 0; k < n; k++) g.unknown[k] = unk[k];
  for (uint32_t e = 0; e < sumE; e++) if (cnt[e]) { g.err = "cnt scratch not left zeroed"; return 1; }
  // every element sits in its key's table exactly once, and a table is at most half full
  for (uint32_t k = 0; k < n; k++) {
    uint32_t used = 0;
    for (uint64_t s = 0; g.plan[k].E && s <= enc[k].mask; s++) used += tab[enc[k].tab_off + s].col1 != 0u;
    if (used != g.plan[k].E) { g.err = "table does not hold every element once"; return 1; }
  }
  return 0;
}

extern "C" const char* emu_sfe_error() { return g.err.c_str(); }
extern "C" uint32_t emu_sfe_window_words() { return EMU_W; }

// sums of elements and reads, the matrix's words, the repeat counter, whether the dups kernel ran
extern "C" void emu_sfe_shape(uint64_t* out5) {
  out5[0] = g.P.element.size(); out5[1] = g.P.read_ok.size(); out5[2] = g.M.size() - 4; out5[3] = g.repeats; out5[4] = g.dups_ran;
}

// the encoding as tbc_setfull_keys_encoding hands it back; per key the pitch and the matrix's offset (words); the matrix
extern "C" void emu_sfe_get(tbc_setfull_encoding* out, uint32_t* pitch, uint64_t* m_off, uint32_t* M) {
  const sfenc::Plan& P = g.P;
  const auto give = [](auto* dst, const auto& src, size_t n) { if (dst && n) std::memcpy(dst, src.data(), n * sizeof(src[0])); };
  give(out->n_elements, P.n_elements, P.n_elements.size()); give(out->n_reads, P.n_reads, P.n_reads.size());
  give(out->element, P.element, P.element.size()); give(out->add_invoke, P.add_invoke, P.add_invoke.size());
  give(out->add_ok, P.add_ok, P.add_ok.size()); give(out->read_invoke, P.read_invoke, P.read_invoke.size());
  give(out->read_ok, P.read_ok, P.read_ok.size()); give(out->dup_max, g.dup_max, P.element.size());
  give(out->dup_count, g.dup_count, g.dup_count.size()); give(out->unknown_values, g.unknown, g.unknown.size());
  out->ns_encode = 0;
  for (size_t k = 0; k < g.plan.size(); k++) { pitch[k] = g.plan[k].PITCH; m_off[k] = g.plan[k].m_off; }
  give(M, g.M, g.M.size() - 4);
}
