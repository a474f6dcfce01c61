// perf_plan.h -- the host plan of tbc_perf_series (the series behind the reference's perf plots, include/tbcheck.h): plain C++ with no
// HIP call in it.  perf_host.hip runs every call through it, and so do the emulator program of the kernels (tests/emu/emu_perf.cpp) and
// the stand-alone program of the plan (tests/emu/perf_plan.cpp), so the rules below have one statement in C.
//
//   validate   every rule of tbc_perf_in that the kernels trust, O(ops)
//   plan       O(ops), one pass: the PARTNER column (knossos.history/pair-index: per process the open invocation, in a hash map),
//              t_max over all ops, nb_all and n_plot, the cell numbering -- quantile cell (f, bucket) = f * nb_all + bucket, class
//              (f, outcome) = f * 3 + outcome - 1, class cell = class * nb_all + bucket --, the chunks of the open scan, and the
//              arena as named regions with 256 B starts.
//   steps      the call from the plan to the filled output, over a call frame: the library's and the emulator's run this one list
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/tbcheck.h"
#include "oneshot_plan.h"

#ifndef PF_SELECT_TILE
#define PF_SELECT_TILE TBC_PERF_SELECT_TILE
#endif

namespace pf {

constexpr uint32_t kPfTile = PF_SELECT_TILE;        // latencies a workgroup sorts in LDS (a power of two); the emulator build takes a small one
constexpr uint32_t kPfNone = 0xFFFFFFFFu;           // partner: none
constexpr long long kPfSecond = 1000000000ll;
constexpr long long kPfTimeEnd = 1ll << 52;         // times are below this: a double holds them exactly, and long(t / 1e9) is t / 10^9
constexpr uint32_t kPfScanTile = 256;               // cells a workgroup of the cell scan takes
constexpr uint64_t kPfCarryWords = 1ull << 22;      // the open scan's carried totals: chunks x classes words at most (but one chunk at least)
constexpr uint32_t kPfChunksMax = 4096;
static_assert((kPfTile & (kPfTile - 1u)) == 0u && kPfTile >= 2u, "the LDS tile is a power of two");

// what the kernels add up, in device memory (the head of the arena, zeroed)
struct PfAcc { uint32_t n_client, n_invocations, n_matched, n_completions, max_cell, pad[3]; };

// what the kernels take (perf_kernels.h), every pointer into the arena
struct PfArgs {
  PfAcc* acc; tbc_perf_summary* summary;
  const long long* time; const int32_t* process; const uint8_t* type; const uint16_t* f; const uint32_t* partner;
  uint32_t n_ops, n_f, nb_all, n_plot; long long t_max;
  uint32_t n_cells, n_class;                          // n_f * nb_all; n_f * 3
  uint32_t chunk_ops, n_chunks, n_scan_tiles, grid;   // grid: the workgroups of a grid-stride launch (the launcher's to choose)
  long long* op_latency; uint8_t* op_outcome; int32_t* op_open_after;
  uint32_t *q_count, *q_off, *q_cur, *tile_sum; unsigned long long* lat_cell; long long* q_value;
  uint32_t* rate_count; uint32_t* carry; unsigned long long* open_word; int32_t *open_last, *open_fill;
};

// Every kernel of the call on `stream` (a hipStream_t: this header names no HIP type): pf::sequence of perf_kernels.h over the library's
// launcher; defined in perf.hip, the unit that holds the kernels.  The grids are the sequence's to choose (`grid` of `A` is ignored).
void launch(void* stream, PfArgs A);

using oneshot::Region;
using PfRegion = Region;                   // (the name it had while this header held it: programs written against that still build)

// The call's one arena, in order: what the device adds up or claims (zeroed before the kernels), the summary, the plan's partner
// column and the caller's columns (copied in), and what the kernels write in full.
struct PfArena {
  Region acc, q_count, rate_count, carry, open_word;                                       // zeroed
  Region summary;                                                                          // (the end of the zeroed part)
  Region partner, time, process, type, f;                                                  // copied in
  Region op_latency, op_outcome, op_open_after, q_off, q_cur, tile_sum, lat_cell, q_value, open_last, open_fill;
  size_t bytes = 0;
  size_t zero_bytes() const { return summary.at; }
};

struct Plan {
  uint32_t n_ops = 0, n_f = 0, nb_all = 1, n_plot = 0, n_cells = 0, n_class = 0, chunk_ops = 64, n_chunks = 0, n_scan_tiles = 0;
  uint32_t n_client = 0, n_matched = 0;
  int64_t t_max = 0;
  std::vector<uint32_t> partner;                      // [n_ops] the op's completion / invocation, kPfNone if it has none
  PfArena arena;
};

// TBC_OK, or the status and in `err` the entry point and the op
inline tbc_status validate(const char* fn, const tbc_perf_in* in, std::string& err) {
  char buf[256];
  const auto say = [&](const char* what) { std::snprintf(buf, sizeof buf, "%s: %s", fn, what); err = buf; };
  const auto fail = [&](const char* what, uint32_t i) { std::snprintf(buf, sizeof buf, "%s: op %u: %s", fn, i, what); err = buf; };
  if (in->n_ops && (!in->time || !in->process || !in->type || !in->flags || !in->f)) { say("null argument (time, process, type, flags, f)"); return TBC_ERR_INVALID_ARG; }
  if (in->n_f > 65536u) { say("n_f is at most 65536 (f is 16 bits)"); return TBC_ERR_INVALID_ARG; }
  if (in->n_ops == 0xFFFFFFFFu) { say("2^32 - 1 ops in one call"); return TBC_ERR_INVALID_ARG; }
  for (uint32_t i = 0; i < in->n_ops; i++) {
    if (in->type[i] > TBC_PERF_T_INFO) { fail("type is not a TBC_PERF_T_*", i); return TBC_ERR_INVALID_ARG; }
    if (in->flags[i] & ~TBC_PERF_F_CLIENT) { fail("unknown op flags", i); return TBC_ERR_INVALID_ARG; }
    const bool client = (in->flags[i] & TBC_PERF_F_CLIENT) != 0;
    if (client != (in->process[i] != TBC_PERF_NO_PROCESS)) { fail("TBC_PERF_F_CLIENT is set on exactly the ops whose process is not INT32_MIN", i); return TBC_ERR_INVALID_ARG; }
    if (client && in->f[i] >= in->n_f) { fail("f is not below n_f", i); return TBC_ERR_INVALID_ARG; }
    if (in->time[i] == INT64_MIN) { fail("the op has no :time", i); return TBC_ERR_BAD_HISTORY; }
    if (in->time[i] < 0) { fail("negative :time", i); return TBC_ERR_BAD_HISTORY; }
    if (in->time[i] >= kPfTimeEnd) { fail(":time is 2^52 ns or more", i); return TBC_ERR_BAD_HISTORY; }
  }
  return TBC_OK;
}

// the buckets whose midpoint is <= t_max, as the reference compares them: doubles
inline uint32_t plotted_buckets(int64_t t_max, uint32_t nb_all) {
  return (double)(nb_all - 1u) + 0.5 <= (double)t_max / 1e9 ? nb_all : nb_all - 1u;
}

// the sizes alone (the input has passed `validate`).  TBC_OK, or TBC_ERR_UNSUPPORTED: too many cells for one call (`err` says so)
inline tbc_status sizes(const char* fn, const tbc_perf_in* in, tbc_perf_sizes& s, std::string& err) {
  int64_t t_max = 0;
  for (uint32_t i = 0; i < in->n_ops; i++) t_max = std::max(t_max, in->time[i]);
  s.n_ops = in->n_ops; s.n_f = in->n_f; s.t_max = t_max;
  s.nb_all = (uint32_t)(t_max / kPfSecond) + 1u;
  s.n_plot = plotted_buckets(t_max, s.nb_all);
  if ((uint64_t)s.n_f * 4u * s.nb_all >= (1ull << 31)) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "%s: %u f's x 4 x %u one-second buckets is 2^31 cells or more in one call", fn, s.n_f, s.nb_all);
    err = buf;
    return TBC_ERR_UNSUPPORTED;
  }
  return TBC_OK;
}

// (the input has passed `validate`.)  TBC_OK, or TBC_ERR_UNSUPPORTED: too much for one call (`err` says what)
inline tbc_status plan(const char* fn, const tbc_perf_in* in, Plan& P, std::string& err) {
  P = Plan{};
  tbc_perf_sizes s{};
  const tbc_status st = sizes(fn, in, s, err);
  if (st != TBC_OK) return st;
  P.n_ops = s.n_ops; P.n_f = s.n_f; P.t_max = s.t_max; P.nb_all = s.nb_all; P.n_plot = s.n_plot;
  P.n_cells = P.n_f * P.nb_all; P.n_class = P.n_f * 3u;
  P.partner.assign(P.n_ops, kPfNone);
  std::unordered_map<int32_t, uint32_t> open;         // process -> its open invocation
  for (uint32_t i = 0; i < P.n_ops; i++) {
    if (!(in->flags[i] & TBC_PERF_F_CLIENT)) continue;
    P.n_client++;
    if (in->type[i] == TBC_PERF_T_INVOKE) { open[in->process[i]] = i; continue; }
    const auto it = open.find(in->process[i]);
    if (it == open.end()) continue;
    P.partner[it->second] = i; P.partner[i] = it->second; P.n_matched++;
    open.erase(it);
  }
  // the open scan: chunks of whole wavefronts' worth of ops, as many as keep chunks x classes words of carried totals within bounds
  const uint64_t chunks_max = std::max<uint64_t>(1, std::min<uint64_t>(kPfChunksMax, kPfCarryWords / std::max<uint32_t>(1u, P.n_class)));
  P.chunk_ops = oneshot::chunk_size(P.n_ops, chunks_max);
  P.n_chunks = (uint32_t)(((uint64_t)P.n_ops + P.chunk_ops - 1u) / P.chunk_ops);
  P.n_scan_tiles = (P.n_cells + kPfScanTile - 1u) / kPfScanTile;
  PfArena& A = P.arena;
  oneshot::Cursor c;
  const size_t n = P.n_ops, cells = P.n_cells, ccells = (size_t)P.n_class * P.nb_all;
  A.acc = c.take(sizeof(PfAcc)); A.q_count = c.take(cells * 4); A.rate_count = c.take(ccells * 4);
  A.carry = c.take((size_t)P.n_chunks * P.n_class * 4); A.open_word = c.take(ccells * 8);
  A.summary = c.take(sizeof(tbc_perf_summary)); A.partner = c.take(n * 4);
  A.time = c.take(n * 8); A.process = c.take(n * 4); A.type = c.take(n); A.f = c.take(n * 2);
  A.op_latency = c.take(n * 8); A.op_outcome = c.take(n); A.op_open_after = c.take(n * 4);
  A.q_off = c.take(cells * 4); A.q_cur = c.take(cells * 4); A.tile_sum = c.take((size_t)P.n_scan_tiles * 4);
  A.lat_cell = c.take((size_t)P.n_matched * 8); A.q_value = c.take(cells * 4 * 8);
  A.open_last = c.take(ccells * 4); A.open_fill = c.take((size_t)P.n_class * P.n_plot * 4);
  A.bytes = c.at;
  return TBC_OK;
}

// the kernels' arguments over an arena at `base`
inline PfArgs args(const Plan& P, char* base) {
  const PfArena& L = P.arena;
  const auto at = [&](const Region& r) { return base + r.at; };
  PfArgs A{};
  A.acc = (PfAcc*)at(L.acc); A.summary = (tbc_perf_summary*)at(L.summary);
  A.time = (const long long*)at(L.time); A.process = (const int32_t*)at(L.process); A.type = (const uint8_t*)at(L.type);
  A.f = (const uint16_t*)at(L.f); A.partner = (const uint32_t*)at(L.partner);
  A.n_ops = P.n_ops; A.n_f = P.n_f; A.nb_all = P.nb_all; A.n_plot = P.n_plot; A.t_max = P.t_max;
  A.n_cells = P.n_cells; A.n_class = P.n_class; A.chunk_ops = P.chunk_ops; A.n_chunks = P.n_chunks; A.n_scan_tiles = P.n_scan_tiles;
  A.op_latency = (long long*)at(L.op_latency); A.op_outcome = (uint8_t*)at(L.op_outcome); A.op_open_after = (int32_t*)at(L.op_open_after);
  A.q_count = (uint32_t*)at(L.q_count); A.q_off = (uint32_t*)at(L.q_off); A.q_cur = (uint32_t*)at(L.q_cur); A.tile_sum = (uint32_t*)at(L.tile_sum);
  A.lat_cell = (unsigned long long*)at(L.lat_cell); A.q_value = (long long*)at(L.q_value);
  A.rate_count = (uint32_t*)at(L.rate_count); A.carry = (uint32_t*)at(L.carry); A.open_word = (unsigned long long*)at(L.open_word);
  A.open_last = (int32_t*)at(L.open_last); A.open_fill = (int32_t*)at(L.open_fill);
  return A;
}

// The call from a finished plan to the filled `out`, over an open frame (oneshot_plan.h, "the frame interface"): the zeroed head, the
// plan's partner column and the caller's columns straight to their regions, the kernels -- run.sequence(A) --, and the results back in
// one copy per array the caller asked for.
template <class Frame, class Run>
tbc_status steps(Frame& C, Run&& run, const tbc_perf_in* in, const Plan& P, tbc_perf_out* out) {
  const PfArena& L = P.arena;
  C.fill(L.acc, 0, L.zero_bytes());
  C.put(L.partner, P.partner.data());
  C.put(L.time, in->time); C.put(L.process, in->process); C.put(L.type, in->type); C.put(L.f, in->f);
  C.timed([&] { run.sequence(args(P, C.base())); });
  C.get(out->op_latency, L.op_latency); C.get(out->op_outcome, L.op_outcome); C.get(out->op_open_after, L.op_open_after);
  C.get(out->q_count, L.q_count); C.get(out->q_value, L.q_value); C.get(out->rate_count, L.rate_count);
  C.get(out->open_last, L.open_last); C.get(out->open_fill, L.open_fill);
  C.get(&out->summary, L.summary);
  if (C.sync() != TBC_OK) return C.status;
  oneshot::account(C, out->summary);
  return TBC_OK;
}

}  // namespace pf
