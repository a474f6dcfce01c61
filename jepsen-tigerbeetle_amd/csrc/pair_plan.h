// pair_plan.h -- the host plan of tbc_pair_events_batch (tbc_pair_events for many histories a call, on the device; include/tbcheck.h):
// plain C++ with no HIP call in it.  pair_host.hip runs every call through it, and so does the emulator program of the kernels
// (tests/emu/emu_pair.cpp), so the rules below have one statement in C.
//
//   validate   every rule of tbc_event_batch / tbc_pair_out that the kernels trust, O(histories): nothing looks at an event
//   plan       the arena as named regions with 256 B starts: the caller's columns as they are (14 B an event), the scratch per
//              event (comp_of: an invocation's completion row; the surviving ops of a history in order, at the history's first
//              events: invocation row, completion row, dense process), the descriptors per history, and the op columns the caller asked
//              for, for min(ops_cap, events) ops (a history has no more ops than events)
//   steps      the call from the plan to the filled output, over a call frame: the library's and the emulator's run this one list
// THE PACKED FORM (tbc_pair_packed_batch; include/tbcheck.h, "the packed event word"): the same plan and the same list, with the region
// ev_word (4 B an event) in place of type, f, a and b (10 B); PrArgs.ev_word tells the kernels which they read.
// A BATCH'S EVENT ARENA (tbc_batch_map_events / tbc_batch_submit_events, batch_stream.hip): plan_batch lays the same regions out once
// for the batch's capacities -- packed input, scratch, descriptors, no op columns: those are the batch's device stage -- and
// batch_refusal states the all-or-nothing rule of such an input.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include "../../include/tbcheck.h"
#include "oneshot_plan.h"

namespace pr {

constexpr uint32_t kPrTable = TBC_PAIR_MAX_PROCESS;   // entries of the process table in LDS (a power of two): the wire format's processes
constexpr uint32_t kPrNone = 0xFFFFFFFFu;             // comp_of: no completion; bad_row: none
static_assert((kPrTable & (kPrTable - 1u)) == 0u && kPrTable == 4096u, "the table's hash folds 12 bits");

// the table's hash of a process id (the kernel's; the tests make colliding ids with it)
constexpr uint32_t table_hash(uint32_t k) { return (k ^ (k >> 12) ^ (k >> 24)) & (kPrTable - 1u); }

// what the kernels add up, in device memory (the head of the arena, zeroed)
struct PrAcc { unsigned long long total_ops; uint32_t n_bad, pad; };

// what the kernels take (pair_kernels.h), every pointer into the arena
struct PrArgs {
  PrAcc* acc;
  uint32_t n_hist, grid, want_word, pad;
  unsigned long long out_cap;                          // ops the output regions hold
  const unsigned long long* ev_off;
  const uint8_t* type; const int32_t* process; const uint8_t* f; const int32_t* a; const int32_t* b;
  uint32_t* comp_of;                                   // [events] by invocation row: its completion's row, kPrNone
  uint32_t *s_inv, *s_ret, *s_proc;                    // [events] history h's surviving op k at ev_off[h] + k
  uint32_t* cnt;                                       // [n_hist] surviving ops (0 for a history that is refused)
  unsigned long long* op_off; uint32_t *n_events, *n_process; int32_t* status; uint32_t* bad_row;
  uint8_t* o_f; int32_t *o_a, *o_b, *o_process; uint32_t *o_inv, *o_ret, *o_word;      // null: not asked for
  const uint32_t* ev_word;                             // null: type, f, a, b are read from their columns; else from TBC_EVENT_WORD
};

// Every kernel of the call on `stream` (a hipStream_t: this header names no HIP type): the sequences of pair_kernels.h over the
// library's launcher; defined in pair.hip, the unit that holds the kernels.
void launch_pair(void* stream, PrArgs A);
void launch_emit(void* stream, PrArgs A);

using oneshot::Region;

struct PrArena {
  Region acc;                                                                               // zeroed
  Region ev_off, type, process, f, a, b;                                                    // copied in
  Region ev_word;                                                                           // ... the packed form: instead of type, f, a, b
  Region comp_of;                                                                           // 0xFF all over
  Region s_inv, s_ret, s_proc, cnt, op_off, n_events, n_process, status, bad_row;           // written by the kernels
  Region o_f, o_a, o_b, o_process, o_inv, o_ret, o_word;                                    // (0 bytes: not asked for)
  size_t bytes = 0;
};

struct Plan {
  uint32_t n_hist = 0;
  uint64_t n_events = 0, out_cap = 0;
  bool packed = false;                                 // the events are ev_word + process
  PrArena arena;
};

// TBC_OK, or TBC_ERR_INVALID_ARG and in `err` the entry point and the rule
// (the rules of ev_off and of the output arrays: what the two forms of the input share)
// (the rules of the output arrays alone: tbc_pair_keyed_events, whose ev_off is made on the device, holds its `out` to them; split_plan.h)
inline tbc_status validate_out(const char* fn, const tbc_pair_out* out, std::string& err) {
  const auto say = [&](const char* what) { err = std::string(fn) + ": " + what; return TBC_ERR_INVALID_ARG; };
  if (out && (!out->op_off || !out->n_events || !out->n_process || !out->status || !out->bad_row)) return say("null argument (op_off, n_events, n_process, status, bad_row)");
  if (out && out->ops_cap && (!out->inv_pos || !out->ret_pos)) return say("null argument (inv_pos, ret_pos)");
  return TBC_OK;
}
inline tbc_status validate_offsets(const char* fn, uint32_t n_hist, const uint64_t* ev_off, const tbc_pair_out* out, std::string& err) {
  char buf[256];
  const auto say = [&](const char* what) { std::snprintf(buf, sizeof buf, "%s: %s", fn, what); err = buf; return TBC_ERR_INVALID_ARG; };
  if (!ev_off) return say("null argument (ev_off)");
  if (validate_out(fn, out, err) != TBC_OK) return TBC_ERR_INVALID_ARG;
  if (ev_off[0] != 0) return say("ev_off[0] is not 0");
  for (uint32_t h = 0; h < n_hist; h++) {
    if (ev_off[h + 1] < ev_off[h]) { std::snprintf(buf, sizeof buf, "%s: history %u: ev_off descends", fn, h); err = buf; return TBC_ERR_INVALID_ARG; }
    if (ev_off[h + 1] - ev_off[h] >= (1ull << 31)) { std::snprintf(buf, sizeof buf, "%s: history %u has 2^31 events or more", fn, h); err = buf; return TBC_ERR_INVALID_ARG; }
  }
  if (ev_off[n_hist] > 0xFFFFFFFFull) return say("more than 2^32 - 1 events in one call");
  return TBC_OK;
}

inline tbc_status validate(const char* fn, const tbc_event_batch* in, const tbc_pair_out* out, std::string& err) {
  const tbc_status st = validate_offsets(fn, in->n_hist, in->ev_off, out, err);
  if (st != TBC_OK) return st;
  if (in->ev_off[in->n_hist] && (!in->type || !in->process || !in->f || !in->a || !in->b)) { err = std::string(fn) + ": null argument (type, process, f, a, b)"; return TBC_ERR_INVALID_ARG; }
  return TBC_OK;
}

inline tbc_status validate(const char* fn, const tbc_packed_event_batch* in, const tbc_pair_out* out, std::string& err) {
  const tbc_status st = validate_offsets(fn, in->n_hist, in->ev_off, out, err);
  if (st != TBC_OK) return st;
  if (in->ev_off[in->n_hist] && (!in->ev_word || !in->process)) { err = std::string(fn) + ": null argument (ev_word, process)"; return TBC_ERR_INVALID_ARG; }
  return TBC_OK;
}

// the arena of `nh` histories and `n_events` events, packed or in columns; `out` (null: none) names the op columns asked for
inline void plan_sizes(uint32_t n_hist, uint64_t n_events, uint64_t out_cap, bool packed, const tbc_pair_out* out, Plan& P) {
  P = Plan{};
  P.n_hist = n_hist;
  P.n_events = n_events;
  P.out_cap = out_cap;
  P.packed = packed;
  PrArena& A = P.arena;
  oneshot::Cursor c;
  const size_t n = (size_t)P.n_events, nh = P.n_hist, cap = out ? (size_t)P.out_cap : 0;
  const tbc_pair_out none{};
  if (!out) out = &none;
  A.acc = c.take(sizeof(PrAcc));
  A.ev_off = c.take((nh + 1) * 8);
  A.type = c.take(packed ? 0 : n); A.process = c.take(n * 4); A.f = c.take(packed ? 0 : n); A.a = c.take(packed ? 0 : n * 4); A.b = c.take(packed ? 0 : n * 4);
  A.ev_word = c.take(packed ? n * 4 : 0);
  A.comp_of = c.take(n * 4);
  A.s_inv = c.take(n * 4); A.s_ret = c.take(n * 4); A.s_proc = c.take(n * 4);
  A.cnt = c.take(nh * 4); A.op_off = c.take((nh + 1) * 8); A.n_events = c.take(nh * 4); A.n_process = c.take(nh * 4);
  A.status = c.take(nh * 4); A.bad_row = c.take(nh * 4);
  A.o_f = c.take(out->f ? cap : 0); A.o_a = c.take(out->a ? cap * 4 : 0); A.o_b = c.take(out->b ? cap * 4 : 0);
  A.o_process = c.take(out->process ? cap * 4 : 0); A.o_inv = c.take(out->inv_pos ? cap * 4 : 0); A.o_ret = c.take(out->ret_pos ? cap * 4 : 0);
  A.o_word = c.take(out->word ? cap * 4 : 0);
  A.bytes = c.at;
}

// (the input has passed `validate`)
inline void plan(const tbc_event_batch* in, const tbc_pair_out* out, Plan& P) {
  const uint64_t n = in->ev_off[in->n_hist];
  plan_sizes(in->n_hist, n, std::min<uint64_t>(out->ops_cap, n), false, out, P);
}
inline void plan(const tbc_packed_event_batch* in, const tbc_pair_out* out, Plan& P) {
  const uint64_t n = in->ev_off[in->n_hist];
  plan_sizes(in->n_hist, n, std::min<uint64_t>(out->ops_cap, n), true, out, P);
}
// a batch's event arena: packed events for the batch's capacities, the scratch and the descriptors; the op columns are emitted into
// the batch's device stage, `ops_cap` ops a third (args_stage)
inline void plan_batch(uint32_t n_hist_cap, uint64_t events_cap, uint64_t ops_cap, Plan& P) { plan_sizes(n_hist_cap, events_cap, ops_cap, true, nullptr, P); }

// the kernels' arguments over an arena at `base`
inline PrArgs args(const Plan& P, const tbc_pair_out* out, char* base) {
  const PrArena& L = P.arena;
  const auto at = [&](const Region& r) { return base + r.at; };
  PrArgs A{};
  A.acc = (PrAcc*)at(L.acc);
  A.ev_word = P.packed ? (const uint32_t*)at(L.ev_word) : nullptr;
  A.n_hist = P.n_hist; A.want_word = out->word ? 1u : 0u; A.out_cap = P.out_cap;
  A.ev_off = (const unsigned long long*)at(L.ev_off);
  A.type = (const uint8_t*)at(L.type); A.process = (const int32_t*)at(L.process); A.f = (const uint8_t*)at(L.f);
  A.a = (const int32_t*)at(L.a); A.b = (const int32_t*)at(L.b);
  A.comp_of = (uint32_t*)at(L.comp_of); A.s_inv = (uint32_t*)at(L.s_inv); A.s_ret = (uint32_t*)at(L.s_ret); A.s_proc = (uint32_t*)at(L.s_proc);
  A.cnt = (uint32_t*)at(L.cnt); A.op_off = (unsigned long long*)at(L.op_off); A.n_events = (uint32_t*)at(L.n_events);
  A.n_process = (uint32_t*)at(L.n_process); A.status = (int32_t*)at(L.status); A.bad_row = (uint32_t*)at(L.bad_row);
  A.o_f = out->f ? (uint8_t*)at(L.o_f) : nullptr; A.o_a = out->a ? (int32_t*)at(L.o_a) : nullptr; A.o_b = out->b ? (int32_t*)at(L.o_b) : nullptr;
  A.o_process = out->process ? (int32_t*)at(L.o_process) : nullptr;
  A.o_inv = out->inv_pos ? (uint32_t*)at(L.o_inv) : nullptr; A.o_ret = out->ret_pos ? (uint32_t*)at(L.o_ret) : nullptr;
  A.o_word = out->word ? (uint32_t*)at(L.o_word) : nullptr;
  return A;
}

// the kernels' arguments for `n_hist` histories in a batch's event arena (plan_batch) at `base`: the wire word asked for, and the
// three op columns a batch takes emitted to the thirds of `stage` (3 * P.out_cap words)
inline PrArgs args_stage(const Plan& P, uint32_t n_hist, char* base, uint32_t* stage) {
  tbc_pair_out none{};
  PrArgs A = args(P, &none, base);
  A.n_hist = n_hist; A.want_word = 1u;
  A.o_word = stage; A.o_inv = stage + P.out_cap; A.o_ret = stage + 2u * P.out_cap;
  return A;
}

// The all-or-nothing rule of an input of events for a batch, from the descriptors the pairing left: TBC_OK, or the status the call
// returns and why -- a history that is refused (malformed before unsupported), or more surviving ops than the batch's slots hold
inline tbc_status batch_refusal(const char* fn, uint32_t n_hist, const PrAcc& acc, const int32_t* status, const uint32_t* bad_row, uint64_t ops_cap, std::string& err) {
  char buf[256];
  if (acc.n_bad) {
    uint32_t first = n_hist, first_bad = n_hist;
    for (uint32_t h = 0; h < n_hist; h++) {
      if (status[h] != TBC_OK && first == n_hist) first = h;
      if (status[h] == TBC_ERR_BAD_HISTORY) { first_bad = h; break; }
    }
    if (first_bad < n_hist) {
      std::snprintf(buf, sizeof buf, "%s: history %u of %u refused: malformed at row %u", fn, first_bad, acc.n_bad, bad_row[first_bad]);
      err = buf;
      return TBC_ERR_BAD_HISTORY;
    }
    std::snprintf(buf, sizeof buf, "%s: history %u of %u refused: more than %u processes, or ops the wire format does not hold", fn, first, acc.n_bad, kPrTable);
    err = buf;
    return TBC_ERR_UNSUPPORTED;
  }
  if (acc.total_ops > ops_cap) {
    std::snprintf(buf, sizeof buf, "%s: %llu ops survive, the batch's slots hold %llu", fn, acc.total_ops, (unsigned long long)ops_cap);
    err = buf;
    return TBC_ERR_INVALID_ARG;
  }
  return TBC_OK;
}

// The call from a finished plan to the filled `out`, over an open frame (oneshot_plan.h, "the frame interface"): the caller's columns
// straight to their regions, the pairing and the scan of the histories' op counts -- run.pair(A) --, the total read back and held
// against ops_cap BEFORE any op is written, the op columns -- run.emit(A) --, and the results back in one copy per array the caller
// asked for, the first `total` ops of each.
template <class Frame>
void put_events(Frame& C, const PrArena& L, const tbc_event_batch* in) {
  C.put(L.type, in->type); C.put(L.process, in->process); C.put(L.f, in->f); C.put(L.a, in->a); C.put(L.b, in->b);
}
template <class Frame>
void put_events(Frame& C, const PrArena& L, const tbc_packed_event_batch* in) { C.put(L.ev_word, in->ev_word); C.put(L.process, in->process); }

// The second half of the call, from the pairing launched to the filled `out`: what `steps` below and the keyed call (split_plan.h,
// whose histories are made on the device: A.n_hist of them, P.n_hist at most) both end with.
template <class Frame, class Run>
tbc_status finish(Frame& C, Run&& run, const char* fn, const PrArena& L, const PrArgs& A, tbc_pair_out* out) {
  const size_t nh = A.n_hist;
  PrAcc acc{};
  C.get(&acc, L.acc);
  if (C.sync() != TBC_OK) return C.status;
  if (acc.total_ops > out->ops_cap)
    return C.fail(TBC_ERR_INVALID_ARG, "%s: %llu ops survive, ops_cap is %llu", fn, acc.total_ops, (unsigned long long)out->ops_cap);
  const size_t T = (size_t)acc.total_ops;
  if (T) C.timed([&] { run.emit(A); });
  C.get(out->f, L.o_f, out->f ? T : 0); C.get(out->a, L.o_a, out->a ? T * 4 : 0); C.get(out->b, L.o_b, out->b ? T * 4 : 0);
  C.get(out->process, L.o_process, out->process ? T * 4 : 0);
  C.get(out->inv_pos, L.o_inv, out->inv_pos ? T * 4 : 0); C.get(out->ret_pos, L.o_ret, out->ret_pos ? T * 4 : 0);
  C.get(out->word, L.o_word, out->word ? T * 4 : 0);
  C.get(out->op_off, L.op_off, (nh + 1) * 8); C.get(out->n_events, L.n_events, nh * 4); C.get(out->n_process, L.n_process, nh * 4);
  C.get(out->status, L.status, nh * 4); C.get(out->bad_row, L.bad_row, nh * 4);
  if (C.sync() != TBC_OK) return C.status;
  out->n_bad = acc.n_bad; out->reserved0 = 0; out->n_ops = acc.total_ops;
  oneshot::account(C, *out);
  return TBC_OK;
}

template <class Frame, class Run, class In>
tbc_status steps(Frame& C, Run&& run, const char* fn, const In* in, const Plan& P, tbc_pair_out* out) {
  const PrArena& L = P.arena;
  const PrArgs A = args(P, out, C.base());
  C.fill(L.acc, 0, L.acc.bytes);
  C.put(L.ev_off, in->ev_off);
  put_events(C, L, in);
  C.fill(L.comp_of, 0xFF, L.comp_of.bytes);
  C.timed([&] { run.pair(A); });
  return finish(C, run, fn, L, A, out);
}

}  // namespace pr
