// set_full_encode_plan.h -- jepsen.checker/set-full's encoding of a history given as op columns (tbc_setfull_keys_create_ops): the
// O(ops) part, on the host.  Plain C++ (no HIP): set_full_host.hip includes it, and so does the emulator program of the encoding kernels
// (tests/emu/emu_setfull_encode.cpp), so the rules below have one statement in C.
//
// From a key's columns (tbc_setfull_ops_in: index, type, f, process, value per client op, in history order) the plan makes what
// sf_create takes for a key -- add_invoke / add_ok per element, read_invoke / read_ok per read -- plus the element values and, per
// read, WHERE its raw values lie in `vals` (a slice, not a copy).  The O(values) part -- which column each value of each read names --
// is the device's (set_full_encode.h).  The rules (jepsen.checker/set-full, as jepsen/set_full.py `Encoded` states them):
//   elements  an element is a distinct :add value; an :add INVOCATION makes a fresh element state, so an element added again is
//             numbered by its LAST invocation, and elements are numbered in the order of those
//   add_ok    the first :ok add of the value after that last invocation, whichever process sent it; an :ok add of a value never
//             invoked is ignored
//   reads     an :ok read is paired with the open read invocation of ITS process; :fail closes the open read; :info leaves it open
//             until the process invokes a read again; an :ok read whose value is nil, or that has no open invocation, closes the open
//             read and makes no row; an :ok read with an empty value makes an all-zero row; rows are ordered by invocation
// An :add whose value is nil (TBC_SETFULL_T_NIL) names no int64 element and is skipped.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/tbcheck.h"

namespace sfenc {

// What the plan makes of all keys, key after key (the layout of tbc_setfull_keys_in and tbc_setfull_encoding).
struct Plan {
  std::vector<uint32_t> n_elements, n_reads;               // [n_keys]
  std::vector<int64_t> element;                            // [sum n_elements] the value of each column
  std::vector<uint32_t> add_invoke, add_ok;                // [sum n_elements]
  std::vector<uint32_t> read_invoke, read_ok;              // [sum n_reads]
  std::vector<uint64_t> val_lo, val_hi;                    // [sum n_reads] the read's values are vals[val_lo .. val_hi)
  uint64_t n_values = 0;                                   // the greatest val_hi: how much of `vals` the rows name
};

// Every rule of tbc_setfull_ops_in that can be checked without reading a value, before anything else looks at the columns.  false: `err`
// names the entry point, the key and the op (the op by its row in the key and by its index).
inline bool validate(const char* fn, const tbc_setfull_ops_in* in, std::string& err) {
  char buf[256];
  const auto fail = [&](const char* what, uint32_t k, uint64_t i) {
    std::snprintf(buf, sizeof buf, "%s: key %u op %llu (index %u): %s", fn, k, (unsigned long long)(i - in->op_off[k]), in->index[i], what);
    err = buf;
    return false;
  };
  for (uint32_t k = 0; k < in->n_keys; k++)
    if (in->op_off[k + 1] < in->op_off[k]) {
      std::snprintf(buf, sizeof buf, "%s: key %u: op_off must be ascending", fn, k);
      err = buf;
      return false;
    }
  if (in->val_off[0] != 0) { std::snprintf(buf, sizeof buf, "%s: val_off[0] must be 0", fn); err = buf; return false; }
  for (uint32_t k = 0; k < in->n_keys; k++) {
    for (uint64_t i = in->op_off[k]; i < in->op_off[k + 1]; i++) {
      if (i > in->op_off[k] && in->index[i] <= in->index[i - 1]) return fail("index must be strictly ascending within a key", k, i);
      if (in->index[i] == 0xFFFFFFFFu) return fail("index 2^32 - 1 is TBC_NO_OP", k, i);
      if ((in->type[i] & ~TBC_SETFULL_T_NIL) > TBC_SETFULL_T_INFO) return fail("type is not a TBC_SETFULL_T_*", k, i);
      if (in->f[i] > TBC_SETFULL_OP_READ) return fail("f is not a TBC_SETFULL_OP_*", k, i);
      if (in->val_off[i + 1] < in->val_off[i]) return fail("val_off must be ascending", k, i);
    }
  }
  return true;
}

// The plan of every key (the input has passed `validate`).  O(ops): one hash map of the key's elements, one of its processes' open reads.
inline void plan(const tbc_setfull_ops_in* in, Plan& P) {
  struct Elem { uint32_t invoke, ok; };
  struct Read { uint32_t invoke, ok; uint64_t lo, hi; };
  std::unordered_map<int64_t, Elem> elems;
  std::unordered_map<int64_t, uint32_t> open_reads;        // process -> its open read's invocation
  std::vector<Read> reads;
  P = Plan{};
  P.n_elements.assign(in->n_keys, 0u); P.n_reads.assign(in->n_keys, 0u);
  for (uint32_t k = 0; k < in->n_keys; k++) {
    elems.clear(); open_reads.clear(); reads.clear();
    const uint64_t o0 = in->op_off[k], o1 = in->op_off[k + 1];
    for (uint64_t i = o0; i < o1; i++) {
      const uint32_t type = in->type[i] & ~TBC_SETFULL_T_NIL, idx = in->index[i];
      const bool nil = (in->type[i] & TBC_SETFULL_T_NIL) != 0;
      if (in->f[i] == TBC_SETFULL_OP_ADD) {
        if (nil) continue;
        if (type == TBC_SETFULL_T_INVOKE) {
          elems[in->value[i]] = Elem{idx, 0xFFFFFFFFu};                    // a fresh element state: nothing known yet
        } else if (type == TBC_SETFULL_T_OK) {
          const auto it = elems.find(in->value[i]);
          if (it != elems.end() && it->second.ok == 0xFFFFFFFFu) it->second.ok = idx;
        }
      } else if (in->f[i] == TBC_SETFULL_OP_READ) {
        if (type == TBC_SETFULL_T_INVOKE) {
          open_reads[in->process[i]] = idx;
        } else if (type == TBC_SETFULL_T_FAIL) {
          open_reads.erase(in->process[i]);
        } else if (type == TBC_SETFULL_T_OK) {
          const auto it = open_reads.find(in->process[i]);
          if (it == open_reads.end()) continue;
          if (!nil) reads.push_back(Read{it->second, idx, in->val_off[i], in->val_off[i + 1]});
          open_reads.erase(it);
        }
      }
    }
    // elements in the order of their last invocation: the ops once more, an invocation counts if it is its value's last
    for (uint64_t i = o0; i < o1; i++) {
      if (in->f[i] != TBC_SETFULL_OP_ADD || in->type[i] != TBC_SETFULL_T_INVOKE) continue;
      const Elem& e = elems.find(in->value[i])->second;
      if (e.invoke != in->index[i]) continue;
      P.element.push_back(in->value[i]); P.add_invoke.push_back(e.invoke); P.add_ok.push_back(e.ok);
    }
    std::sort(reads.begin(), reads.end(), [](const Read& a, const Read& b) { return a.invoke < b.invoke; });
    for (const Read& r : reads) {
      P.read_invoke.push_back(r.invoke); P.read_ok.push_back(r.ok); P.val_lo.push_back(r.lo); P.val_hi.push_back(r.hi);
      P.n_values = std::max(P.n_values, r.hi);
    }
    P.n_elements[k] = (uint32_t)elems.size(); P.n_reads[k] = (uint32_t)reads.size();
  }
}

// the capacity of a key's element table: the power of two at or above 2 E (0 for a key without elements: every value misses)
inline uint64_t table_slots(uint32_t E) {
  if (E == 0) return 0;
  uint64_t c = 2;
  while (c < 2ull * E) c <<= 1;
  return c;
}

}  // namespace sfenc
