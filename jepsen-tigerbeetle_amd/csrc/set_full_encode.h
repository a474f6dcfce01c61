// set_full_encode.h -- the O(values) part of tbc_setfull_keys_create_ops on the MI355X (gfx950): from the raw values of every read to
// the reads x elements membership matrix the scan loads, and the duplicates.  Included by set_full_host.hip; the host part (which value is
// which column, which read is which row, where a row's values lie) is set_full_encode_plan.h, the tables' slots and each key's share of
// them (SfEncSlot, SfEncKey) set_full_plan.h.
//
//   sf_table_build_kernel  a thread per element of every key: the element's value goes into its key's open-addressing table (16 B
//                          slots {value, column + 1}; capacity the power of two at or above 2 E, linear probing).  A thread claims the
//                          first free slot of its probe sequence by a CAS on the slot's column word and then writes the value: a
//                          key's elements are distinct, so an insert never compares values.  The kernel boundary orders the build
//                          before every lookup.
//   sf_values_kernel<W>    a workgroup of 256 per read row (grid-stride over the rows of all keys, as setfull_rows_kernel): the row is
//                          assembled in an LDS window of W words -- zeroed, then the row's values streamed (8 B a lane, coalesced), each
//                          probed in the table and its bit OR-ed into the window -- and the window written to the matrix with 16 B
//                          stores once all values are in, the padding up to the pitch as zeros: no word the scan loads is left unset.
//                          A row wider than the window takes one pass over its values per window, each keeping its own columns.  A
//                          value that names no element is dropped and counted (the first pass only; one atomic per wavefront).  An OR
//                          that finds its bit set already is a REPEAT: the row's flag byte and the key's are set and a global counter
//                          grows -- which is all the common path pays for duplicates.
//   sf_dups_kernel         launched only if that counter, read back at create, is not zero: the exact multiplicities.  A workgroup per
//                          key that has flagged rows, one flagged row at a time: count every value of the row into the key's cnt[e],
//                          barrier, dup_max[e] = max(dup_max[e], cnt[e]) where cnt[e] > 1, barrier, zero the touched cnt[e]; at the end
//                          the key's elements with dup_max > 1 are counted.
// Ballots, the workgroup barrier and the workgroup's index / thread go through wave_env.h / wave_env_wg.h; the atomics (on LDS words
// and on global memory) are plain HIP, which tests/emu/emu_setfull_encode.cpp states for the host emulator -- these very kernels run
// there lane by lane, with a window of a few words, against jepsen/set_full.py `Encoded` (tests/test_set_full_encode_emu.py).
#pragma once
#include "wave_env_wg.h"
#include "set_full_plan.h"

namespace {

struct SfEncArgs {
  const SfKeyPlan* plan; const uint32_t* first; const SfEncKey* enc; uint32_t n_keys, R_all, E_all, grid;
  const long long* element;                  // [E_all] the value of each column, key after key
  SfEncSlot* slots;                          // every key's table (zeroed before the build)
  const long long* vals;                     // the reads' raw values
  const unsigned long long *val_lo, *val_hi; // [R_all] row r's values are vals[val_lo[r] .. val_hi[r])
  uint32_t* M;
  uint8_t* row_flag;                         // [R_all] 1: the row holds a repeat
  uint32_t* key_flag;                        // [n_keys] 1: some row of the key does
  unsigned long long* unknown;               // [n_keys]
  uint32_t* repeats;                         // one counter for the whole object
  uint32_t *cnt, *dup_max;                   // [E_all] each: sf_dups_kernel's scratch (zero between rows) and result
  uint32_t* dup_count;                       // [n_keys]
};

// (sf_enc_hash and sf_enc_lookup, the probe of a table, are enc_table.h's: the ledger checkers probe a table of the same slots)

// the key that holds element g of the object (elements lie key after key): the last key whose elem_base is <= g -- a key without
// elements shares its successor's base and is never picked
__device__ __forceinline__ uint32_t sf_enc_key_of_element(const SfKeyPlan* __restrict__ plan, uint32_t n_keys, uint32_t g) {
  uint32_t lo = 0, hi = n_keys;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (plan[mid].elem_base <= g) lo = mid; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(256) void sf_table_build_kernel(SfEncArgs A) {
  const uint32_t g = wv::wg_index() * 256u + wv::wg_thread();
  if (g >= A.E_all) return;
  const uint32_t key = sf_enc_key_of_element(A.plan, A.n_keys, g);
  const SfEncKey k = A.enc[key];
  SfEncSlot* const tab = A.slots + k.tab_off;
  const long long v = A.element[g];
  const uint32_t col1 = g - A.plan[key].elem_base + 1u;
  for (uint32_t s = sf_enc_hash(v) & k.mask;; s = (s + 1u) & k.mask)
    if (atomicCAS(&tab[s].col1, 0u, col1) == 0u) { tab[s].value = v; return; }
}

template <uint32_t W>
__global__ __launch_bounds__(256) void sf_values_kernel(SfEncArgs A) {
  static_assert(W % 4u == 0u, "the window is written with 16 B stores");
  __shared__ uint32_t s_win[W];
  const uint32_t t = wv::wg_thread();
  for (uint32_t r = wv::wg_index(); r < A.R_all; r += A.grid) {
    const uint32_t key = sf_find_key(A.first + kFirstRows * (A.n_keys + 1u), A.n_keys, r);
    const SfKeyPlan& p = A.plan[key];
    const SfEncKey k = A.enc[key];
    const SfEncSlot* __restrict__ tab = A.slots + k.tab_off;
    uint32_t* __restrict__ row = A.M + p.m_off + (uint64_t)(r - p.row_base) * p.PITCH;
    const unsigned long long lo = A.val_lo[r], hi = A.val_hi[r];
    const uint32_t E = p.E, PITCH = p.PITCH;
    uint32_t n_miss = 0, n_rep = 0;                       // of this WAVEFRONT (from ballots: uniform across it)
    // (a key without elements has no words to write, but its reads' values are all unknown: one pass that only counts)
    for (uint32_t w0 = 0; w0 == 0u || w0 < PITCH; w0 += W) {
      const uint32_t wn = PITCH - w0 < W ? PITCH - w0 : W;
      for (uint32_t i = t; i < wn; i += 256u) s_win[i] = 0u;
      wv::wg_barrier();
      for (unsigned long long base = lo; base < hi; base += 256u) {
        const unsigned long long i = base + t;
        const bool in = i < hi;
        uint32_t col = kNoneU;
        if (in && E) col = sf_enc_lookup(tab, k.mask, A.vals[i]);
        bool rep = false;
        if (col != kNoneU && (col >> 5) - w0 < wn) {      // (unsigned: a column below the window wraps past wn)
          const uint32_t bit = 1u << (col & 31u);
          rep = (atomicOr(&s_win[(col >> 5) - w0], bit) & bit) != 0u;
        }
        if (w0 == 0u) n_miss += (uint32_t)__popcll(wv::ballot(in && col == kNoneU));
        n_rep += (uint32_t)__popcll(wv::ballot(rep));
      }
      wv::wg_barrier();
      for (uint32_t i = 4u * t; i < wn; i += 1024u)
        *reinterpret_cast<uint4*>(row + w0 + i) = make_uint4(s_win[i], s_win[i + 1u], s_win[i + 2u], s_win[i + 3u]);
      wv::wg_barrier();                                   // (the window is zeroed again only when everybody has stored from it)
    }
    if ((t & 63u) == 0u) {
      if (n_miss) atomicAdd(&A.unknown[key], (unsigned long long)n_miss);
      if (n_rep) { atomicAdd(A.repeats, n_rep); A.row_flag[r] = 1; atomicOr(&A.key_flag[key], 1u); }
    }
  }
}

// cnt / dup_max are touched by atomics only (several wavefronts of the workgroup, words that no plain load may have cached)
__global__ __launch_bounds__(256) void sf_dups_kernel(SfEncArgs A) {
  const uint32_t key = wv::wg_index(), t = wv::wg_thread();
  if (A.key_flag[key] == 0u) return;
  const SfKeyPlan& p = A.plan[key];
  const SfEncKey k = A.enc[key];
  const SfEncSlot* __restrict__ tab = A.slots + k.tab_off;
  uint32_t* const cnt = A.cnt + p.elem_base;
  uint32_t* const dup_max = A.dup_max + p.elem_base;
  for (uint32_t r = p.row_base; r < p.row_base + p.R; r++) {
    if (A.row_flag[r] == 0u) continue;                    // (uniform across the workgroup)
    const unsigned long long lo = A.val_lo[r], hi = A.val_hi[r];
    for (unsigned long long i = lo + t; i < hi; i += 256u) {
      const uint32_t col = sf_enc_lookup(tab, k.mask, A.vals[i]);
      if (col != kNoneU) atomicAdd(&cnt[col], 1u);
    }
    wv::wg_barrier();
    for (unsigned long long i = lo + t; i < hi; i += 256u) {
      const uint32_t col = sf_enc_lookup(tab, k.mask, A.vals[i]);
      if (col == kNoneU) continue;
      const uint32_t c = atomicAdd(&cnt[col], 0u);
      if (c > 1u) atomicMax(&dup_max[col], c);
    }
    wv::wg_barrier();
    for (unsigned long long i = lo + t; i < hi; i += 256u) {
      const uint32_t col = sf_enc_lookup(tab, k.mask, A.vals[i]);
      if (col != kNoneU) atomicAnd(&cnt[col], 0u);
    }
    wv::wg_barrier();
  }
  uint32_t n = 0;
  for (uint32_t e0 = 0; e0 < p.E; e0 += 256u) {
    const uint32_t e = e0 + t;
    n += (uint32_t)__popcll(wv::ballot(e < p.E && atomicMax(&dup_max[e], 0u) > 1u));
  }
  if ((t & 63u) == 0u && n) atomicAdd(&A.dup_count[key], n);
}

}  // namespace
