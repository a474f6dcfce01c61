// split_kernels.h -- tbc_pair_keyed_events on the MI355X (gfx950): the kernels that split ONE keyed event history by key.  split.hip
// compiles them into libtbcheck.so; their launches are sp::keys_sequence and sp::sort_sequence at the end of this file; the host plan
// (validation, the arena, the steps) is split_plan.h.  The specification is columns.split_events: the distinct keys in order of FIRST
// APPEARANCE, every key's rows in the order they had.  The pairing kernels (pair_kernels.h) then run unchanged over the keys.
//
// TWO RULES.  (1) No output depends on the order in which atomics arrive: the table's atomics claim a slot and take a MINIMUM over rows,
// and that is all they do; every position comes from a scan or from a ballot, i.e. from the row's number.  (2) No workgroup waits for
// another: the kernel boundary is the only ordering between workgroups.  Which SLOT of the table a key gets depends on arrival, as it
// does in pair_kernels.h; no output does.
//
// In launch order (a TILE is sp::kTile = 1,024 rows, walked by one wavefront in 16 chunks of 64, lane = row):
//   sp_insert_kernel   a row per thread: the key's slot in the table (HBM; open addressing from sp::table_hash, linear probing, a slot is
//                      key << 32 | first_row, all ones when empty), claimed by a 64-bit compare-and-swap; a later row of the key lowers
//                      first_row by a 64-bit atomicMin -- the key in the high half makes that a minimum over rows.  A row that READS
//                      a first_row at or below itself issues no atomic (the word only falls), so a hot key costs loads, not atomics.
//   sp_first_kernel    per tile: every row looks its key up again (read only) and keeps the key's first row; the tile's first rows
//                      (first[r] == r) are counted by ballots.
//   (scan)             the tiles' counts -> the first rows before each tile, their total = n_keys.
//   sp_ids_kernel      per tile: a first row's id is the tile's base plus the first rows before it in the tile (ballots, carried from
//                      chunk to chunk): keys[id] = key, rid[row] = id.
//   -- the host reads n_keys, holds it against keys_cap, and knows how many 8-bit passes the ids need --
//   sp_rid_kernel      a row per thread: a row that is not its key's first takes the first's id (reads at first rows, writes at the others).
//   per pass p, digit = (id >> 8p) & 255, LEAST significant first:
//   sp_hist_kernel     per tile: the rows of each digit, counted by matching lanes (one ballot per bit of the digit); digit-major in thist
//   (scan)             thist over (digit, tile) -> where the tile's rows of the digit go
//   sp_scatter_kernel  per tile, STABLE: a row goes to the tile's base of its digit plus the rows of that digit before it in the tile --
//                      the lanes below it in its chunk (ballots) and what the chunks before left in LDS.  (id, row) move together, 8 B a
//                      row a pass; pass 0 reads rid and the row's own number.
//   sp_gather_kernel   split row j takes the event of its original row into the regions the pairing kernels read; where the id changes
//                      a key's rows begin: ev_off, without any count; row_of if asked for.
// THE SCAN is chunked: sp_sum_kernel (a block of 1,024 words per workgroup: its sum), sp_top_kernel (ONE workgroup over the block
// sums, 256 a step with a carried base -- n / 4,096 of them for thist), sp_apply_kernel (every block scanned in place from its base).
// Ballots, the barriers and index / thread go through wave_env.h / wave_env_wg.h; the 64-bit atomics on the table are plain HIP, which
// tests/emu/emu_split.cpp states for the host emulator -- these very kernels run there in a permuted order of workgroups.
// SPLIT_MUTATION (1: ids by key VALUE instead of first appearance; 2: the scatter ranks within the tile only; 3: sp_top_kernel
// stores a block's base without what its earlier steps of 256 carried; 4: the probe of the table stays in the last slot instead of
// going on in slot 0) exists for tests/test_keyed_events_emu.py alone, which must see all four.
#pragma once
#include "wave_env_wg.h"
#include "split_plan.h"
#include "wg_scan.h"

namespace {

using sp::SpArgs;

#if defined(TBC_EMU)
static inline unsigned long long sp_ld64(const unsigned long long* p) { return *p; }
#else
// (agent scope: never a stale line of this compute unit's L1 -- a stale word would only cost an atomic, a line that is never
// refreshed would cost the probe its end)
__device__ __forceinline__ unsigned long long sp_ld64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

__device__ __forceinline__ unsigned long long sp_mask(const SpArgs& A) { return (1ull << A.bits) - 1ull; }

// the lanes that `act` and hold this lane's 8-bit `digit`: one ballot per bit
__device__ __forceinline__ unsigned long long sp_same_digit(bool act, uint32_t digit) {
  unsigned long long same = wv::ballot(act);
  for (uint32_t bit = 0; bit < 8u; bit++) {
    const bool one = ((digit >> bit) & 1u) != 0u;
    const unsigned long long m = wv::ballot(act && one);
    same &= one ? m : ~m;
  }
  return same;
}

__global__ __launch_bounds__(256) void sp_insert_kernel(SpArgs A) {
  const unsigned long long mask = sp_mask(A);
  for (unsigned long long r = (unsigned long long)wv::wg_index() * 256u + wv::wg_thread(); r < A.n; r += (unsigned long long)A.grid * 256u) {
    const uint32_t k = (uint32_t)A.key[r];
    const unsigned long long mine = ((unsigned long long)k << 32) | r;
    unsigned long long idx = sp::table_hash(k, A.bits);
    for (unsigned long long t = 0; t <= mask; t++, idx = (idx + 1ull) & mask) {          // (2n slots or more: an empty one comes)
#if defined(SPLIT_MUTATION) && SPLIT_MUTATION == 4
      if (t != 0ull && idx == 0ull) idx = mask;                                        // (the step behind the last slot stays in it)
#endif
      unsigned long long w = sp_ld64(&A.table[idx]);
      if (w == sp::kEmpty) {
        w = atomicCAS(&A.table[idx], sp::kEmpty, mine);
        if (w == sp::kEmpty) break;                                                    // claimed: the first row so far is this one
      }
      if ((uint32_t)(w >> 32) != k) continue;                                          // another key's
      if ((uint32_t)w > (uint32_t)r) atomicMin(&A.table[idx], mine);
      break;
    }
  }
}

// the first row of `k` (every key of the history is in the table)
__device__ __forceinline__ uint32_t sp_first_row(const SpArgs& A, uint32_t k) {
  const unsigned long long mask = sp_mask(A);
  unsigned long long idx = sp::table_hash(k, A.bits);
  for (unsigned long long t = 0; t <= mask; t++, idx = (idx + 1ull) & mask) {
#if defined(SPLIT_MUTATION) && SPLIT_MUTATION == 4
    if (t != 0ull && idx == 0ull) idx = mask;
#endif
    const unsigned long long w = A.table[idx];
    if ((uint32_t)(w >> 32) == k && w != sp::kEmpty) return (uint32_t)w;
    if (w == sp::kEmpty) break;                                                        // (never)
  }
  return 0xFFFFFFFFu;
}

__global__ __launch_bounds__(64) void sp_first_kernel(SpArgs A) {
  const uint32_t lane = wv::wg_thread();
  for (uint32_t tile = wv::wg_index(); tile < A.n_tiles; tile += A.grid) {
    uint32_t cnt = 0;
    for (uint32_t c = 0; c < sp::kTile / 64u; c++) {
      const unsigned long long r = (unsigned long long)tile * sp::kTile + c * 64u + lane;
      bool is_first = false;
      if (r < A.n) {
        const uint32_t fr = sp_first_row(A, (uint32_t)A.key[r]);
        A.first[r] = fr;
        is_first = fr == (uint32_t)r;
      }
      cnt += (uint32_t)__popcll(wv::ballot(is_first));
    }
    if (lane == 0u) A.tile_cnt[tile] = cnt;
  }
}

__global__ __launch_bounds__(64) void sp_ids_kernel(SpArgs A) {
  const uint32_t lane = wv::wg_thread();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t tile = wv::wg_index(); tile < A.n_tiles; tile += A.grid) {
    uint32_t before = A.tile_cnt[tile];                                                // (scanned: the first rows of the tiles before)
    for (uint32_t c = 0; c < sp::kTile / 64u; c++) {
      const unsigned long long r = (unsigned long long)tile * sp::kTile + c * 64u + lane;
      const bool is_first = r < A.n && A.first[r] == (uint32_t)r;
      const unsigned long long fm = wv::ballot(is_first);
      if (is_first) {
        uint32_t id = before + (uint32_t)__popcll(fm & below);
#if defined(SPLIT_MUTATION) && SPLIT_MUTATION == 1
        id = 0;
        for (unsigned long long s = 0; s <= sp_mask(A); s++)
          if (A.table[s] != sp::kEmpty && (int32_t)(A.table[s] >> 32) < A.key[r]) id++;
#endif
        A.rid[r] = id;
        A.keys[id] = A.key[r];
      }
      before += (uint32_t)__popcll(fm);
    }
  }
}

__global__ __launch_bounds__(256) void sp_rid_kernel(SpArgs A) {
  for (unsigned long long r = (unsigned long long)wv::wg_index() * 256u + wv::wg_thread(); r < A.n; r += (unsigned long long)A.grid * 256u) {
    const uint32_t fr = A.first[r];
    if (fr != (uint32_t)r && fr < A.n) A.rid[r] = A.rid[fr];                           // (reads at first rows only, writes at the others only)
  }
}

// the (id, row) pairs a pass reads and writes: pass 0 reads rid and the row's own number, then the two buffers take turns
__device__ __forceinline__ const uint32_t* sp_src_id(const SpArgs& A, uint32_t pass) { return pass == 0u ? A.rid : ((pass & 1u) ? A.id_b : A.id_a); }
__device__ __forceinline__ const uint32_t* sp_src_row(const SpArgs& A, uint32_t pass) { return pass == 0u ? nullptr : ((pass & 1u) ? A.row_b : A.row_a); }

__global__ __launch_bounds__(64) void sp_hist_kernel(SpArgs A) {
  __shared__ uint32_t s_h[256];
  const uint32_t lane = wv::wg_thread();
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t* ids = sp_src_id(A, A.pass);
  const uint32_t shift = 8u * A.pass;
  for (uint32_t tile = wv::wg_index(); tile < A.n_tiles; tile += A.grid) {
    for (uint32_t i = lane; i < 256u; i += 64u) s_h[i] = 0u;
    wv::barrier();
    for (uint32_t c = 0; c < sp::kTile / 64u; c++) {
      const unsigned long long j = (unsigned long long)tile * sp::kTile + c * 64u + lane;
      const bool act = j < A.n;
      const uint32_t d = act ? (ids[j] >> shift) & 255u : 0u;
      const unsigned long long same = sp_same_digit(act, d);
      if (act && (same & below) == 0ull) s_h[d] += (uint32_t)__popcll(same);           // (one lane a digit)
      wv::barrier();
    }
    for (uint32_t i = lane; i < 256u; i += 64u) A.thist[(size_t)i * A.n_tiles + tile] = s_h[i];
    wv::barrier();
  }
}

__global__ __launch_bounds__(64) void sp_scatter_kernel(SpArgs A) {
  __shared__ uint32_t s_at[256];
  const uint32_t lane = wv::wg_thread();
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t* ids = sp_src_id(A, A.pass);
  const uint32_t* rows = sp_src_row(A, A.pass);
  uint32_t* out_id = (A.pass & 1u) ? A.id_a : A.id_b;
  uint32_t* out_row = (A.pass & 1u) ? A.row_a : A.row_b;
  const uint32_t shift = 8u * A.pass;
  for (uint32_t tile = wv::wg_index(); tile < A.n_tiles; tile += A.grid) {
#if defined(SPLIT_MUTATION) && SPLIT_MUTATION == 2
    for (uint32_t i = lane; i < 256u; i += 64u) s_at[i] = A.thist[(size_t)i * A.n_tiles];
#else
    for (uint32_t i = lane; i < 256u; i += 64u) s_at[i] = A.thist[(size_t)i * A.n_tiles + tile];
#endif
    wv::barrier();
    for (uint32_t c = 0; c < sp::kTile / 64u; c++) {
      const unsigned long long j = (unsigned long long)tile * sp::kTile + c * 64u + lane;
      const bool act = j < A.n;
      const uint32_t id = act ? ids[j] : 0u;
      const uint32_t d = (id >> shift) & 255u;
      const unsigned long long same = sp_same_digit(act, d);
      const uint32_t to = act ? s_at[d] + (uint32_t)__popcll(same & below) : 0u;
      wv::barrier();                                                                   // (every lane has read s_at)
      if (act) {
        if (to < A.n) { out_id[to] = id; out_row[to] = rows ? rows[j] : (uint32_t)j; } // (thist adds up to n: always)
        if ((same >> lane) <= 1ull) s_at[d] += (uint32_t)__popcll(same);               // the digit's last lane leaves where the next chunk goes on
      }
      wv::barrier();
    }
  }
}

__global__ __launch_bounds__(256) void sp_gather_kernel(SpArgs A) {
  const uint32_t* ids = sp_src_id(A, A.n_pass);
  const uint32_t* rows = sp_src_row(A, A.n_pass);
  for (unsigned long long j = (unsigned long long)wv::wg_index() * 256u + wv::wg_thread(); j < A.n; j += (unsigned long long)A.grid * 256u) {
    const uint32_t r = rows ? rows[j] : (uint32_t)j;
    const uint32_t id = ids[j];
    if (r >= A.n || id >= A.n_keys) continue;                                          // (a permutation of the rows, ids below n_keys: never)
    if (j == 0ull || ids[j - 1ull] != id) A.ev_off[id] = j;
    if (j + 1ull == A.n) A.ev_off[A.n_keys] = A.n;
    if (A.r_word) A.g_word[j] = A.r_word[r];
    else { A.g_type[j] = A.r_type[r]; A.g_f[j] = A.r_f[r]; A.g_a[j] = A.r_a[r]; A.g_b[j] = A.r_b[r]; }
    A.g_process[j] = A.r_process[r];
    if (A.row_of) A.row_of[j] = r;
  }
}

// ---- the chunked scan of `m` words in place (exclusive), the total to *total
struct SpScan { uint32_t* buf; uint32_t* sums; uint32_t* total; uint32_t m, n_blocks, grid, pad; };

__global__ __launch_bounds__(256) void sp_sum_kernel(SpScan S) {
  __shared__ uint32_t s_scan[256];
  const uint32_t t = wv::wg_thread();
  for (uint32_t b = wv::wg_index(); b < S.n_blocks; b += S.grid) {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; k++) {
      const unsigned long long i = (unsigned long long)b * sp::kScanBlock + t * 4u + k;
      if (i < S.m) v += S.buf[i];
    }
    uint32_t total;
    (void)wg_scan_excl(v, s_scan, t, 0u, total, [](uint32_t a, uint32_t c) { return a + c; });
    if (t == 0u) S.sums[b] = total;
  }
}

__global__ __launch_bounds__(256) void sp_top_kernel(SpScan S) {                        // (one workgroup)
  __shared__ uint32_t s_scan[256];
  const uint32_t t = wv::wg_thread();
  uint32_t base = 0;
  for (uint32_t b0 = 0; b0 < S.n_blocks; b0 += 256u) {
    const uint32_t b = b0 + t;
    const uint32_t v = b < S.n_blocks ? S.sums[b] : 0u;
    uint32_t total;
    const uint32_t ex = wg_scan_excl(v, s_scan, t, 0u, total, [](uint32_t a, uint32_t c) { return a + c; });
    if (b < S.n_blocks) S.sums[b] = base + ex;
#if defined(SPLIT_MUTATION) && SPLIT_MUTATION == 3
    if (b < S.n_blocks) S.sums[b] = ex;
#endif
    base += total;
  }
  if (t == 0u) *S.total = base;
}

__global__ __launch_bounds__(256) void sp_apply_kernel(SpScan S) {
  __shared__ uint32_t s_scan[256];
  const uint32_t t = wv::wg_thread();
  for (uint32_t b = wv::wg_index(); b < S.n_blocks; b += S.grid) {
    uint32_t v[4], sum = 0;
    for (uint32_t k = 0; k < 4u; k++) {
      const unsigned long long i = (unsigned long long)b * sp::kScanBlock + t * 4u + k;
      v[k] = i < S.m ? S.buf[i] : 0u;
      sum += v[k];
    }
    uint32_t total;
    uint32_t at = S.sums[b] + wg_scan_excl(sum, s_scan, t, 0u, total, [](uint32_t a, uint32_t c) { return a + c; });
    for (uint32_t k = 0; k < 4u; k++) {
      const unsigned long long i = (unsigned long long)b * sp::kScanBlock + t * 4u + k;
      if (i < S.m) S.buf[i] = at;
      at += v[k];
    }
  }
}

}  // namespace

namespace sp {

// The launches of the call in order, over a launcher (oneshot_plan.h): THE statement of them -- the library runs them over a stream
// (split.hip), the tests over the emulator.
template <class Launcher>
void scan_sequence(Launcher& go, const SpArgs& A, uint32_t* buf, uint32_t m, uint32_t* total) {
  SpScan S{};
  S.buf = buf; S.sums = A.sums; S.total = total; S.m = m; S.n_blocks = (m + kScanBlock - 1u) / kScanBlock;
  S.grid = go.grid(S.n_blocks, 4096u);
  go.launch(sp_sum_kernel, S.grid, 256u, S);
  const uint32_t blocks = S.grid;
  S.grid = go.grid(1u, 1u);
  go.launch(sp_top_kernel, S.grid, 256u, S);
  S.grid = blocks;
  go.launch(sp_apply_kernel, S.grid, 256u, S);
}

// the keys and their ids by first appearance; acc->n_keys  (n rows, n > 0)
template <class Launcher>
void keys_sequence(Launcher& go, SpArgs A) {
  const uint32_t rows = go.grid(((uint64_t)A.n + 255u) / 256u, 4096u), tiles = go.grid(A.n_tiles, 8192u);
  A.grid = rows;
  go.launch(sp_insert_kernel, A.grid, 256u, A);
  A.grid = tiles;
  go.launch(sp_first_kernel, A.grid, 64u, A);
  scan_sequence(go, A, A.tile_cnt, A.n_tiles, &A.acc->n_keys);
  go.launch(sp_ids_kernel, A.grid, 64u, A);
}

// (the host has read n_keys: A.n_keys, A.n_pass) every row's id, the stable sort of the rows on it, the gather
template <class Launcher>
void sort_sequence(Launcher& go, SpArgs A) {
  const uint32_t rows = go.grid(((uint64_t)A.n + 255u) / 256u, 4096u), tiles = go.grid(A.n_tiles, 8192u);
  A.grid = rows;
  go.launch(sp_rid_kernel, A.grid, 256u, A);
  for (A.pass = 0; A.pass < A.n_pass; A.pass++) {
    A.grid = tiles;
    go.launch(sp_hist_kernel, A.grid, 64u, A);
    scan_sequence(go, A, A.thist, 256u * A.n_tiles, &A.acc->scan_total);
    go.launch(sp_scatter_kernel, A.grid, 64u, A);
  }
  A.grid = rows;
  go.launch(sp_gather_kernel, A.grid, 256u, A);
}

}  // namespace sp
