// set_full_plan.h -- the plan of a set-full object: the plan TABLE, what every kernel of set_full.hip (the scan), set_full_results.h and
// set_full_encode.h finds its key with, and the PLANNER, sf_make_layout: from the keys' sizes and the source of the matrix to that table,
// the first tile of every grid and the place of every array in the object's one arena.  The planner is plain C++ with no HIP call in it:
// set_full_host.hip builds every object from it, and the emulator programs (tests/emu/emu_setfull_encode.cpp, emu_setfull_results.cpp,
// setfull_plan.cpp) call this very function, so the plan has one statement.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "set_full_encode_plan.h"          // sfenc::table_slots: the capacity of a key's element table (Ops)
#include "enc_table.h"                     // kNoneU, SfEncSlot and the probe of an element table (shared with the ledger checkers)

namespace {

constexpr uint32_t kSetFullRows = 2048;      // rows per chunk at most (their metadata is staged in LDS)
constexpr uint32_t kWordCounters = 256;      // the words-loaded statistic: a wavefront adds to counter (its workgroup mod 256), 128 B apart -- thousands of
                                             // atomics on ONE address queue up in one L2 channel; the host adds the counters up
constexpr size_t kCounterBytes = (size_t)kWordCounters * 128;
constexpr uint32_t kSelTile = 2048;          // the results' passes: elements per workgroup of 256 (a wavefront takes 512 consecutive ones, 64 a step)

// ---- the plan: every object holds n_keys keys (tbc_setfull_create / _create_rows: one) in ONE arena, and each pass is ONE launch over
// the tiles of all keys.  The plan table (built on the host at create) gives each key its arrays' offsets, its chunking and the first tile
// of each grid; a workgroup finds its key by a binary search over those first tiles (uniform across the workgroup: scalar loads) and
// then works on that key alone.  Each key's pitch is a multiple of four words, so every 16 B load and store of the scan is aligned; the
// bits at or above a key's E never count (the kernels mask them, and the padding words of a row are zeros).
struct SfKeyPlan {                 // one key (device table; offsets in 32-bit words)
  uint32_t E, R, WPR, PITCH, rows_per_chunk, chunks, elem_base, row_base;
  uint32_t pmax_off, any_gy;
  unsigned long long m_off, sum_off;
};
enum { kFirstRows = 0, kFirstPrefix, kFirstAny, kFirstResolve, kFirstSelect, kFirsts };   // first[g * (n_keys + 1) + k]: key k's first tile in grid g
                                                                                         // (kFirstSelect: the results' passes, set_full_results.h)

// tbc_setfull_keys_create_ops: a key's open-addressing table of element values (set_full_encode.h)
struct SfEncKey { unsigned long long tab_off; uint32_t mask, pad; };         // the key's table: slots tab_off .. tab_off + mask (E = 0: none)

#if defined(__HIPCC__) || defined(TBC_EMU)
// the last key whose first tile (row) is <= b: keys with no tile share their successor's first and are never picked for a tile of theirs
__device__ __forceinline__ uint32_t sf_find_key(const uint32_t* __restrict__ first, uint32_t n_keys, uint32_t b) {
  uint32_t lo = 0, hi = n_keys;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (first[mid] <= b) lo = mid; else hi = mid; }
  return lo;
}
#endif

// ---- the planner (host).  Where the membership matrix comes from: the caller's dense rows (tbc_setfull_create), the reads' compact form
// top / exc_off / exc (tbc_setfull_create_rows, tbc_setfull_keys_create), or the reads' raw values (tbc_setfull_keys_create_ops)
enum class SfSource { Dense, Rows, Ops };

// a cursor over an arena: every region starts on a multiple of 256 B (a region of no bytes takes none and shares its successor's start)
struct SfRegion { size_t at = 0, bytes = 0; };
struct SfCursor { size_t at = 0; SfRegion take(size_t bytes) { const SfRegion r{at, bytes}; at += (bytes + 255) & ~(size_t)255; return r; } };

// The object's arena, in order (round 6: fourteen hipMalloc and as many hipFree -- each of which waits for the device -- were most of a
// caller's 5 ms around a 0.16 ms scan; the reference checks one history per call site, set_full.clj:157, so create + run + destroy IS its
// time to verdict): what the host makes (the head: ONE image, one copy), the caller's arrays, what the device makes, and -- Ops only -- the
// element values, the rows' value slices and what starts as zeros, side by side.  A region its source does not use has no bytes.
struct SfArena {
  SfRegion plan, first, pmax, enc;                                            // the head (pmax: the chunks' greatest prefixes, then their least)
  SfRegion add_invoke, add_ok, read_invoke, read_ok, top, exc_off, exc;       // the caller's arrays (top, exc_off, exc: Rows)
  SfRegion M, P, any, out, words;                                             // any: any_p | any_a; out: known | last_present | last_absent
  SfRegion element, val_lo, val_hi;                                           // Ops
  SfRegion slots, row_flag, key_flag, unknown, repeats, cnt, dup_max, dup_count;      // Ops: zeroed before the encoding kernels
  size_t bytes = 0;
  size_t head_bytes() const { return add_invoke.at; }
  size_t enc_zero_bytes() const { return bytes - slots.at; }
};

struct SfLayout {
  uint32_t n_keys = 0, sumE = 0, sumR = 0;
  std::vector<SfKeyPlan> plan;               // [n_keys]
  std::vector<uint32_t> first;               // [kFirsts][n_keys + 1]
  std::vector<SfEncKey> enc_keys;            // [n_keys], Ops only
  uint64_t tiles[kFirsts] = {};              // every grid's total ([kFirstRows]: the reads)
  uint64_t m_words = 0, sum_words = 0, pmax_words = 0, tab_slots = 0, bytes_matrix = 0;
  SfArena arena;
  bool fits() const { return !(pmax_words >= 0xFFFFFFFFull || tiles[kFirstAny] >= 0x7FFFFFFFull || tiles[kFirstResolve] >= 0x7FFFFFFFull); }
};

// enough chunks to fill the GPU with wavefronts that each stream a good stretch of rows; short chunks: what pass 2 walks again is one chunk
inline uint32_t sf_chunks(uint32_t WPR, uint32_t R) {
  const uint32_t col_blocks = std::max(1u, (WPR + 255) / 256);
  uint32_t chunks = std::max(1u, std::min(256u, 8192u / col_blocks));
  while (chunks > 1 && R / chunks < 64) chunks >>= 1;
  while ((R + chunks - 1) / chunks > kSetFullRows) chunks <<= 1;
  return chunks;
}

// Per key its chunking (a key of a few reads is one chunk) and its place in the arena's regions; per grid the first tile of every key; then
// the arena.  words_per_row: the caller's (Dense; it only counts into bytes_matrix); n_exceptions: exc_off[sum of reads] (Rows).  The sums
// of elements and of reads are below 2^32 - 1 (the entry points refuse more).
inline SfLayout sf_make_layout(uint32_t n, const uint32_t* n_elements, const uint32_t* n_reads, SfSource source, uint32_t words_per_row, uint64_t n_exceptions) {
  SfLayout L;
  const bool ops = source == SfSource::Ops, rows = source == SfSource::Rows;
  L.n_keys = n; L.plan.assign(n, SfKeyPlan{}); L.first.assign((size_t)kFirsts * (n + 1), 0u); L.enc_keys.assign(ops ? n : 0u, SfEncKey{});
  const auto up = [](uint64_t x, uint64_t a) { return (x + a - 1) / a * a; };
  uint64_t* const tiles = L.tiles;
  uint32_t eb = 0, rb = 0;
  for (uint32_t k = 0; k < n; k++) {
    SfKeyPlan& p = L.plan[k];
    p.E = n_elements[k]; p.R = n_reads[k]; p.elem_base = eb; p.row_base = rb;
    // (PITCH: the words between two rows in device memory.  A pitch padded off the power of two was measured -- 16 .. 1,088 words: the
    // same scan within 3 % either way, profiles/r06_setfull_pad_scan.txt -- so it is the words of a row, rounded up to four)
    p.WPR = (p.E + 31u) / 32u; p.PITCH = (p.WPR + 3u) / 4u * 4u;
    const bool scan = p.E && p.R;
    p.chunks = scan ? sf_chunks(p.WPR, p.R) : 1u; p.rows_per_chunk = std::max(1u, (p.R + p.chunks - 1) / p.chunks);
    p.any_gy = (p.PITCH / 4u + 255u) / 256u;
    L.m_words = up(L.m_words, 64); p.m_off = L.m_words; L.m_words += (uint64_t)p.R * p.PITCH;
    L.sum_words = up(L.sum_words, 64); p.sum_off = L.sum_words; L.sum_words += scan ? (uint64_t)p.chunks * p.PITCH : 0;
    p.pmax_off = (uint32_t)L.pmax_words; L.pmax_words += 2ull * p.chunks;
    const uint32_t nb = (p.WPR + 3u) / 4u;        // resolve: every key that has elements (one without reads: "nothing seen" is written there)
    L.first[kFirstRows * (n + 1) + k] = rb;
    L.first[kFirstPrefix * (n + 1) + k] = (uint32_t)tiles[kFirstPrefix]; tiles[kFirstPrefix] += scan ? (p.R + 255u) / 256u : 0u;
    L.first[kFirstAny * (n + 1) + k] = (uint32_t)tiles[kFirstAny]; tiles[kFirstAny] += scan ? (uint64_t)p.chunks * p.any_gy : 0u;
    // (a key of a multiple of eight resolve workgroups starts on a multiple of eight: setfull_resolve_kernel's XCD-contiguous order)
    if (nb && nb % 8u == 0u) tiles[kFirstResolve] = up(tiles[kFirstResolve], 8);
    L.first[kFirstResolve * (n + 1) + k] = (uint32_t)tiles[kFirstResolve]; tiles[kFirstResolve] += nb;
    L.first[kFirstSelect * (n + 1) + k] = (uint32_t)tiles[kFirstSelect]; tiles[kFirstSelect] += (p.E + kSelTile - 1u) / kSelTile;
    L.bytes_matrix += (uint64_t)p.R * (source == SfSource::Dense ? words_per_row : p.WPR) * 4;
    if (ops) {
      const uint64_t cap = sfenc::table_slots(p.E);
      L.enc_keys[k].tab_off = L.tab_slots; L.enc_keys[k].mask = cap ? (uint32_t)(cap - 1u) : 0u;
      L.tab_slots += cap;
    }
    eb += p.E; rb += p.R;
  }
  L.sumE = eb; L.sumR = rb;
  tiles[kFirstRows] = rb;
  for (int g = 0; g < kFirsts; g++) L.first[(size_t)g * (n + 1) + n] = (uint32_t)tiles[g];
  const size_t sumE = eb, sumR = rb;
  SfArena& A = L.arena;
  SfCursor c;
  A.plan = c.take(sizeof(SfKeyPlan) * n); A.first = c.take(L.first.size() * 4); A.pmax = c.take(L.pmax_words * 4);
  A.enc = c.take(sizeof(SfEncKey) * L.enc_keys.size());
  A.add_invoke = c.take(sumE * 4); A.add_ok = c.take(sumE * 4); A.read_invoke = c.take(sumR * 4); A.read_ok = c.take(sumR * 4);
  A.top = c.take(rows ? sumR * 4 : 0); A.exc_off = c.take(rows ? (sumR + 1) * 8 : 0); A.exc = c.take(rows ? n_exceptions * 4 : 0);
  A.M = c.take(L.m_words * 4); A.P = c.take(sumR * 4); A.any = c.take(L.sum_words * 8);
  A.out = c.take(sumE * 12); A.words = c.take(kCounterBytes);
  A.element = c.take(ops ? sumE * 8 : 0); A.val_lo = c.take(ops ? sumR * 8 : 0); A.val_hi = c.take(ops ? sumR * 8 : 0);
  A.slots = c.take(L.tab_slots * sizeof(SfEncSlot)); A.row_flag = c.take(ops ? sumR : 0); A.key_flag = c.take(ops ? (size_t)n * 4 : 0);
  A.unknown = c.take(ops ? (size_t)n * 8 : 0); A.repeats = c.take(ops ? 4 : 0); A.cnt = c.take(ops ? sumE * 4 : 0);
  A.dup_max = c.take(ops ? sumE * 4 : 0); A.dup_count = c.take(ops ? (size_t)n * 4 : 0);
  A.bytes = c.at;
  return L;
}

// The greatest op index among each key's inputs (-1: none): what tbc_setfull_results holds a call's times against.  It reads the callers'
// arrays, so it is no part of the layout.  (add_invoke and read_invoke ascend: their last entries are their greatest; add_ok may be TBC_NO_OP)
inline std::vector<int64_t> sf_key_max(const SfLayout& L, const uint32_t* add_invoke, const uint32_t* add_ok, const uint32_t* read_invoke, const uint32_t* read_ok) {
  std::vector<int64_t> key_max(L.n_keys, -1);
  for (uint32_t k = 0; k < L.n_keys; k++) {
    const SfKeyPlan& p = L.plan[k];
    int64_t& mx = key_max[k];
    if (p.E) mx = std::max<int64_t>(mx, add_invoke[p.elem_base + p.E - 1u]);
    for (uint32_t e = 0; e < p.E; e++) if (add_ok[p.elem_base + e] != kNoneU) mx = std::max<int64_t>(mx, add_ok[p.elem_base + e]);
    if (p.R) mx = std::max<int64_t>(mx, read_invoke[p.row_base + p.R - 1u]);
    for (uint32_t r = 0; r < p.R; r++) mx = std::max<int64_t>(mx, read_ok[p.row_base + r]);
  }
  return key_max;
}

}  // namespace
