// split_plan.h -- the host plan of tbc_pair_keyed_events (ONE keyed event history split by key on the device, then paired per key;
// include/tbcheck.h): plain C++ with no HIP call in it.  split_host.hip runs every call through it, and so does the emulator program of
// the kernels (tests/emu/emu_split.cpp).
//
//   validate   the rules of tbc_keyed_events / tbc_split_out / tbc_pair_out that the kernels trust, O(1): nothing looks at a row
//   plan       ONE arena: the pairing's own (pair_plan.h, at the arena's start: keys_cap histories at most over n events, its event
//              regions filled by the gather instead of by copies) and behind it the split's regions -- the raw input as it came (12 B
//              a row packed, 18 B in columns), the key table, the scratch per row and per tile
//   steps      the call from the plan to the filled outputs over a call frame: the keys -- run.keys(A) --, their number read back and
//              held against keys_cap BEFORE the sort, the sort, the gather and the pairing in one section -- run.sort(A),
//              run.pair(PA) --, and pr::finish, the pairing call's own second half
// THE SPECIFICATION is columns.split_events in numpy (keys by first appearance, a stable split) followed by tbc_pair_events per key.
#pragma once
#include "pair_plan.h"

namespace sp {

constexpr uint32_t kTile = 1024u;                      // rows a tile: one wavefront walks it, 16 chunks of 64 (first rows, histogram, scatter)
constexpr uint32_t kScanBlock = 1024u;                 // words a block of the chunked scan: 256 threads, four words each
constexpr uint64_t kMaxRows = 0xFFFFFFFEull;           // (key = -1, row) never equals the empty word
constexpr unsigned long long kEmpty = ~0ull;           // a table slot nobody has claimed

// the key table: a power of two of slots at or above 2n (64 at least); a slot is key << 32 | first_row
inline uint32_t table_bits(uint64_t n) {
  uint32_t bits = 6;
  while ((1ull << bits) < 2u * n) bits++;
  return bits;
}
// the table's hash of a key (the kernel's; the tests make colliding keys with it): the top `bits` bits of a 64-bit product
constexpr uint64_t table_hash(uint32_t key, uint32_t bits) { return ((uint64_t)key * 0x9E3779B97F4A7C15ull) >> (64u - bits); }
// the 8-bit passes of the sort on ids 0 .. n_keys - 1 (one key: none)
inline uint32_t sort_passes(uint32_t n_keys) {
  uint32_t p = 0;
  for (uint64_t top = n_keys ? n_keys - 1u : 0u; top; top >>= 8) p++;
  return p;
}

// what the kernels add up, in device memory (zeroed)
struct SpAcc { uint32_t n_keys, scan_total; };

// what the kernels take (split_kernels.h), every pointer into the arena
struct SpArgs {
  SpAcc* acc;
  uint32_t n, grid, n_tiles, bits;                     // rows, the launch's workgroups, tiles of kTile rows, the table's size
  uint32_t n_keys, n_pass, pass, pad;                  // (known once the host has read acc) ; the pass a launch is of
  const int32_t* key;
  const uint32_t* r_word; const int32_t* r_process; const uint8_t* r_type; const uint8_t* r_f; const int32_t* r_a; const int32_t* r_b;   // the raw input
  unsigned long long* ev_off; uint32_t* g_word; int32_t* g_process; uint8_t* g_type; uint8_t* g_f; int32_t* g_a; int32_t* g_b;           // the pairing's
  unsigned long long* table;                           // [1 << bits]
  uint32_t* first;                                     // [n] the first row of the row's key
  uint32_t* rid;                                       // [n] the id of the row's key
  int32_t* keys;                                       // [n] (as many as there are keys)
  uint32_t* tile_cnt;                                  // [n_tiles] first rows in the tile; scanned: before the tile
  uint32_t* thist;                                     // [256 * n_tiles] digit-major: rows of digit d in tile t; scanned: where they go
  uint32_t* sums;                                      // the scan's block sums
  uint32_t *id_a, *row_a, *id_b, *row_b;               // [n] each: the sort's two buffers
  uint32_t* row_of;                                    // [n] the final order, written by the gather (null: not asked for)
};

// Every kernel of the call on `stream` (a hipStream_t); defined in split.hip
void launch_keys(void* stream, SpArgs A);
void launch_sort(void* stream, SpArgs A);

using oneshot::Region;

struct SpArena {
  Region acc;                                                                 // zeroed
  Region key, r_word, r_process, r_type, r_f, r_a, r_b;                       // copied in
  Region table;                                                               // 0xFF all over
  Region first, rid, keys, tile_cnt, thist, sums, id_a, row_a, id_b, row_b, row_of;
};

struct Plan {
  uint32_t n = 0, n_tiles = 0, bits = 0;
  bool packed = false;
  pr::Plan pair;                                       // its arena is the head of the call's
  SpArena arena;
  size_t bytes = 0;
};

inline tbc_status validate(const char* fn, const tbc_keyed_events* in, const tbc_split_out* split, const tbc_pair_out* out, std::string& err) {
  const auto say = [&](const char* what) { err = std::string(fn) + ": " + what; return TBC_ERR_INVALID_ARG; };
  if (!split->keys || !split->ev_off) return say("null argument (keys, ev_off)");
  if (pr::validate_out(fn, out, err) != TBC_OK) return TBC_ERR_INVALID_ARG;
  if ((uint64_t)in->n > kMaxRows) return say("more than 2^32 - 2 rows");
  if (in->n && (!in->key || !in->process)) return say("null argument (key, process)");
  if (in->n && !in->ev_word && (!in->type || !in->f || !in->a || !in->b)) return say("null argument (ev_word, or type, f, a, b)");
  return TBC_OK;
}

// the split's regions for P.n rows from `first` bytes on; P.bytes: where they end
inline void lay_out(Plan& P, size_t first, bool row_of) {
  SpArena& A = P.arena;
  oneshot::Cursor c;
  c.at = first;
  const size_t n = P.n, nt = P.n_tiles, words = 256u * nt;
  A.acc = c.take(sizeof(SpAcc));
  A.key = c.take(n * 4);
  A.r_word = c.take(P.packed ? n * 4 : 0); A.r_process = c.take(n * 4);
  A.r_type = c.take(P.packed ? 0 : n); A.r_f = c.take(P.packed ? 0 : n); A.r_a = c.take(P.packed ? 0 : n * 4); A.r_b = c.take(P.packed ? 0 : n * 4);
  A.table = c.take(n ? (size_t)8 << P.bits : 0);
  A.first = c.take(n * 4); A.rid = c.take(n * 4); A.keys = c.take(n * 4);
  A.tile_cnt = c.take(nt * 4); A.thist = c.take(words * 4); A.sums = c.take(((words + kScanBlock - 1u) / kScanBlock) * 4);
  A.id_a = c.take(n * 4); A.row_a = c.take(n * 4); A.id_b = c.take(n * 4); A.row_b = c.take(n * 4); A.row_of = c.take(row_of ? n * 4 : 0);
  P.bytes = c.at;
}

// (the input has passed `validate`)
inline void plan(const tbc_keyed_events* in, const tbc_split_out* split, const tbc_pair_out* out, Plan& P) {
  P = Plan{};
  const size_t n = in->n;
  P.n = in->n;
  P.packed = in->ev_word != nullptr;
  P.n_tiles = (uint32_t)((n + kTile - 1u) / kTile);
  P.bits = table_bits(n);
  pr::plan_sizes((uint32_t)std::min<uint64_t>(split->keys_cap, n), n, out ? std::min<uint64_t>(out->ops_cap, n) : 0u, P.packed, out, P.pair);
  lay_out(P, P.pair.arena.bytes, split->row_of != nullptr);                  // (a multiple of 256)
}

// A BATCH'S SPLIT ARENA (tbc_batch_map_keyed_events / tbc_batch_submit_keyed_events, batch_stream.hip): the split's regions alone, laid
// out once for the batch's events_cap -- packed input, row_of included -- in an allocation of their own beside the batch's event
// arena (pr::plan_batch), into whose input regions the gather writes.  A submit of n events uses the head of every region.
inline void plan_batch(uint64_t events_cap, Plan& P) {
  P = Plan{};
  P.n = (uint32_t)events_cap;
  P.packed = true;
  P.n_tiles = (uint32_t)((events_cap + kTile - 1u) / kTile);
  P.bits = table_bits(events_cap);
  lay_out(P, 0, true);
}

// the kernels' arguments over an arena at `base`
// (`pair_base`, L: the pairing's arena, where the gather writes)
inline SpArgs args(const Plan& P, char* base, char* pair_base, const pr::PrArena& L) {
  const SpArena& S = P.arena;
  const auto at = [&](const Region& r) { return base + r.at; };
  const auto pat = [&](const Region& r) { return pair_base + r.at; };
  SpArgs A{};
  A.acc = (SpAcc*)at(S.acc);
  A.n = P.n; A.n_tiles = P.n_tiles; A.bits = P.bits;
  A.key = (const int32_t*)at(S.key);
  A.r_word = P.packed ? (const uint32_t*)at(S.r_word) : nullptr; A.r_process = (const int32_t*)at(S.r_process);
  A.r_type = (const uint8_t*)at(S.r_type); A.r_f = (const uint8_t*)at(S.r_f); A.r_a = (const int32_t*)at(S.r_a); A.r_b = (const int32_t*)at(S.r_b);
  A.ev_off = (unsigned long long*)pat(L.ev_off); A.g_word = (uint32_t*)pat(L.ev_word); A.g_process = (int32_t*)pat(L.process);
  A.g_type = (uint8_t*)pat(L.type); A.g_f = (uint8_t*)pat(L.f); A.g_a = (int32_t*)pat(L.a); A.g_b = (int32_t*)pat(L.b);
  A.table = (unsigned long long*)at(S.table);
  A.first = (uint32_t*)at(S.first); A.rid = (uint32_t*)at(S.rid); A.keys = (int32_t*)at(S.keys);
  A.tile_cnt = (uint32_t*)at(S.tile_cnt); A.thist = (uint32_t*)at(S.thist); A.sums = (uint32_t*)at(S.sums);
  A.id_a = (uint32_t*)at(S.id_a); A.row_a = (uint32_t*)at(S.row_a); A.id_b = (uint32_t*)at(S.id_b); A.row_b = (uint32_t*)at(S.row_b);
  A.row_of = (uint32_t*)at(S.row_of);
  return A;
}

inline SpArgs args(const Plan& P, char* base) { return args(P, base, base, P.pair.arena); }
// a submit of n events (n <= the batch's events_cap) in a batch's split arena at `base`, gathering into its event arena `L` at `pair_base`
inline SpArgs args_batch(const Plan& P, uint32_t n, char* base, char* pair_base, const pr::PrArena& L) {
  SpArgs A = args(P, base, pair_base, L);
  A.n = n; A.n_tiles = (n + kTile - 1u) / kTile; A.bits = table_bits(n);
  return A;
}

// The call from a finished plan to the filled `split` and `out` (null: split only), over an open frame (oneshot_plan.h, "the frame
// interface").  The raw columns go straight to their regions; the keys, their ids by first appearance -- run.keys(A) --; the number
// of keys is read back and held against keys_cap BEFORE a row moves; then the sort, the gather into the pairing's regions and the
// pairing itself in one section -- run.sort(A), run.pair(PA) -- and the pairing call's own second half (pr::finish: the total held
// against ops_cap before an op is written).  The split goes to the caller last: a call that is refused has written nothing.
template <class Frame, class Run>
tbc_status steps(Frame& C, Run&& run, const char* fn, const tbc_keyed_events* in, const Plan& P, tbc_split_out* split, tbc_pair_out* out) {
  const SpArena& S = P.arena;
  const pr::PrArena& L = P.pair.arena;
  SpArgs A = args(P, C.base());
  const tbc_pair_out none{};
  pr::PrArgs PA = pr::args(P.pair, out ? out : &none, C.base());
  C.fill(S.acc, 0, S.acc.bytes);
  C.fill(L.acc, 0, L.acc.bytes);
  if (P.n) {
    C.put(S.key, in->key);
    if (P.packed) { C.put(S.r_word, in->ev_word); C.put(S.r_process, in->process); }
    else { C.put(S.r_type, in->type); C.put(S.r_process, in->process); C.put(S.r_f, in->f); C.put(S.r_a, in->a); C.put(S.r_b, in->b); }
    C.fill(S.table, 0xFF, S.table.bytes);
    C.timed([&] { run.keys(A); });
  }
  SpAcc acc{};
  C.get(&acc, S.acc);
  if (C.sync() != TBC_OK) return C.status;
  if (acc.n_keys > split->keys_cap) return C.fail(TBC_ERR_INVALID_ARG, "%s: %u distinct keys, keys_cap is %u", fn, acc.n_keys, split->keys_cap);
  A.n_keys = acc.n_keys; A.n_pass = sort_passes(acc.n_keys);
  if (!split->row_of) A.row_of = nullptr;
  PA.n_hist = acc.n_keys;
  if (!P.n) C.fill(L.ev_off, 0, 8);
  C.fill(L.comp_of, 0xFF, L.comp_of.bytes);
  C.timed([&] {
    if (P.n) run.sort(A);
    if (out) run.pair(PA);
  });
  if (out && pr::finish(C, run, fn, L, PA, out) != TBC_OK) return C.status;
  C.get(split->keys, S.keys, (size_t)acc.n_keys * 4); C.get(split->ev_off, L.ev_off, ((size_t)acc.n_keys + 1) * 8);
  C.get(split->row_of, S.row_of, split->row_of ? (size_t)P.n * 4 : 0);
  if (C.sync() != TBC_OK) return C.status;
  split->n_keys = acc.n_keys;
  return TBC_OK;
}

}  // namespace sp
