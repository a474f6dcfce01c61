// open_walk_impl.h -- K1b's front walk with LANE = FRONT (gfx950; mask_words == 1, i.e. at most 64 process slots).
//
// What it leaves in HBM is what pack_open.hip's open_walk_kernel<1> + open_dprod_kernel + front_meta_kernel leave, word for
// word (lst / twn / rdm rows or front records / look; the definitions are in that file's header and tbc_internal.h).  How it
// gets there is turned round.  open_walk_kernel gives a wavefront 64 fronts and walks them ONE AFTER THE OTHER with lane =
// process slot: every front costs ~140 vector instructions, and of the 64 lanes each of them drives, the six that hold an open
// call do something (rocprofv3, round 3: SQ_ACTIVE_INST_VALU 95 % of the kernel's 70 ms per 32,768 histories -- the walk is
// bound by vector issue and nothing else).  Here a wavefront still owns 64 consecutive fronts, but lane = front, and the loop
// runs over the CANDIDATES: the calls open at some front of the chunk (plus, for the lookahead's producer distance, those that
// completed within the seven ranks before it).  A process has one call open at a time, so all but the last candidate of a
// slot complete inside ranks F_lo - 7 .. F_hi - 1: at most 71 completions + one call per slot = 135 candidates, ~75 at six
// calls in flight.  The candidates sit in LDS in slot order (32 B each, with what the loop asks of them worked out once, as
// flag bits); iteration t broadcasts candidate t to the 64 lanes and each lane decides for ITS front whether the call is open
// there (inv <= F <= ret), appends it to its front's list, ors its slot into its read row / lookahead mask, keeps the nearest
// producer.  Everything that was per-front overhead -- list positions, record addresses, the lookahead word, the front
// record's windows -- is per lane, i.e. done for 64 fronts by one instruction.
//
// Twin masks (tbc_internal.h): entry (front F, call c) gets the slots of the calls open at F with c's effect that complete
// before c.  "Same effect, completes earlier, lifetimes overlap" does not depend on the front: with the candidates ALSO held one
// per lane (three register sets), one ballot per write / cas candidate finds its few static twins, and each of those costs the
// lanes one membership test.
//
// THE SPARSE FORM of phase C (rows of at most 8 entries, i.e. open_walk_fronts_kernel<8>).  The loop above asks NC x 64 times "is this
// call open at my front?" for the ~6 x 64 times the answer is yes.  The sparse form has no loop over the candidates with lane = front: a
// call is open at fronts inv .. ret, so with lane = candidate it toggles a bit ON at the first of them and OFF behind the last in a 64-entry
// array in LDS, and with lane = front an inclusive XOR scan over the lanes gives every front its set of open calls.  Three kinds of set:
// bit = place in list order (the fronts leave their sets in LDS and the list entries are stored with lane = ENTRY, 64 consecutive entries of
// the chunk a store instruction -- whole lines of lst / twn: an entry lane finds its front and takes the k-th set bit of the front's words,
// sparse_lists; a twin mask comes down a chain that links the calls of one effect by completion, phase B2), bit = process slot per read-row entry present (the scan is the row entry), bit =
// process slot per produced value some front needs (the scan is the producer mask).  The producer distance comes from byte counters of the
// invocation ranks, per produced value.  The tables it leaves are the dense loop's, word for word.
// What keeps the dense loop, decided per chunk by a uniform condition (`sparse` in walk_chunk):
//   * rows of more than 8 entries (open_walk_fronts_kernel<32>);
//   * a chunk of more than kSparseCand = 101 candidates: the form's round buffer lies over the end of the candidate table, so that a block
//     keeps its 20 KB of LDS and 64 registers (eight blocks a CU: at six the kernel gave back what the form saves), and a table that full
//     has no room for it.  At the bench's shape (6.4 calls in flight, ~75 candidates) no chunk comes near it.
//
// A wavefront of the kernel takes a RUN of kWalkRun consecutive chunks of one history (walk_run), one after the other: the first
// chunk finds each slot's first candidate by a binary search of the slot's records, the others carry the cursor on from the chunk
// before (phase A).  walk_wave is one chunk from nothing; both forms share the body, walk_chunk.
//
// walk_chunk is the setup of a chunk (struct Chunk: pointers and flags, all uniform) and one call per PHASE, each a function of its own
// with its comment above it:
//   A   fill_candidates     lane = slot: the slot's cursor (searched or carried), its candidates, the table in LDS
//   A2  list_places         lane = candidate: its place in list order (places_by_counting, else places_by_compare)
//   B   sparse_flags / dense_twin_keys      the candidates once more, one per lane, in registers
//   B2  link_twins          (sparse, twin masks) the chain of each effect's calls by completion
//   C   front_of            lane = front: the front's list position and the call completing there; then either
//       sparse_read_rows, sparse_producers, sparse_lists   -- rdm rows; look records; lst / twn entries -- (rounds of toggles: open_bits)
//       or dense_loop       the candidate loop, all three at once, the row in registers
//   D   compact_tail        words 6 and 7 of a compact front record
//
// The body is written against wave_env.h like the narrow search kernel, so tests/emu runs it on the CPU (lane-accurate
// emulator) and compares every word with tables built on the host from the definitions (tests/test_walk_emu.py: walk_wave;
// tests/test_walk_runs_emu.py: walk_run, where the emulated build also searches and counts a carried cursor that differs;
// tests/test_walk_sparse_emu.py: the sparse form, its schedule counts, three planted mutations of it, and the dense loop beside it).
#pragma once
#include "wave_env.h"
#include "tbc_internal.h"

namespace tbc {
namespace walk {

constexpr uint32_t kCandCap = 136;          // 71 completions (ranks F_lo - 7 .. F_hi - 1) + one more call per slot (64 slots), rounded up
constexpr uint32_t kCandWords = 8;          // inv_rank, ret_rank, opidx, f | slot << 8;  a, b, flags (below), effect key
constexpr uint32_t kAuxWords = 80;          // the scan of the per-slot counts; later the rank codes of the chunk + 6
constexpr uint32_t kKeyWords = 32, kKeyBits = 32 * kKeyWords;       // A2's map of the live candidates' keys and its prefix, over the same words
static_assert(2 * kKeyWords <= kAuxWords && kKeyWords == 32, "the map and its prefix fit the scratch; two rows of 16 lanes scan it");
constexpr uint32_t kCursorWords = 64 + 32;   // what a slot lane carries from a chunk of a run to the next (walk_run): where this chunk's candidates
//                                             ended (a word), and how many of them the next chunk still has (16 bits: eight at most, see phase A)
WV_HD constexpr uint32_t walk_lds_words() { return kCandCap * kCandWords + kAuxWords + kCursorWords; }
static_assert(4u * walk_lds_words() * sizeof(uint32_t) <= 20u * 1024u, "eight blocks of four wavefronts a CU");
// The sparse form's round buffer (see phase C): per front index an ON pair and an OFF pair of toggle words, then the byte counters of the
// invocation ranks F_lo - 7 .. F_lo + 63 (71 bytes; a front reads three words from its own).  It lies over the END of the candidate table:
// a chunk of more than kSparseCand candidates has no room for it and takes the dense loop.
constexpr uint32_t kTogWords = 64 * 4, kRankCntWords = 24;
constexpr uint32_t kSparseCand = kCandCap - (kTogWords + kRankCntWords) / kCandWords;
constexpr int kSparseSets = 2;               // ... so the form holds its candidates one per lane in two register sets, not three
static_assert(kSparseCand <= 64u * kSparseSets, "two sets of 64 candidates");
static_assert((kTogWords + kRankCntWords) % kCandWords == 0u && (kSparseCand * kCandWords) % 4u == 0u && kSparseCand >= 96u, "the toggle words of a front are 16 bytes, aligned");
// blocks of four wavefronts a CU the <8> kernel is compiled for (__launch_bounds__' second argument)
#ifndef TBC_WALK_BLOCKS
#define TBC_WALK_BLOCKS 8
#endif

// candidate word 6: what the loop does with the call, decided once when the table is filled
constexpr uint32_t kCList = 1u;             // live and in the fronts' lists (branch lists: not a read)
constexpr uint32_t kCTwin = 2u;             // ... and its entries carry a twin mask (a write / cas, twin masks wanted)
constexpr uint32_t kCRow = 4u;              // a live read whose value has a row entry: bits 4..8 = the entry
constexpr uint32_t kCLook = 8u;             // produces a register value (bits 24..31): lookahead mask, producer distance
//                                             bits 12..17 = the process slot

// m |= cond ? 1 << slot : 0 with a UNIFORM slot: one half of the mask, two vector instructions.  (wv::opaque keeps the branch
// a branch: left alone, the compiler computes both halves and selects.)
WV_DEV void or_slot(uint32_t& lo, uint32_t& hi, bool cond, uint32_t slot) {
  if (slot < 32u) lo = wv::opaque(lo | (cond ? (1u << slot) : 0u));
  else hi = wv::opaque(hi | (cond ? (1u << (slot - 32u)) : 0u));
}
// what "same effect" compares, in one word.  Twin masks are only built under the dominance rules, i.e. for register values
// 0 .. kMaxRuleValue (tbc_api.hip switches the rules off for anything else): f, a and -- for a cas -- b fit 2 + 15 + 15 bits
WV_DEV uint32_t effect_key(uint32_t f, int32_t a, int32_t b) {
  return (f & 3u) | (((uint32_t)a & 0x7FFFu) << 2) | ((f == TBC_F_CAS ? ((uint32_t)b & 0x7FFFu) : 0u) << 17);
}
static_assert(kMaxRuleValue < 0x7FFF && TBC_F_READ < 3 && TBC_F_WRITE < 3 && TBC_F_CAS < 3, "effect_key packs f and two rule values into a word, and no key has all bits set");
static_assert(kLookNone <= 0xFFu, "the produced value shares a word with the flags");

// the nine bits a compact front record keeps per rank (front_rank_code), from the completing call itself
WV_DEV uint32_t rank_code(uint32_t slot, uint32_t f, int32_t a, uint32_t vpad) {
  return front_rank_code(slot, f == TBC_F_READ ? (rdm_index(a, vpad) & 0xFFu) : 0xFFu);
}

// A front's open-read row lives in registers as u32x16 vectors (16 words = 8 entries each: entry v = words 2v, slots 0..31, and
// 2v + 1), the word to touch picked by a UNIFORM index: s_set_gpr_idx, one indexed move each way.  (Plain locals on purpose: as
// members of a struct the compiler moves them to scratch, and a chain of compares over an array made it copy the whole array.)
template <int Q>
WV_DEV void store_entries(const wv::u32x16& r, uint64_t* row, uint32_t n) {       // entries 8Q .. 8Q + 7 below n
  WV_UNROLL
  for (int v = 0; v < 8; v++) if ((uint32_t)(8 * Q + v) < n) row[8 * Q + v] = (uint64_t)r[2 * v] | ((uint64_t)r[2 * v + 1] << 32);
}

// A wavefront of the kernel owns a RUN of kWalkRun consecutive chunks of one history (walk_run below) and takes them one after the
// other; what it carries from a chunk to the next is, per slot lane, where this chunk's candidates ended and how many of them are the next
// chunk's too (LDS, kCursorWords) -- so only a run's first chunk searches (phase A).
#ifndef TBC_WALK_RUN
#define TBC_WALK_RUN 8
#endif
constexpr uint32_t kWalkRun = TBC_WALK_RUN;
static_assert(kWalkRun >= 1u, "a run has a chunk");
// wv::stat ids of an emulated run (tests/emu): chunks that searched, chunks that took the carried cursors, slot lanes whose carried
// cursor is not what the search finds
constexpr uint32_t kStatWalkSearch = 40, kStatWalkCarried = 41, kStatWalkCursorMiss = 42;
// ... chunks that took the sparse form of phase C / the dense loop; trips of the sparse form's emission loop (a wavefront's), per-lane
// steps through a static twin list, value rounds (rows, then lookahead), per-lane exact compares where the static twins are found
constexpr uint32_t kStatWalkSparse = 43, kStatWalkDense = 44, kStatWalkEmitTrips = 45, kStatWalkTwinSteps = 46, kStatWalkRounds = 47, kStatWalkTwinFind = 48;
constexpr uint32_t kStatWalkCands = 49;     // + 0 / 1 / 2: chunks of at most 64, of 65 .. kSparseCand, of more candidates
// what the WAVEFRONT runs of the two per-lane loops, i.e. the longest lane's steps: of B2's bucket walk (per pass and set), of the twin chain (per trip)
constexpr uint32_t kStatWalkFindWave = 52, kStatWalkChainWave = 53;
// the sparse form's stores with lane = entry (its emission trips are passes of 64 entries): list entries of the chunks, fronts whose off[] is not
// where the running sum of the counts puts them, entries that have no candidate (both zero unless a mutation is planted), entries whose place in
// list order is in the second set of 64
constexpr uint32_t kStatWalkEntries = 54, kStatWalkNotContiguous = 55, kStatWalkBadPlace = 56, kStatWalkSecondSet = 57;
constexpr uint32_t kStatWalkLstLines = 58;  // the 128-byte lines of lst the form's store instructions touch, summed over the instructions
#if defined(TBC_EMU)
// (emulated build) the largest n over the lanes, added to a count: one ballot per step of the longest lane
#define WV_STAT_WAVE_MAX(id, n) do { for (uint32_t k_ = 1u; wv::ballot((n) >= k_) != 0ull; k_++) if (lane == 0u) wv::stat((id), 1); } while (0)
// (emulated build) the different 128-byte lines one store instruction touches -- `on`: the lane stores, at byte `at` of its table -- added to a count
#define WV_STAT_WAVE_LINES(id, on, at) do { uint32_t n_ = 0u; uint64_t seen_[64]; \
    for (uint32_t j_ = 0u; j_ < 64u; j_++) { const uint64_t l_ = wv::readlane64((on) ? ((uint64_t)(at) >> 7) + 1ull : 0ull, j_); bool new_ = l_ != 0ull; \
      for (uint32_t i_ = 0u; i_ < n_; i_++) new_ = new_ && seen_[i_] != l_; \
      if (new_) seen_[n_++] = l_; } \
    if (lane == 0u) wv::stat((id), n_); } while (0)
#else
#define WV_STAT_WAVE_MAX(id, n) do { (void)(n); } while (0)
#define WV_STAT_WAVE_LINES(id, on, at) do { } while (0)
#endif

// ---- the sparse form of phase C: what it is made of
// an inclusive XOR scan over the 64 lanes, in the form of A2's popcount scan: four row steps, then the rows' totals by lane reads
WV_DEV uint32_t xor_scan(uint32_t x, uint32_t lane) {
  x ^= wv::row_shr0<1>(x); x ^= wv::row_shr0<2>(x); x ^= wv::row_shr0<4>(x); x ^= wv::row_shr0<8>(x);
  const uint32_t t0 = wv::readlane(x, 15u), t1 = wv::readlane(x, 31u), t2 = wv::readlane(x, 47u);
  return x ^ (lane >= 16u ? t0 : 0u) ^ (lane >= 32u ? t1 : 0u) ^ (lane >= 48u ? t2 : 0u);
}
// where a call's bit goes OFF: the front after its last (tests/emu plants 0 here and must see the tables differ)
#ifndef TBC_WALK_OFF_AFTER
#define TBC_WALK_OFF_AFTER 1u
#endif
// (the three planted mutations -- this one, TBC_WALK_TWIN_LE, TBC_WALK_NO_SELF_EXCLUSION -- exist for the emulated build only)
#if !defined(TBC_EMU) && (defined(TBC_WALK_TWIN_LE) || defined(TBC_WALK_NO_SELF_EXCLUSION) || (TBC_WALK_OFF_AFTER != 1u))
#error "the planted mutations of the front walk are for tests/emu (TBC_EMU) only"
#endif
// lane = candidate: the call (inv, ret) toggles bit `slot` ON at its first front of the chunk and OFF behind its last one.  tog: per
// front index four words, ON low / high, OFF low / high.  No ON when it completed before the chunk, no OFF when it outlasts it.
WV_DEV void toggle_slot(uint32_t* tog, uint32_t F_lo, uint32_t inv, uint32_t ret, uint32_t slot) {
  if (ret < F_lo) return;
  const uint32_t on = inv > F_lo ? inv - F_lo : 0u, offi = ret + TBC_WALK_OFF_AFTER - F_lo, bit = 1u << (slot & 31u), w = slot >> 5;
  wv::lds_add32(&tog[on * 4u + w], bit);
  if (ret != kInf && offi < 64u) wv::lds_add32(&tog[offi * 4u + 2u + w], bit);
}
// a front's four toggle words zeroed (the zero is made here: as a constant the compiler keeps it in registers over the whole run of chunks)
WV_DEV void zero_toggles(uint32_t* tog, uint32_t lane) {
  const uint32_t z = wv::opaque(0u);
  *reinterpret_cast<wv::u32x4*>(tog + lane * 4u) = wv::u32x4{z, z, z, z};
}
// A round of the form is  zero_toggles, barrier, the candidates' toggles, then this: with lane = front, the inclusive XOR scan of ON ^ OFF
// over the lanes -- the bits whose call is open at the lane's front, low word | high word << 32.  high: whether a bit can be in the high
// word at all (else: one scan).  The caller puts a barrier between its last use of the round's words and the next round's zero_toggles.
WV_DEV uint64_t open_bits(const uint32_t* tog, uint32_t lane, bool high) {
  wv::barrier();
  const wv::u32x4 t4 = *reinterpret_cast<const wv::u32x4*>(tog + lane * 4u);
  const uint32_t lo = xor_scan(t4.x ^ t4.z, lane), hi = high ? xor_scan(t4.y ^ t4.w, lane) : 0u;
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
// The rounds that go by value take the value of the first candidate still pending (set 0 first, then lane order): its flag word, uniform.
// 0 when none is pending (a pending candidate's word has at least the bit that made it pending).
WV_DEV uint32_t next_pending(const bool (&pend)[kSparseSets], const uint32_t (&c_fl)[kSparseSets], uint32_t NC) {
  const uint64_t b0 = wv::ballot(pend[0]), b1 = NC > 64u ? wv::ballot(pend[1]) : 0ull;
  if ((b0 | b1) == 0ull) return 0u;
  return b0 ? wv::readlane(c_fl[0], (uint32_t)__builtin_ctzll(b0)) : wv::readlane(c_fl[1], (uint32_t)__builtin_ctzll(b1));
}
WV_DEV uint32_t key_bucket(uint32_t key) { return (key * 0x9E3779B1u) >> 26; }
#if defined(TBC_EMU)
inline bool& emu_force_dense() { static bool f = false; return f; }      // tests/emu: the dense loop for everything
#endif

// a UNIFORM value, opaque to the optimiser: what a chunk of a run derives from the history's number is worked out again per chunk
// instead of being kept in registers over the whole run (wv::opaque does the same for the lane number)
#if defined(TBC_EMU)
WV_DEV uint32_t opaque_uniform(uint32_t v) { return v; }
#else
WV_DEV uint32_t opaque_uniform(uint32_t v) { asm volatile("" : "+s"(v)); return v; }
#endif

// What the walk only reads and reads at a UNIFORM address (a history's descriptors, its list of slot starts), as constant memory: scalar
// loads.  A run's later chunks come after the stores of the chunks before, and behind a store the compiler takes a load from global memory
// through the vector memory pipe whatever its address -- a dozen vector loads and two dependent trips at the head of every chunk.
#if defined(TBC_EMU)
template <class T> using ro_t = const T;
#else
template <class T> using ro_t = const __attribute__((address_space(4))) T;
#endif
template <class T>
WV_DEV ro_t<T>* read_only(const T* p) { return (ro_t<T>*)(uintptr_t)p; }

// the first of the slot's records [l, hi) that has not completed before ret_from (hi: the tail sentinel)
WV_DEV uint32_t first_open(const Rec* rec, uint32_t l, uint32_t hi, uint32_t ret_from) {
  while (l < hi) {
    const uint32_t mid = (l + hi) >> 1;
    if (rec[mid].ret_rank >= ret_from) hi = mid; else l = mid + 1u;
  }
  return l;
}

// What the phases of a chunk are handed by walk_chunk: where the chunk is, the history's tables, the wavefront's LDS.  All of it is UNIFORM.
// (What a lane keeps from phase to phase -- places, keys, flag words, the list position -- are plain locals of walk_chunk passed by
// reference, and the dense loop's row registers are locals of dense_loop: see store_entries.)
struct Chunk {
  ro_t<PackOpenArgs>* A;                     // (the kernarg segment, wv::cold: what a phase alone reads it takes from here where it uses it)
  ro_t<Hist>* H;
  ro_t<BeamHist>* B;
  uint32_t R, F_lo, F_hi, W;                 // the history's ranks, the chunk's fronts [F_lo, F_hi), the history's slots
  uint32_t ret_from;                         // candidates: the calls that have not completed before this rank (phase A)
  const Rec* rec; const uint32_t* seg; const uint32_t* off;
  OpRec* lst; uint64_t* twn;                 // twn: null = no twin masks
  bool want_tw;
  uint32_t V, FW;                            // row entries; u64 words per front: a plain row, or a front record
  bool compact;                              // the 64 B record, written whole (masks, list location, windows)
  uint64_t* rdm; uint64_t* look;             // null = no rows / no lookahead records
  uint32_t *cand, *aux;                      // LDS: the candidate table; the scratch words (scans, A2's key map, D's rank codes)
  uint16_t* perm;                            //      over aux: the table index of the candidate at each place in list order
  uint32_t* cur_end; uint16_t* cur_left;     //      the cursors: a lane reads what it wrote itself (no barrier)
  uint32_t *tog, *rcnt;                      //      the sparse form's round buffer, over the end of the table
};

// ---- A. lane = process slot: the slot's candidates are consecutive records -- from the first that has not completed before
// F_lo (lookahead: F_lo - 7, for the producer distance) to the last invoked before the chunk's last front.
// The records of a slot are in order of invocation AND of completion, and the next chunk's ret_from is no smaller: its first
// candidate is this chunk's first plus those of this chunk's candidates that complete before the next ret_from (counted where
// the table is filled), and the record after this chunk's last candidate -- invoked at F_hi or later, so completing there or
// later -- is where the next chunk's scan of invocation ranks goes on.  Only a run's first chunk searches.  (Of a slot's candidates
// at most eight are the next chunk's as well: a slot has one call open at a time, so they complete at ranks of their own from
// F_lo + 64 - 7 on, and only the last of them at F_lo + 64 or later.)
// The scan loads four ranks a trip and looks at none behind the first that ends it, which the slot's tail sentinel (inv = kInf) does at
// the latest: the indices are kept inside the HISTORY's records, not the slot's.
// Returns the chunk's candidates, all slots'; the table holds the first kCandCap of them (never more: see the header).
WV_DEV uint32_t fill_candidates(const Chunk& K, uint32_t lane, bool carried) {
  const Rec* rec = K.rec;
  const uint32_t* seg = K.seg;
  const uint32_t F_lo = K.F_lo, F_hi = K.F_hi, W = K.W, V = K.V, ret_from = K.ret_from;
  const uint32_t ret_from_next = K.look ? F_lo + 64u - (kLookahead - 1u) : F_lo + 64u;
  uint32_t lo = 0, k = 0;
  if (lane == 0u) wv::stat(carried ? kStatWalkCarried : kStatWalkSearch, 1);
  if (lane < W) {
    uint32_t i;
    if (carried) { i = K.cur_end[lane]; lo = i - K.cur_left[lane]; }
    else {
      lo = first_open(rec, seg[lane] + 1u, seg[lane + 1] - 1u, ret_from);      // (up to the slot's tail sentinel: inv = ret = kInf)
      i = lo;
    }
#if defined(TBC_EMU)
    if (carried && lo != first_open(rec, seg[lane] + 1u, seg[lane + 1] - 1u, ret_from)) wv::stat(kStatWalkCursorMiss, 1);
    if (i > seg[lane + 1] - 1u) wv::stat(kStatWalkCursorMiss, 1);     // (the scan starts at the tail sentinel at the latest)
#endif
    const uint32_t last = read_only(seg)[W] - 1u;                              // the history's last record (the last slot's tail sentinel)
    for (;;) {                                                      // four invocation ranks per trip (one or two calls is the rule)
      const uint32_t i1 = i + 1u < last ? i + 1u : last, i2 = i + 2u < last ? i + 2u : last, i3 = i + 3u < last ? i + 3u : last;
      const uint32_t v0 = rec[i].inv_rank, v1 = rec[i1].inv_rank, v2 = rec[i2].inv_rank, v3 = rec[i3].inv_rank;
      if (v0 >= F_hi) break;
      i++;
      if (v1 >= F_hi) break;
      i++;
      if (v2 >= F_hi) break;
      i++;
      if (v3 >= F_hi) break;
      i++;
    }
    k = i - lo;
  }
  // where each slot's candidates start: inclusive scan of k over the lanes (through LDS)
  uint32_t incl = k;
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    K.aux[lane] = incl;
    wv::barrier();
    const uint32_t add = lane >= d ? K.aux[lane - d] : 0u;
    wv::barrier();
    incl += add;
  }
  const uint32_t base = incl - k;
  const uint32_t NC_all = wv::readlane(incl, 63u);
  uint32_t gone = 0;                                                // of the slot's candidates: completed before the next chunk's ret_from
  for (uint32_t j = 0; j < k; j++) {
    const Rec r = rec[lo + j];
    gone += r.ret_rank < ret_from_next ? 1u : 0u;
    if (base + j < kCandCap) {
      const bool live = (r.cls & 2u) != 0u, isread = (r.cls & 16u) != 0u, wc = (r.cls & 8u) != 0u;
      const bool in_chunk = r.ret_rank >= F_lo;                     // (else: completed just before the chunk, a producer only)
      const bool listed = live && in_chunk && !(K.A->branch_lists && isread);
      const uint32_t vi = rdm_index(r.a, V);
      uint32_t fl = (lane << 12) | (r.prod << 24);
      if (listed) fl |= kCList;
      if (listed && wc && K.want_tw) fl |= kCTwin;
      if (live && in_chunk && isread && K.rdm && V && (vi != 0u || r.a == TBC_NIL)) fl |= kCRow | (vi << 4);
      if (K.look && (r.cls & 6u) && r.prod != kLookNone) fl |= kCLook;
      uint32_t* e = K.cand + (base + j) * kCandWords;
      e[0] = r.inv_rank; e[1] = r.ret_rank; e[2] = r.opidx; e[3] = r.f | (lane << 8);
      e[4] = (uint32_t)r.a; e[5] = (uint32_t)r.b; e[6] = fl;
      e[7] = (live && wc && in_chunk) ? effect_key(r.f, r.a, r.b) : 0xFFFFFFFFu;
    }
  }
  K.cur_end[lane] = lo + k; K.cur_left[lane] = (uint16_t)(k - gone);
  wv::barrier();
  return NC_all;
}

// ---- A2. list_order 1: phase C takes the candidates in order of completion (then every front's list comes out in that
// order: a front's entries are appended as the loop meets its members).  Candidate i's place = the candidates that complete before it
// (ties -- crashed calls, ret = kInf, which are in no list -- by table position); the places as 16-bit words over the scan's scratch.
// list_order 2: in order of completion with the :write calls after everything else -- the search takes a config's candidates last to
// first and pops the last child first, so a :cas the state allows NOW is tried before a :write, which the state always allows
// (oracle/wgl_beam.c list order 4: at 19 calls in flight a quarter fewer rounds again than plain completion order).  The key: the
// completion rank plus 2^30 for a :write (ranks are below 2^30).
// list_order 16 + W: a :write takes the place of a call completing W ranks later (the soft form of the same preference; keys are doubled
// ranks, a :write's odd: after the call it ties with) -- W = 16 .. 24 is the best of the scan at 6, 19 and 32 calls in flight (oracle list
// order 16 + W: at 19 in flight 19 - 22k rounds a history against 28k writes last, 59k plain completion order).  Any key gives a
// permutation: a place is the count of smaller keys, ties by table position.
// The keys are made UNIQUE so that a place is one compare per pair: completion ranks are (live calls), and so are ranks + 2^30 for
// the writes and doubled ranks with the writes' odd; the only ties of the definition are among crashed calls (ret = kInf), which are in
// no list -- and what phase C does for an unlisted candidate (a bit of a read row, of the lookahead mask, the producer distance)
// does not depend on when it meets it: they take keys above every live one, by table position.
//
// places_by_compare, the fallback.  The keys stay in registers, one candidate per lane (three sets); candidate j's key reaches the lanes by
// a lane read (j is uniform), and every lane counts the smaller keys for each of its candidates: 1 + 2 vector instructions per set instead
// of a dozen with two LDS reads.  That is NC x 3 .. 5 instructions a chunk.  place: zero on entry
WV_DEV void places_by_compare(uint32_t NC, const uint32_t (&my)[3], uint32_t (&place)[3]) {
  if (NC <= 64u) {
    for (uint32_t j = 0; j < NC; j++) place[0] += wv::readlane(my[0], j) < my[0] ? 1u : 0u;
  } else if (NC <= 128u) {
    for (uint32_t j = 0; j < 64u; j++) { const uint32_t kj = wv::readlane(my[0], j); place[0] += kj < my[0] ? 1u : 0u; place[1] += kj < my[1] ? 1u : 0u; }
    for (uint32_t j = 0; j < NC - 64u; j++) { const uint32_t kj = wv::readlane(my[1], j); place[0] += kj < my[0] ? 1u : 0u; place[1] += kj < my[1] ? 1u : 0u; }
  } else {
    WV_UNROLL
    for (int s2 = 0; s2 < 3; s2++) {
      const uint32_t cnt = s2 < 2 ? 64u : NC - 128u;
      for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t kj = wv::readlane(my[s2], j);
        place[0] += kj < my[0] ? 1u : 0u; place[1] += kj < my[1] ? 1u : 0u; place[2] += kj < my[2] ? 1u : 0u;
      }
    }
  }
}
// places_by_counting.  A live candidate completes at ret_from or later (phase A's search), and all but a slot's last one before F_hi: the live
// keys sit in a window above ret_from's that is a few hundred wide unless a call stays open for hundreds of ranks.  Key - base is then a
// bit of a kKeyBits-bit map in LDS (the keys are unique: adding the bit is setting it), 32 lanes prefix the words' popcounts, and a
// place is the bits below the candidate's own; the crashed calls follow the live ones by table position (ballots).  list_order 2 is
// two windows of half the bits, the writes' after the others'.  A chunk with a live key outside its window -- decided per chunk, so
// this covers a race's per-history order_of and any W -- takes the compare loop; so does a list_order whose write offset alone
// exceeds the window.
// d: key - base of a live candidate (inside the window, all of them), else kInf
WV_DEV void places_by_counting(uint32_t* aux, uint32_t NC, uint32_t lane, const uint32_t (&d)[3], uint32_t (&place)[3]) {
  if (lane < kKeyWords) aux[lane] = 0u;
  wv::barrier();
  WV_UNROLL
  for (int s = 0; s < 3; s++) if (d[s] != kInf) wv::lds_add32(&aux[d[s] >> 5], 1u << (d[s] & 31u));
  wv::barrier();
  const uint32_t wc = lane < kKeyWords ? (uint32_t)__builtin_popcount(aux[lane]) : 0u;
  uint32_t y = wc;                                              // inclusive scan over lanes 0 .. 31: two rows of 16
  y += wv::row_shr0<1>(y); y += wv::row_shr0<2>(y); y += wv::row_shr0<4>(y); y += wv::row_shr0<8>(y);
  const uint32_t row0 = wv::readlane(y, 15u);
  y += lane >= 16u ? row0 : 0u;
  const uint32_t n_live = wv::readlane(y, kKeyWords - 1u);
  if (lane < kKeyWords) aux[kKeyWords + lane] = y - wc;
  // the crashed candidates (in no list): after the live ones, by table position
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t cr_before = n_live;
  WV_UNROLL
  for (int s = 0; s < 3; s++) {
    const uint32_t idx = lane + 64u * (uint32_t)s;
    const uint64_t cr = wv::ballot(idx < NC && d[s] == kInf);
    if (d[s] == kInf) place[s] = cr_before + (uint32_t)__builtin_popcountll(cr & below);
    cr_before += (uint32_t)__builtin_popcountll(cr);
  }
  wv::barrier();
  WV_UNROLL
  for (int s = 0; s < 3; s++)
    if (d[s] != kInf) place[s] = aux[kKeyWords + (d[s] >> 5)] + (uint32_t)__builtin_popcount(aux[d[s] >> 5] & ((1u << (d[s] & 31u)) - 1u));
  wv::barrier();                                                // (the places go over the words of the map)
}
// list_places (list_order != 0; else the places are the table's and there is no perm).  place[s]: the place in list order of candidate
// lane + 64 s; K.perm: the candidate at each place
WV_DEV void list_places(const Chunk& K, uint32_t NC, uint32_t lane, uint32_t list_order, uint32_t (&place)[3]) {
  const uint32_t wr_last = list_order == 2u ? 0x40000000u : list_order >= 16u ? 2u * (list_order - 16u) + 1u : 0u;
  const uint32_t rk_mul = list_order >= 16u ? 2u : 1u;
  const uint32_t wr_ofs = list_order == 2u ? kKeyBits / 2u : wr_last, lim_other = list_order == 2u ? kKeyBits / 2u : kKeyBits;
  uint32_t my[3];                                                   // the key
  uint32_t d[3];                                                    // key - base of a live candidate inside the window, else kInf
  bool outside = false;
  WV_UNROLL
  for (int s = 0; s < 3; s++) {
    const uint32_t idx = lane + 64u * (uint32_t)s;
    const uint32_t* e = K.cand + (idx < NC ? idx : 0u) * kCandWords;
    const uint32_t rt = e[1];
    const bool wr = (e[3] & 0xFFu) == TBC_F_WRITE;
    my[s] = idx >= NC ? 0xFFFFFFFFu : rt == kInf ? (0xFFFFFF00u | idx) : rt * rk_mul + (wr ? wr_last : 0u);
    const bool live = idx < NC && rt != kInf;
    const uint32_t x = rt - K.ret_from;                             // (a live call's: below 2^30)
    const bool inside = x < kKeyBits && x * rk_mul + (wr ? wr_ofs : 0u) < (wr ? kKeyBits : lim_other);
    d[s] = (live && inside) ? x * rk_mul + (wr ? wr_ofs : 0u) : kInf;
    outside = outside || (live && !inside);
    place[s] = 0u;
  }
  if (wr_ofs < kKeyBits && wv::ballot(outside) == 0ull) places_by_counting(K.aux, NC, lane, d, place);
  else places_by_compare(NC, my, place);
  WV_UNROLL
  for (int s = 0; s < 3; s++) {
    const uint32_t idx = lane + 64u * (uint32_t)s;
    if (idx < NC) K.perm[place[s]] = (uint16_t)idx;
  }
  wv::barrier();
}

// ---- B. the candidates once more, one per lane: what the sparse form's toggles (two sets) / the dense loop's static twin test (three) ask of them
// (sparse) the flag word of the lane's candidates with the place in list order in its free bits: 18..23 the place's low six bits, 9..10 its pass
WV_DEV void sparse_flags(const Chunk& K, uint32_t NC, uint32_t lane, const uint32_t (&place)[3], uint32_t (&c_fl)[kSparseSets]) {
  WV_UNROLL
  for (int s = 0; s < kSparseSets; s++) {
    const uint32_t idx = lane + 64u * (uint32_t)s;
    if (idx < NC) c_fl[s] = K.cand[idx * kCandWords + 6u] | ((place[s] & 63u) << 18) | ((place[s] >> 6) << 9);
  }
}
// (dense, twin masks) the effect key and the completion rank
WV_DEV void dense_twin_keys(const Chunk& K, uint32_t NC, uint32_t lane, uint32_t (&c_key)[3], uint32_t (&c_ret)[3]) {
  WV_UNROLL
  for (int s = 0; s < 3; s++) {
    const uint32_t idx = lane + 64u * (uint32_t)s;
    const uint32_t* e = K.cand + (idx < NC ? idx : 0u) * kCandWords;
    c_key[s] = idx < NC ? e[7] : 0xFFFFFFFFu;
    c_ret[s] = e[1];
  }
}

// ---- B2 (sparse, twin masks).  The calls of one effect that complete in the chunk or later, chained by completion: with lane = candidate,
// each finds the call of its effect that completes LAST BEFORE IT (its table index, 0xFF = none).  Per set of 64 source candidates, each
// adds its lane's bit to the bucket of its effect key (64 buckets of two words), and every candidate steps through the few bits of its own
// key's bucket with the exact test.  The links then take the place of the keys in the table (word 7): phase C has no other use for a
// key.  An entry's twins at a front are found down the chain (sparse_lists).
// c_key, c_ret: two sets of the registers dense_twin_keys fills for the dense loop, which a chunk on the sparse form does not run
WV_DEV void link_twins(const Chunk& K, uint32_t NC, uint32_t lane, uint32_t (&c_key)[3], uint32_t (&c_ret)[3]) {
  uint32_t* const cand = K.cand;
  uint32_t* const tog = K.tog;
  uint32_t prev[kSparseSets] = {0xFFu, 0xFFu}, prev_ret[kSparseSets] = {0u, 0u};
  WV_UNROLL
  for (int s = 0; s < kSparseSets; s++) {
    const uint32_t idx = lane + 64u * (uint32_t)s;
    if (idx < NC) { c_key[s] = cand[idx * kCandWords + 7u]; c_ret[s] = cand[idx * kCandWords + 1u]; }
  }
  WV_UNROLL
  for (int sp = 0; sp < kSparseSets; sp++) {
    if (64u * (uint32_t)sp >= NC) continue;
    { const uint32_t z = wv::opaque(0u); tog[lane * 2u] = z; tog[lane * 2u + 1u] = z; }
    wv::barrier();
    if (c_key[sp] != 0xFFFFFFFFu) wv::lds_add32(&tog[key_bucket(c_key[sp]) * 2u + (lane >> 5)], 1u << (lane & 31u));
    wv::barrier();
    WV_UNROLL
    for (int s = 0; s < kSparseSets; s++) {
      uint64_t mk = 0ull;
      if (c_key[s] != 0xFFFFFFFFu) {
        const uint32_t hb = key_bucket(c_key[s]);
        mk = (uint64_t)tog[hb * 2u] | ((uint64_t)tog[hb * 2u + 1u] << 32);
      }
      WV_STAT_WAVE_MAX(kStatWalkFindWave, (uint32_t)__builtin_popcountll(mk));
      while (mk) {
        const uint32_t u = 64u * (uint32_t)sp + (uint32_t)__builtin_ctzll(mk);
        mk &= mk - 1ull;
        const uint32_t* eu = cand + u * kCandWords;
        const uint32_t ru = eu[1];
        wv::stat(kStatWalkTwinFind, 1);
#if defined(TBC_WALK_TWIN_LE)       // (planted by tests/emu: the call itself becomes its own twin; sparse_lists stops at a link to itself)
        if (eu[7] == c_key[s] && ru <= c_ret[s] && (prev[s] == 0xFFu || ru > prev_ret[s])) { prev[s] = u; prev_ret[s] = ru; }
#else
        if (eu[7] == c_key[s] && ru < c_ret[s] && (prev[s] == 0xFFu || ru > prev_ret[s])) { prev[s] = u; prev_ret[s] = ru; }
#endif
      }
    }
    wv::barrier();
  }
  WV_UNROLL
  for (int s = 0; s < kSparseSets; s++) if (lane + 64u * (uint32_t)s < NC) cand[(lane + 64u * (uint32_t)s) * kCandWords + 7u] = prev[s];
  wv::barrier();
}

// ---- C. lane = front.  What a lane knows of its front before it looks at a candidate, read only from here on: where its list starts, and
// the call completing there, from the op columns (pack_kernel copied the records from them) -- its slot; what it needs, produces and how
// long it has been open (lookahead); its function and argument (compact records).  Fc: the front the idle lanes of the last chunk load from.
struct Front {
  uint32_t F, Fc; bool active;
  uint32_t pos0, px, need, xprod, di, x, xf; int32_t xa;
};
WV_DEV Front front_of(const Chunk& K, uint32_t lane) {
  const auto& A = *K.A;
  const auto* H = K.H;
  Front f;
  f.F = K.F_lo + lane;
  f.active = f.F < K.F_hi;
  f.Fc = f.active ? f.F : K.F_hi - 1u;                              // (loads of the idle lanes of the last chunk stay in range)
  f.pos0 = K.off[f.Fc];
  f.px = A.ret_slot[H->ret_off + f.Fc];
  f.need = kLookNone; f.xprod = kLookNone; f.di = 0; f.x = 0; f.xf = kFNone; f.xa = 0;
  if (K.look || K.compact) {
    f.x = A.ret_op[H->ret_off + f.Fc];
    f.xf = A.f[H->op_off + f.x];
    f.xa = A.a[H->op_off + f.x];
  }
  if (K.look) {
    const int32_t xb = A.b[H->op_off + f.x];
    const uint32_t xinv = A.scratch[H->frame_off + f.x];
    f.need = look_need(f.xf, f.xa); f.xprod = look_prod(f.xf, f.xa, xb);
    f.di = f.F - xinv < 255u ? f.F - xinv : 255u;
  }
  return f;
}
// the front's lookahead record: pm = the slots of the calls open here that produce what the completing call needs, dmin = the producer distance
WV_DEV void store_look(const Chunk& K, const Front& f, uint64_t pm, uint32_t dmin) {
  if (f.active && K.look) {
    pm &= ~(1ull << (f.px & 63u));                                  // one call per slot is open at a front: this is the completing call itself
    K.look[(uint64_t)f.F * 2u] = look_word0(f.px, f.need, f.xprod, f.di, dmin);
    K.look[(uint64_t)f.F * 2u + 1u] = pm;
  }
}

// ---- C, THE SPARSE FORM.  No loop over the candidates with lane = front: a call is open at the fronts inv .. ret, so with lane =
// candidate it toggles a bit ON at index max(inv, F_lo) - F_lo and OFF at ret + 1 - F_lo of a 64-entry array in LDS (toggle_slot), and
// with lane = front the inclusive XOR scan of ON ^ OFF over the lanes is the set of calls open at each front (open_bits).  The bits are
// unique per (word, index) -- a slot has one call open at a time, its next call is invoked at a later rank than its last completion, a
// crashed call's slot is not reused -- so adding is setting; a slot whose call ends at F - 1 and whose next begins at F gets both events at F.
// sparse_read_rows: bit = process slot, a round per read-row entry present among the chunk's candidates: the scan IS the front's row entry,
// stored where it is made (no row in registers); the entries no round made are stored as zero afterwards
WV_DEV void sparse_read_rows(const Chunk& K, uint32_t NC, uint32_t lane, const Front& f, const uint32_t (&c_fl)[kSparseSets]) {
  uint64_t* const row = K.rdm ? K.rdm + (uint64_t)f.F * K.FW : nullptr;
  const uint32_t n_row = K.compact ? 6u : K.V;
  uint32_t made = 0u;
  bool pend[kSparseSets];
  WV_UNROLL
  for (int s = 0; s < kSparseSets; s++) pend[s] = (c_fl[s] & kCRow) != 0u;
  for (uint32_t fl; (fl = next_pending(pend, c_fl, NC)) != 0u;) {
    const uint32_t v = (fl >> 4) & 31u;
    if (lane == 0u) wv::stat(kStatWalkRounds, 1);
    zero_toggles(K.tog, lane);
    wv::barrier();
    WV_UNROLL
    for (int s = 0; s < kSparseSets; s++)
      if (pend[s] && ((c_fl[s] >> 4) & 31u) == v) { const uint32_t* e = K.cand + (lane + 64u * (uint32_t)s) * kCandWords; toggle_slot(K.tog, K.F_lo, e[0], e[1], (c_fl[s] >> 12) & 63u); pend[s] = false; }
    const uint64_t open = open_bits(K.tog, lane, K.W > 32u);
    if (f.active && v < n_row) row[v] = open;
    made |= 1u << v;
    wv::barrier();
  }
  if (K.rdm)
    for (uint32_t v = 0; v < n_row; v++) if (!((made >> v) & 1u) && f.active) row[v] = 0ull;
}
// sparse_producers: bit = process slot, a round per produced value present that some front of the chunk needs: a front takes the scan of its
// own `need` as its producer mask.  The same round counts, a byte per rank, the producers of the value invoked at ranks F_lo - 7 ..
// F_lo + 63 (candidates that completed before the chunk included; at most one per slot and rank, so a byte does not carry): a front
// reads the eight bytes of ranks F - 7 .. F, takes its own call out (it may produce what it needs: a cas v v) and the highest byte
// left that is not zero is the nearest producer.
WV_DEV void sparse_producers(const Chunk& K, uint32_t NC, uint32_t lane, const Front& f, const uint32_t (&c_fl)[kSparseSets]) {
  static_assert(kLookahead == 8u, "a front's window of invocation ranks is eight bytes");
  uint32_t* const rcnt = K.rcnt;
  uint64_t pm = 0ull;
  uint32_t dmin = 255u;
  bool pend[kSparseSets];
  WV_UNROLL
  for (int s = 0; s < kSparseSets; s++) pend[s] = (c_fl[s] & kCLook) != 0u;
  for (uint32_t fl; (fl = next_pending(pend, c_fl, NC)) != 0u;) {
    const uint32_t v = fl >> 24;
    const bool mine = f.active && f.need == v;
    if (wv::ballot(mine) == 0ull) {                              // nobody needs it
      WV_UNROLL
      for (int s = 0; s < kSparseSets; s++) if ((c_fl[s] >> 24) == v) pend[s] = false;
      continue;
    }
    if (lane == 0u) wv::stat(kStatWalkRounds, 1);
    zero_toggles(K.tog, lane);
    if (lane < kRankCntWords) rcnt[lane] = 0u;
    wv::barrier();
    WV_UNROLL
    for (int s = 0; s < kSparseSets; s++)
      if (pend[s] && (c_fl[s] >> 24) == v) {
        const uint32_t* e = K.cand + (lane + 64u * (uint32_t)s) * kCandWords;
        const uint32_t inv = e[0];
        toggle_slot(K.tog, K.F_lo, inv, e[1], (c_fl[s] >> 12) & 63u);
        if (inv + (kLookahead - 1u) >= K.F_lo) {
          const uint32_t ri = inv + (kLookahead - 1u) - K.F_lo;        // (invoked before the chunk's last front: below 71)
          wv::lds_add32(&rcnt[ri >> 2], 1u << (8u * (ri & 3u)));
        }
        pend[s] = false;
      }
    const uint64_t open = open_bits(K.tog, lane, K.W > 32u);
    if (mine) {
      pm = open;
      const uint32_t wb = lane >> 2, sh = 8u * (lane & 3u);
      const uint64_t lo64 = (uint64_t)rcnt[wb] | ((uint64_t)rcnt[wb + 1u] << 32);
      uint64_t xb = sh ? ((lo64 >> sh) | ((uint64_t)rcnt[wb + 2u] << (64u - sh))) : lo64;     // byte j: rank F - 7 + j
#if !defined(TBC_WALK_NO_SELF_EXCLUSION)
      if (f.xprod == f.need && f.di < kLookahead) xb -= 1ull << (8u * (kLookahead - 1u - f.di));
#endif
      dmin = xb ? (uint32_t)__builtin_clzll(xb) >> 3 : 255u;
    }
    wv::barrier();
  }
  store_look(K, f, pm, dmin);
}
// sparse_lists: bit = the candidate's place in list order, listed candidates only, 64 places a round: a front's list entries, ascending bit =
// list order.  The entries are then stored with LANE = ENTRY.  A chunk's entries are one contiguous piece of lst / twn -- off[] is the
// running sum of the fronts' counts, so front F's entries follow front F - 1's -- and a store instruction with consecutive lane = consecutive
// entry writes 1 KB (lst) resp. 512 B (twn) of whole lines, where lane = front wrote 64 pieces some 100 B apart.
//   * The front lanes leave their sets in the round buffer (a front's four toggle words are its two sets of 64 places: the rounds are over) and
//     keep their count; an add-scan over the lanes gives each front the chunk-relative position of its first entry.
//   * The entries are taken 64 at a time.  A front whose first entry lies in the pass marks it: its number in the byte of that entry (the
//     bytes lie over the rank counters of sparse_producers, which is done).  An entry lane finds its front by a max-scan over the lanes of
//     (front, lane of the mark) -- both grow with the lane -- or, before the pass's first mark, takes the front the pass before ended in;
//     its rank k within the front is its distance from the mark.
//   * It takes the k-th set bit of the front's words (kth_set_bit), which is its candidate's place, the candidate's record from the table at an
//     address of its own, and walks the twin chain: the twin mask of an entry at front F is, down the chain of its effect (link_twins) from the
//     call itself, the slots of the calls open at F -- the chain is in order of completion, so it ends at the first call that completed before F.
// Returns where the lane's front's list ends (lst, twn).
// the place (0 .. 127) of the k-th set bit, k from 0, of the 128 bits t.x | t.y << 32 | t.z << 64 | t.w << 96, which have more than k bits set
WV_DEV uint32_t kth_set_bit(const wv::u32x4& t, uint32_t k) {
  const uint32_t c0 = (uint32_t)__builtin_popcount(t.x), c1 = c0 + (uint32_t)__builtin_popcount(t.y), c2 = c1 + (uint32_t)__builtin_popcount(t.z);
  uint32_t w = t.x, p = 0u;
  if (k >= c2) { w = t.w; p = 96u; k -= c2; } else if (k >= c1) { w = t.z; p = 64u; k -= c1; } else if (k >= c0) { w = t.y; p = 32u; k -= c0; }
  WV_UNROLL
  for (uint32_t s = 16u; s != 0u; s >>= 1) {
    const uint32_t c = (uint32_t)__builtin_popcount(w & ((1u << s) - 1u));
    if (k >= c) { k -= c; w >>= s; p += s; }
  }
  return p;
}
// an inclusive max-scan over the 64 lanes (xor_scan's form; 0 is below everything scanned)
WV_DEV uint32_t max_scan(uint32_t x, uint32_t lane) {
  const auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  x = mx(x, wv::row_shr0<1>(x)); x = mx(x, wv::row_shr0<2>(x)); x = mx(x, wv::row_shr0<4>(x)); x = mx(x, wv::row_shr0<8>(x));
  const uint32_t t0 = wv::readlane(x, 15u), t1 = wv::readlane(x, 31u), t2 = wv::readlane(x, 47u);
  return mx(mx(x, lane >= 16u ? t0 : 0u), mx(lane >= 32u ? t1 : 0u, lane >= 48u ? t2 : 0u));
}
// (planted by tests/emu, see test_walk_lines_emu.py: the rank within the front one too high; a front whose first entry is a pass's first is not marked there)
#if !defined(TBC_EMU) && (defined(TBC_WALK_RANK_OFF_BY_ONE) || defined(TBC_WALK_FRONT_LE))
#error "the planted mutations of the front walk are for tests/emu (TBC_EMU) only"
#endif
WV_DEV uint32_t sparse_lists(const Chunk& K, uint32_t NC, uint32_t lane, const Front& f, const uint32_t (&c_fl)[kSparseSets], bool by_ret) {
  static_assert(kSparseSets == 2 && kTogWords == 64u * 4u && kRankCntWords >= 16u, "a front's two sets are its four toggle words; 64 mark bytes");
  const uint32_t* const cand = K.cand;
  uint32_t* const mark = K.rcnt;
  uint64_t open[kSparseSets] = {0ull, 0ull};
  WV_UNROLL
  for (int g = 0; g < kSparseSets; g++) {
    if (64u * (uint32_t)g >= NC) continue;
    zero_toggles(K.tog, lane);
    wv::barrier();
    WV_UNROLL
    for (int s = 0; s < kSparseSets; s++)
      if ((c_fl[s] & kCList) && ((c_fl[s] >> 9) & 3u) == (uint32_t)g) { const uint32_t* e = cand + (lane + 64u * (uint32_t)s) * kCandWords; toggle_slot(K.tog, K.F_lo, e[0], e[1], (c_fl[s] >> 18) & 63u); }
    const uint64_t o = open_bits(K.tog, lane, true);
    open[g] = f.active ? o : 0ull;
    wv::barrier();
  }
  // lane = front: the sets into the round buffer; where the front's entries start within the chunk's
  *reinterpret_cast<wv::u32x4*>(K.tog + lane * 4u) = wv::u32x4{(uint32_t)open[0], (uint32_t)(open[0] >> 32), (uint32_t)open[1], (uint32_t)(open[1] >> 32)};
  const uint32_t n = (uint32_t)__builtin_popcountll(open[0]) + (uint32_t)__builtin_popcountll(open[1]);
  uint32_t incl = n;
  incl += wv::row_shr0<1>(incl); incl += wv::row_shr0<2>(incl); incl += wv::row_shr0<4>(incl); incl += wv::row_shr0<8>(incl);
  {
    const uint32_t t0 = wv::readlane(incl, 15u), t1 = t0 + wv::readlane(incl, 31u), t2 = t1 + wv::readlane(incl, 47u);
    incl += lane >= 48u ? t2 : lane >= 32u ? t1 : lane >= 16u ? t0 : 0u;
  }
  const uint32_t start = incl - n, total = wv::readlane(incl, 63u);
  const uint32_t base = wv::readlane(f.pos0, 0u);                   // (the chunk has a front: lane 0's)
#if defined(TBC_EMU)
  if (f.active && f.pos0 != base + start) wv::stat(kStatWalkNotContiguous, 1);      // off[] is the running sum of the fronts' counts
  if (lane == 0u) wv::stat(kStatWalkEntries, total);
#endif
  // lane = entry, 64 at a time
  uint32_t carry_front = 0u, carry_start = 0u;                      // (uniform) the front the pass before ended in, and where its entries start
  WV_NOUNROLL
  for (uint32_t e0 = 0u; e0 < total; e0 += 64u) {
    if (lane == 0u) wv::stat(kStatWalkEmitTrips, 1);
    if (lane < 16u) mark[lane] = wv::opaque(0u);
    wv::barrier();
#if defined(TBC_WALK_FRONT_LE)
    if (n != 0u && !(start <= e0) && start - e0 < 64u)
#else
    if (n != 0u && !(start < e0) && start - e0 < 64u)
#endif
      wv::lds_add32(&mark[(start - e0) >> 2], (0x40u | lane) << (8u * ((start - e0) & 3u)));      // (one front starts at an entry: adding is setting)
    wv::barrier();
    const uint32_t mb = (mark[lane >> 2] >> (8u * (lane & 3u))) & 0xFFu;
    const uint32_t mv = max_scan(mb ? (0x1000u | ((mb & 63u) << 6) | lane) : 0u, lane);
    const uint32_t fr = mv ? (mv >> 6) & 63u : carry_front;
#if defined(TBC_WALK_RANK_OFF_BY_ONE)
    const uint32_t k = (mv ? lane - (mv & 63u) : e0 + lane - carry_start) + 1u;
#else
    const uint32_t k = mv ? lane - (mv & 63u) : e0 + lane - carry_start;
#endif
    {
      const uint32_t last = wv::readlane(mv, 63u);
      if (last != 0u) { carry_front = (last >> 6) & 63u; carry_start = e0 + (last & 63u); }
    }
    uint32_t chain_steps = 0u;                                      // (counted for the emulated build's statistics only)
    if (e0 + lane < total) {
      const uint32_t F = K.F_lo + fr;
      const wv::u32x4 sets = *reinterpret_cast<const wv::u32x4*>(K.tog + fr * 4u);
      const uint32_t p = kth_set_bit(sets, k);
      uint32_t ci = by_ret ? (uint32_t)K.perm[p] : p;
#if defined(TBC_EMU)
      if (p >= 64u) wv::stat(kStatWalkSecondSet, 1);
      if (ci >= NC || k >= (uint32_t)__builtin_popcount(sets.x) + (uint32_t)__builtin_popcount(sets.y) + (uint32_t)__builtin_popcount(sets.z) + (uint32_t)__builtin_popcount(sets.w)) {
        wv::stat(kStatWalkBadPlace, 1);                             // (no such entry: a planted mutation; the read below stays inside the table)
        ci = 0u;
      }
#endif
      const uint32_t* e = cand + ci * kCandWords;
      const uint64_t at = (uint64_t)base + e0 + lane;
      OpRec o; o.op = e[2]; o.f_slot = e[3] | (e[1] == F ? kAtFront : 0u); o.a = (int32_t)e[4]; o.b = (int32_t)e[5];
      K.lst[at] = o;
      if (K.twn) {
        uint64_t tw = 0ull;
        for (uint32_t u = e[7] & 0xFFu; u != 0xFFu;) {
          const uint32_t* eu = cand + u * kCandWords;
          wv::stat(kStatWalkTwinSteps, 1);
          chain_steps++;
          if (eu[1] < F) break;
          if (eu[0] <= F) tw |= 1ull << ((eu[3] >> 8) & 63u);
#if defined(TBC_WALK_TWIN_LE)
          if ((eu[7] & 0xFFu) == u) break;
#endif
          u = eu[7] & 0xFFu;
        }
        K.twn[at] = tw;
      }
    }
    WV_STAT_WAVE_MAX(kStatWalkChainWave, chain_steps);
    WV_STAT_WAVE_LINES(kStatWalkLstLines, e0 + lane < total, (K.B->lst_off + base + e0 + lane) * sizeof(OpRec));
    wv::barrier();                                                  // (the marks are read: the next pass zeroes them)
  }
  return f.pos0 + n;
}

// ---- C, THE DENSE LOOP: iteration t broadcasts the candidate at place t of the list order to the 64 lanes, and each lane decides for ITS
// front whether the call is open there -- then appends it to its front's list (lst, twn at pos), ors its slot into its read row (registers:
// see store_entries) / its producer mask, keeps the nearest producer.  c_key, c_ret: dense_twin_keys.
template <int VCAP>
WV_DEV uint32_t dense_loop(const Chunk& K, uint32_t NC, uint32_t lane, const Front& f, const uint32_t (&c_key)[3], const uint32_t (&c_ret)[3], bool by_ret, uint32_t pos) {
  const uint32_t* const cand = K.cand;
  const uint32_t F = f.F;
  const bool active = f.active;
  wv::u32x16 r0, r1, r2, r3;                // the front's row (r1 .. r3: rows of more than 8 entries only)
  WV_UNROLL
  for (int i = 0; i < 16; i++) { r0[i] = 0u; r1[i] = 0u; r2[i] = 0u; r3[i] = 0u; }
  uint32_t pm_lo = 0u, pm_hi = 0u, dmin = 255u;
  WV_NOUNROLL
  for (uint32_t t = 0; t < NC; t++) {
    const uint32_t* e = cand + (by_ret ? (uint32_t)K.perm[t] : t) * kCandWords;
    const uint32_t inv = e[0], ret = e[1];
    const uint32_t fl = wv::readfirstlane(e[6]);
    const uint32_t slot = (fl >> 12) & 63u;
    const bool member = active && inv <= F && F <= ret;             // open at this lane's front (a crashed call: ret = kInf)
    if (fl & kCList) {
      uint32_t tw_lo = 0u, tw_hi = 0u;
      if (fl & kCTwin) {
        const uint32_t key_t = e[7];
        // same effect, completes before t, still open when t is invoked: the same at every front
        uint64_t s0 = wv::ballot(c_key[0] == key_t && c_ret[0] < ret && c_ret[0] >= inv);
        uint64_t s1 = 0ull, s2 = 0ull;
        if (NC > 64u) s1 = wv::ballot(c_key[1] == key_t && c_ret[1] < ret && c_ret[1] >= inv);
        if (NC > 128u) s2 = wv::ballot(c_key[2] == key_t && c_ret[2] < ret && c_ret[2] >= inv);
        while (s0 | s1 | s2) {
          uint32_t u;
          if (s0) { u = (uint32_t)__builtin_ctzll(s0); s0 &= s0 - 1ull; }
          else if (s1) { u = 64u + (uint32_t)__builtin_ctzll(s1); s1 &= s1 - 1ull; }
          else { u = 128u + (uint32_t)__builtin_ctzll(s2); s2 &= s2 - 1ull; }
          const uint32_t* eu = cand + u * kCandWords;
          const bool mu = eu[0] <= F && F <= eu[1];                 // ... and open at THIS front
          or_slot(tw_lo, tw_hi, mu, (wv::readfirstlane(eu[6]) >> 12) & 63u);
        }
      }
      if (member) {
        OpRec o; o.op = e[2]; o.f_slot = e[3] | (ret == F ? kAtFront : 0u); o.a = (int32_t)e[4]; o.b = (int32_t)e[5];
        K.lst[pos] = o;
        if (K.twn) K.twn[pos] = (uint64_t)tw_lo | ((uint64_t)tw_hi << 32);
        pos++;
      }
    }
    if (fl & kCRow)                                                 // open-read masks by value: one word of one entry
    {
      const uint32_t w = ((fl >> 4) & 31u) * 2u + (slot >> 5), bit = member ? (1u << (slot & 31u)) : 0u;
      if constexpr (VCAP <= 8) r0[w & 15u] |= bit;
      else {
        const uint32_t q = w >> 4;
        if (q == 0u) r0[w & 15u] |= bit; else if (q == 1u) r1[w & 15u] |= bit; else if (q == 2u) r2[w & 15u] |= bit; else r3[w & 15u] |= bit;
      }
    }
    if (fl & kCLook) {                 // who else, open here, produces what the completing call needs; how recently such a call was invoked
      const bool hit = (fl >> 24) == f.need;
      or_slot(pm_lo, pm_hi, member && hit, slot);
      const uint32_t dist = F - inv;                                // (invoked after this front: wraps past kLookahead)
      if (hit && dist < kLookahead && e[2] != f.x) dmin = dist < dmin ? dist : dmin;
    }
  }
  if (active && K.rdm) {
    uint64_t* row = K.rdm + (uint64_t)F * K.FW;
    const uint32_t n_row = K.compact ? 6u : K.V;
    store_entries<0>(r0, row, n_row);
    if constexpr (VCAP > 8) { store_entries<1>(r1, row, n_row); store_entries<2>(r2, row, n_row); store_entries<3>(r3, row, n_row); }
  }
  store_look(K, f, (uint64_t)pm_lo | ((uint64_t)pm_hi << 32), dmin);
  return pos;
}

// ---- D. the rest of a compact front record: word 6, the list's location (nl entries from pos0) and the count of open calls, and word 7,
// the window of the next seven ranks (tbc_internal.h), through LDS: codes of the chunk + 6 after
WV_DEV void compact_tail(const Chunk& K, uint32_t lane, const Front& f, bool by_ret, uint32_t nl) {
  const auto& A = *K.A;
  const auto* H = K.H;
  uint32_t* const aux = K.aux;
  if (by_ret) wv::barrier();                                        // (the places lived in these words: every lane is past phase C)
  aux[lane] = f.active ? rank_code(f.px, f.xf, f.xa, K.V) : (7u << 6);
  if (lane < kFrontCompactRanks - 1u) {
    const uint32_t G = K.F_lo + 64u + lane;
    uint32_t code = 7u << 6;                                        // (past the last rank: slot 0, not a read)
    if (G < K.R) {
      const uint32_t gx = A.ret_op[H->ret_off + G];
      code = rank_code(A.ret_slot[H->ret_off + G], A.f[H->op_off + gx], A.a[H->op_off + gx], K.V);
    }
    aux[64u + lane] = code;
  }
  wv::barrier();
  uint64_t w7 = 0ull;
  WV_UNROLL
  for (uint32_t l = kFrontCompactRanks; l-- > 0u;) w7 |= (uint64_t)aux[lane + l] << (9u * l);
  const uint64_t w6 = front_word6(f.pos0, nl, A.ncr[K.B->off_off + f.Fc]);
  if (f.active && K.rdm) {
    uint64_t* row = K.rdm + (uint64_t)f.F * K.FW;
    row[6] = w6; row[7] = w7;
  }
}

// One chunk: fronts 64 c .. 64 c + 63 of history h.  carried: the slot cursors are what the chunk before left in LDS (else: from nothing).
// Returns whether the history has a front after this chunk.
// VCAP: row entries kept in registers (vpad <= VCAP)
template <int VCAP>
WV_DEV bool walk_chunk(const PackOpenArgs& A_, uint32_t h, uint32_t c, uint32_t* lds, uint32_t lane, bool carried) {
  const auto& A = *wv::cold(A_);            // (the arguments from the kernarg segment, per chunk: not some sixty scalar registers held over a run)
  const auto* H = read_only(&A.hist[h]);
  const auto* B = read_only(&A.bh[h]);
  const uint32_t R = H->n_ret;
  const uint32_t F_lo = c * 64u;
  if (H->status != 0 || B->status != 0 || F_lo >= R) return false;
  Chunk K;
  K.A = &A; K.H = H; K.B = B;
  K.R = R; K.F_lo = F_lo; K.F_hi = F_lo + 64u < R ? F_lo + 64u : R;
  K.W = H->n_slots;
  K.rec = A.rec + H->rec_off;
  K.seg = A.seg + H->seg_off;
  K.off = A.off + B->off_off;
  K.lst = A.lst + B->lst_off;
  K.twn = A.twn ? A.twn + B->lst_off : nullptr;
  K.want_tw = K.twn != nullptr;
  K.V = A.vpad;
  K.FW = A.front_words ? A.front_words : K.V;
  K.compact = A.front_compact != 0u;
  K.rdm = (A.rdm && (K.V || K.compact)) ? A.rdm + H->op_off * K.FW : nullptr;
  K.look = A.look ? A.look + look_off(H->op_off, h, 1u) : nullptr;
  K.ret_from = K.look ? (F_lo >= kLookahead - 1u ? F_lo - (kLookahead - 1u) : 0u) : F_lo;
  K.cand = lds;
  K.aux = lds + kCandCap * kCandWords;
  K.perm = reinterpret_cast<uint16_t*>(K.aux);
  K.cur_end = K.aux + kAuxWords;
  K.cur_left = reinterpret_cast<uint16_t*>(K.cur_end + 64);
  K.tog = K.cand + kSparseCand * kCandWords;
  K.rcnt = K.tog + kTogWords;

  // A: the candidate table
  const uint32_t NC_all = fill_candidates(K, lane, carried);
  const uint32_t NC = NC_all < kCandCap ? NC_all : kCandCap;      // (never more: see the header)
  // A2: the candidates' places in list order
  const uint32_t list_order = A.order_of ? A.order_of[h] : A.list_order;          // (the history's own order, if the batch says one)
  const bool by_ret = list_order != 0u;
  uint32_t place[3] = {lane, lane + 64u, lane + 128u};              // candidate lane + 64 s: its place in list order (list_order 0: the table's)
  if (by_ret) list_places(K, NC, lane, list_order, place);

  // The sparse form of phase C or the dense loop: decided per chunk, uniformly.  The dense loop takes rows of more than 8 entries
  // (VCAP) and a chunk of more than kSparseCand candidates (the form's round buffer lies over the end of the table).
  bool sparse = VCAP <= 8 && NC_all <= kSparseCand;
#if defined(TBC_EMU)
  if (emu_force_dense()) sparse = false;
#endif
  // B, B2: the candidates in registers, one per lane; (sparse) the twin chains
  uint32_t c_fl[kSparseSets] = {0u, 0u};
  uint32_t c_key[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, c_ret[3] = {0u, 0u, 0u};
  if (sparse) sparse_flags(K, NC, lane, place, c_fl);
  else if (K.want_tw) dense_twin_keys(K, NC, lane, c_key, c_ret);
  if constexpr (VCAP <= 8) if (sparse && K.want_tw) link_twins(K, NC, lane, c_key, c_ret);
  if (lane == 0u) wv::stat(sparse ? kStatWalkSparse : kStatWalkDense, 1);
  if (lane == 0u) wv::stat(kStatWalkCands + (NC_all > 64u ? 1u : 0u) + (NC_all > kSparseCand ? 1u : 0u), 1);

  // C: lane = front.  Either form leaves the fronts' rdm rows, their look records and, from pos on, their lst / twn entries
  const Front f = front_of(K, lane);
  uint32_t pos = f.pos0;
  bool dense = true;
  if constexpr (VCAP <= 8) if (sparse) {
    dense = false;
    sparse_read_rows(K, NC, lane, f, c_fl);
    sparse_producers(K, NC, lane, f, c_fl);
    pos = sparse_lists(K, NC, lane, f, c_fl, by_ret);
  }
  if (dense) pos = dense_loop<VCAP>(K, NC, lane, f, c_key, c_ret, by_ret, pos);
  // D: words 6 and 7 of a compact record
  if (K.compact) compact_tail(K, lane, f, by_ret, pos - f.pos0);
  return F_lo + 64u < R;
}

// one chunk from nothing: chunk wid % chunks_per_hist of history h0 + wid / chunks_per_hist
template <int VCAP>
WV_DEV void walk_wave(const PackOpenArgs& A, uint32_t wid, uint32_t* lds, uint32_t lane) {
  const uint32_t cph = A.chunks_per_hist;
  const uint32_t hr = wid / cph, c = wid - hr * cph, h = A.h0 + hr;
  if (h >= A.n_hist) return;
  (void)walk_chunk<VCAP>(A, h, c, lds, lane, false);
}

// runs a history is cut into: ceil(chunks / RUN)
WV_HD constexpr uint32_t walk_runs_per_hist(uint32_t chunks_per_hist, uint32_t run = kWalkRun) { return (chunks_per_hist + run - 1u) / run; }

// a run: chunks RUN r .. RUN r + RUN - 1 of one history (run_id = history * runs per history + r), one after the other; it ends with
// the history's last front.  The first chunk starts from nothing, the others from the cursors the chunk before left.
template <int VCAP, uint32_t RUN = kWalkRun>
WV_DEV void walk_run(const PackOpenArgs& A, uint32_t run_id, uint32_t* lds, uint32_t lane) {
  const uint32_t rph = walk_runs_per_hist(A.chunks_per_hist, RUN);
  const uint32_t hr = run_id / rph, c0 = (run_id - hr * rph) * RUN, h = A.h0 + hr;
  if (h >= A.n_hist) return;
  WV_NOUNROLL
  for (uint32_t j = 0; j < RUN; j++) {
    if (!walk_chunk<VCAP>(A, opaque_uniform(h), c0 + j, lds, wv::opaque(lane), j != 0u)) break;
    wv::barrier();                                                  // (every lane is done with this chunk's table and scratch words)
  }
}

}  // namespace walk
}  // namespace tbc
