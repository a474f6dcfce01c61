// set_full.hip -- jepsen.checker/set-full's per-element scan on the MI355X (gfx950).
//
// The reference's set-full workload is checked by `(checker/set-full {:linearizable? true})`
// (/root/reference/src/tigerbeetle/workloads/set_full.clj:157; jepsen itself is not in /root/reference --
// the algorithm is recalled and restated in oracle/set_full.py).  Per element three history indices decide
// its outcome: known, last_present, last_absent (include/tbcheck.h).  They are reductions over the
// reads x elements membership matrix:
//   last_present[e] = max read_invoke[r] over reads r that contain e      }  only reads completing after
//   last_absent[e]  = max read_invoke[r] over reads r that do not         }  e's add was invoked count
//   known[e]        = min(add_ok[e], min read_ok[r] over reads containing e)
// This is the one streaming kernel of the path: the matrix is n_reads x n_elements bits (2 GB at 65,536 reads
// of 262,144 elements) and is read about half once.
//
// Layout: rows = reads in invocation order, words_per_row 32-bit words each; a wavefront's 64 lanes take 64
// consecutive words of a row (256 B coalesced).  Two passes, no atomics:
//   setfull_any_kernel      grid = word columns x chunks of rows: a thread ORs "present" and "absent" over FOUR word
//                           columns (128 elements, 16 B loads) of ONE chunk, eight rows in flight -- the streaming
//                           pass, coalesced words written per thread;
//   setfull_resolve_kernel  one thread per word column: the chunk summaries say WHICH chunk holds each element's last
//                           present / last absent / first present read; only those chunks are walked again, bit-parallel
//                           (a 32-bit "still wanted" mask per direction), and the thread writes its own 32 results.
// Elements are numbered by add invocation, so "reads completing after e's add was invoked" is a PREFIX of the elements
// for each row (p[r], one binary search per row in setfull_prefix_kernel) and a chunk whose reads all precede a
// column's adds is skipped without a load: the all-zero triangle below the diagonal is never read.
// known: the first read (in invocation order) containing e need not be the first to complete, so the walk keeps
// offering later rows' read_ok while they were invoked before the latest first-completion seen -- a window bounded by
// the LONGEST READ, in rows: every read invoked while it was open (one paused reader holds the window open over hundreds of rows
// and across chunks, however few readers there are).
//
// One object and one set of kernels behind the three entry points: jepsen.independent splits the reference's set-full history into keys
// (set_full.clj:155) and checks each on its own, so an object holds n_keys keys (tbc_setfull_keys_create), and a single key
// (tbc_setfull_create_rows; tbc_setfull_create with the matrix given dense) is an object of one key.  At real sizes a key's matrix is a
// few MB: one object per key would pay its fixed price (allocation, stream, copies, synchronisation) once per key while its scan
// fills a sliver of the GPU.  Every launch goes through the plan table below; create = rows + prefix, run = any + resolve, whatever
// n_keys is.
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include "tbc_internal.h"
#include "set_full_plan.h"
#include "set_full_encode_plan.h"

using namespace tbc;

namespace {

constexpr uint32_t kSetFullRows = 2048;      // rows per chunk at most (their metadata is staged in LDS)
constexpr uint32_t kWordCounters = 256;      // the words-loaded statistic: a wavefront adds to counter (its workgroup mod 256), 128 B apart -- thousands of
                                             // atomics on ONE address queue up in one L2 channel; the host adds the counters up

__global__ __launch_bounds__(256) void setfull_prefix_kernel(const SfKeyPlan* __restrict__ plan, const uint32_t* __restrict__ first, uint32_t n_keys,
                                                             const uint32_t* add_invoke, const uint32_t* read_ok, uint32_t* P, uint32_t* pmax) {
  const uint32_t* f = first + kFirstPrefix * (n_keys + 1u);
  const uint32_t k = sf_find_key(f, n_keys, blockIdx.x);
  const SfKeyPlan& p = plan[k];
  const uint32_t r = (blockIdx.x - f[k]) * 256u + threadIdx.x;
  if (r >= p.R) return;
  const uint32_t t = read_ok[p.row_base + r];
  uint32_t lo = 0, hi = p.E;                     // first element whose add was invoked at or after this read's completion
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (add_invoke[p.elem_base + mid] < t) lo = mid + 1; else hi = mid; }
  P[p.row_base + r] = lo;
  atomicMax(&pmax[p.pmax_off + r / p.rows_per_chunk], lo);
  atomicMin(&pmax[p.pmax_off + p.chunks + r / p.rows_per_chunk], lo);         // (the minima lie behind the maxima)
}

__device__ __forceinline__ uint32_t prefix_mask(uint32_t p, uint32_t w) {       // bits of word w below element number p
  return p >= 32u * w + 32u ? 0xFFFFFFFFu : (p <= 32u * w ? 0u : (1u << (p - 32u * w)) - 1u);
}

// ---- the membership matrix from the reads' compact form (tbc_setfull_create_rows, tbc_setfull_keys_create): one workgroup per read
// writes its row -- ones below top[r], zeros above (a coalesced stream: the matrix is written once, at HBM's write rate) -- and then
// flips the listed exceptions in it.  No row ever exists on the host.  The whole pitch is written (zeros past E: top <= E), so no word
// of the arena the scan loads is left unset.
__global__ __launch_bounds__(256) void setfull_rows_kernel(const SfKeyPlan* __restrict__ plan, const uint32_t* __restrict__ first, uint32_t n_keys,
                                                           uint32_t R_all, const uint32_t* __restrict__ top, const unsigned long long* __restrict__ exc_off,
                                                           const uint32_t* __restrict__ exc, uint32_t* __restrict__ M) {
  for (uint32_t r = blockIdx.x; r < R_all; r += gridDim.x) {
    const SfKeyPlan& p = plan[sf_find_key(first + kFirstRows * (n_keys + 1u), n_keys, r)];
    uint32_t* __restrict__ row = M + p.m_off + (uint64_t)(r - p.row_base) * p.PITCH;
    const uint32_t t = top[r];
    for (uint32_t w = threadIdx.x; w < p.PITCH; w += 256u) row[w] = prefix_mask(t, w);
    __syncthreads();
    for (unsigned long long i = exc_off[r] + threadIdx.x; i < exc_off[r + 1]; i += 256u) {
      const uint32_t e = exc[i];
      atomicXor(&row[e >> 5], 1u << (e & 31u));
    }
    __syncthreads();
  }
}

// ---- pass 1: per (word column, chunk of rows) -- is any bit of the column present / absent in the chunk?  The streaming
// pass.  A lane takes FOUR consecutive word columns (VEC: 16 B loads, a wavefront 1 KB of a row); eight rows are requested, then
// folded.  Nothing a load returns decides whether the next is issued (a chunk is at most 2,048 rows: stopping at a saturated column
// saved nothing on set-full's matrices, where an element is absent before its add and present after, and cost a round trip every
// eight rows); no atomics.  Three kinds of tile (256 VEC columns x a chunk):
// below the diagonal (return), on it (the general path: the chunk's row metadata in LDS, a mask per row and word), above it (the lean
// path: every column counts in every row).
// Round 6 (profiles/r06_setfull_*, scripts/exp/strip_read.hip = this access pattern, bare: 6.1 TB/s a rectangle, 5.3 the triangle):
// 0.16 -> 0.105 ms.  What it was NOT: bytes in flight (4, 8 or 16 rows a lane read alike), the row pitch (a power of two, padded: the
// same), the per-row masks (the lean path alone: 3 %).  What it was: the summaries' scattered 4 B stores (43 us, below) and the XCDs
// (column block j in blockIdx.x was XCD j: 7 %).
// The summaries lie CHUNK-major ([chunk][word column], SP words a chunk, SP a multiple of four): this pass writes a thread's four
// columns as one 16 B store, a wavefront 1 KB.  Rounds 2 - 5 kept them column-major for pass 2's sake (a column's chunks as one line)
// and paid for it here without knowing: 4 B stores 1 KB apart, every one a masked write of its own into a line that sixteen
// workgroups on eight XCDs write -- 43 us of this kernel's 150 (scripts/exp/strip_read.hip: the bare triangle 0.114 ms, with the
// column-major stores 0.157, with these 0.117).  Pass 2 reads a column's chunks as 64 words of 64 lines now, and is given its
// columns so that the workgroups of one XCD share those lines (setfull_resolve_kernel).
constexpr int VEC = 4;
__device__ __forceinline__ void store_summary(uint32_t* __restrict__ any_p, uint32_t* __restrict__ any_a, uint32_t SP, uint32_t c, uint32_t w0,
                                              const uint32_t (&pa)[VEC], const uint32_t (&aa)[VEC]) {
  const uint64_t at = (uint64_t)c * SP + w0;
  *reinterpret_cast<uint4*>(any_p + at) = make_uint4(pa[0], pa[1], pa[2], pa[3]);
  *reinterpret_cast<uint4*>(any_a + at) = make_uint4(aa[0], aa[1], aa[2], aa[3]);
}

__global__ __launch_bounds__(256) void setfull_any_kernel(const SfKeyPlan* __restrict__ plan, const uint32_t* __restrict__ first, uint32_t n_keys,
                                                          const uint32_t* __restrict__ M_all, const uint32_t* __restrict__ P_all,
                                                          const uint32_t* __restrict__ pmax_all, uint32_t* __restrict__ any_p_all,
                                                          uint32_t* __restrict__ any_a_all, unsigned long long* words_loaded) {
  const uint32_t* f = first + kFirstAny * (n_keys + 1u);
  const uint32_t key = sf_find_key(f, n_keys, blockIdx.x);
  const SfKeyPlan& p = plan[key];
  const uint32_t tile = blockIdx.x - f[key];
  // the key's grid = (chunks, column blocks), the CHUNK in x: tile t is (t % chunks, t / chunks), the order a 2-D launch hands them out in
  const uint32_t gx = p.chunks, gy = p.any_gy, bx = tile % gx, by = tile / gx;
  const uint32_t* __restrict__ M = M_all + p.m_off;
  const uint32_t* __restrict__ P = P_all + p.row_base;
  const uint32_t* __restrict__ pmax = pmax_all + p.pmax_off;
  uint32_t* __restrict__ any_p = any_p_all + p.sum_off;
  uint32_t* __restrict__ any_a = any_a_all + p.sum_off;
  const uint32_t E = p.E, R = p.R, WPR = p.WPR, PITCH = p.PITCH, rows_per_chunk = p.rows_per_chunk, SP = p.PITCH;
  constexpr uint32_t U = 8u;                            // rows in flight per lane (16 B each)
  // Workgroup b runs on XCD b % 8 (observed, MI355X_MICROARCH.md "Workgroup dispatch"),
  // and the work is a triangle: column block j counts in the chunks above j / n of the rows only.  With the column block in x (rounds
  // 3 - 5: eight of them for 262,144 elements, i.e. column block j WAS XCD j) XCD 0 streamed 256 chunks and XCD 7 32 -- the kernel
  // lasted as long as XCD 0's 22 % of the matrix through one XCD's fabric port.  With the chunk in x every XCD gets every eighth
  // chunk of every column block.
  // The order the workgroups are handed out in (x fastest, then y): the LAST column block first, and in every column block the chunks
  // from its diagonal on -- the tiles on the diagonal decide per row (the general path below: the longest workgroups) and start first,
  // the tiles below the diagonal, which return at once, come last.
  const uint32_t cb = gy - 1u - by;
  const uint32_t c = (bx + (uint32_t)((uint64_t)cb * gx / gy)) % gx;
  const uint32_t w0 = (cb * 256u + threadIdx.x) * (uint32_t)VEC;
  uint32_t loaded = 0;
  __shared__ uint32_t s_P[kSetFullRows];
  const uint32_t r0 = min(c * rows_per_chunk, R), r1 = min(r0 + rows_per_chunk, R);     // (a trailing chunk may be empty)
  // the whole workgroup lies below the diagonal: nothing to stage, nothing to read, nothing to write (which workgroups these are is
  // fixed with the object -- P is -- and tbc_setfull_create zeroed the summaries)
  if (pmax[c] <= 32u * (cb * 256u * (uint32_t)VEC)) return;
  // A workgroup whose columns ALL count in EVERY row of its chunk (the chunk's least prefix reaches past its last column: four tiles in
  // five of set-full's triangle) has nothing to decide per row: no row metadata, no masks, eight 16 B loads a lane and two instructions
  // a word -- the fold of the general path below costs ~50 vector instructions a row and wavefront, 43 us of a SIMD's time per launch
  // beside 88 us of streaming (scripts/exp/strip_read.hip: this very access pattern, bare, reads at 6.1 TB/s, 6.7 non-temporal).
  const uint32_t tile_hi = 32u * ((cb + 1u) * 256u * (uint32_t)VEC);
  if (pmax[gx + c] >= (tile_hi < E ? tile_hi : E)) {
    if (w0 < WPR) {
      typedef uint32_t wvec __attribute__((ext_vector_type(VEC)));
      uint32_t po[VEC], na[VEC];
#pragma unroll
      for (int v = 0; v < VEC; v++) { po[v] = 0u; na[v] = 0xFFFFFFFFu; }
      const uint32_t* src = M + (uint64_t)r0 * PITCH + w0;
      uint32_t r = r0;
      constexpr uint32_t UL = 8u;
      for (; r + UL <= r1; r += UL, src += (uint64_t)UL * PITCH) {
        wvec x[UL];
#pragma unroll
        for (uint32_t q = 0; q < UL; q++) x[q] = __builtin_nontemporal_load(reinterpret_cast<const wvec*>(src + (uint64_t)q * PITCH));
#pragma unroll
        for (uint32_t q = 0; q < UL; q++)
#pragma unroll
          for (int v = 0; v < VEC; v++) { po[v] |= x[q][v]; na[v] &= x[q][v]; }
      }
      for (; r < r1; r++, src += PITCH) {
        const wvec x = __builtin_nontemporal_load(reinterpret_cast<const wvec*>(src));
#pragma unroll
        for (int v = 0; v < VEC; v++) { po[v] |= x[v]; na[v] &= x[v]; }
      }
      uint32_t pa[VEC], aa[VEC];
#pragma unroll
      for (int v = 0; v < VEC; v++) {
        const uint32_t lo = 32u * (w0 + (uint32_t)v);
        const uint32_t full = lo >= E ? 0u : (E - lo >= 32u ? 0xFFFFFFFFu : (1u << (E - lo)) - 1u);
        pa[v] = po[v] & full; aa[v] = ~na[v] & full;
        loaded += full ? r1 - r0 : 0u;
      }
      store_summary(any_p, any_a, SP, c, w0, pa, aa);
    }
    unsigned long long tot = loaded;
    for (int d = 32; d >= 1; d >>= 1) tot += __shfl_xor(tot, d);
    if ((threadIdx.x & 63u) == 0 && tot) atomicAdd(words_loaded + 16u * (blockIdx.x % kWordCounters), tot);
    return;
  }
  for (uint32_t i = threadIdx.x; i < r1 - r0; i += 256u) s_P[i] = P[r0 + i];
  __syncthreads();
  if (w0 < WPR) {
    uint32_t pa[VEC], aa[VEC], full[VEC];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      pa[v] = 0u; aa[v] = 0u;
      const uint32_t lo = 32u * (w0 + (uint32_t)v);
      full[v] = lo >= E ? 0u : (E - lo >= 32u ? 0xFFFFFFFFu : (1u << (E - lo)) - 1u);
    }
    if (pmax[c] > 32u * w0) {
      // rows [hi - U, hi) of the chunk (latest first; fewer at its start): requested ...
      const auto fetch = [&](uint32_t hi, uint32_t (&wd)[U][VEC], uint32_t (&pr)[U]) {
        const uint32_t lo = hi - r0 >= U ? hi - U : r0;
#pragma unroll
        for (uint32_t q = 0; q < U; q++) {
          const uint32_t r = hi - 1u - q;
          const bool in = hi - lo > q;
          const uint32_t pv = s_P[in ? r - r0 : 0u];                    // (read either way: no branch between the loads)
          pr[q] = in ? pv : 0u;                                         // (0: no element of the row counts)
          const bool need = pr[q] > 32u * w0 && full[0] != 0u;
          // a row that does not count is not fetched -- but by an ADDRESS, not a branch: such a lane reads row 0's words (one hot line
          // for the whole grid; the fold masks them out, vm = 0).  A branch around every load hides from the compiler how many loads
          // are outstanding, and it then waits for ALL of them (s_waitcnt vmcnt(0)) before the fold: the rows requested ahead would
          // be waited for at once, i.e. nothing would be ahead
          const uint32_t* src = M + (need ? (uint64_t)r * PITCH : 0ull) + w0;
          const uint4 x = *reinterpret_cast<const uint4*>(src);
          wd[q][0] = x.x; wd[q][1] = x.y; wd[q][2] = x.z; wd[q][3] = x.w;
        }
      };
      // ... and folded into the column's two words
      const auto fold = [&](const uint32_t (&wd)[U][VEC], const uint32_t (&pr)[U]) {
#pragma unroll
        for (uint32_t q = 0; q < U; q++) {
#pragma unroll
          for (int v = 0; v < VEC; v++) {
            const uint32_t vm = prefix_mask(pr[q], w0 + (uint32_t)v) & full[v];
            pa[v] |= wd[q][v] & vm; aa[v] |= ~wd[q][v] & vm; loaded += vm ? 1u : 0u;
          }
        }
      };
      // U rows requested, then folded (scripts/exp/strip_read.hip: at this occupancy a second set of registers on its way while the first
      // is folded reads no faster than this, and a workgroup's chain of waits is half as long with eight rows a wait as with four)
      uint32_t wa[U][VEC], pra[U];
      uint32_t hi = r1;
      while (hi > r0) {
        fetch(hi, wa, pra);
        hi = hi - r0 >= U ? hi - U : r0;
        fold(wa, pra);
      }
    }
    store_summary(any_p, any_a, SP, c, w0, pa, aa);
  }
  unsigned long long tot = loaded;
  for (int d = 32; d >= 1; d >>= 1) tot += __shfl_xor(tot, d);
  if ((threadIdx.x & 63u) == 0 && tot) atomicAdd(words_loaded + 16u * (blockIdx.x % kWordCounters), tot);
}

// ---- pass 2: one WAVEFRONT per word column resolves its 32 elements.  The chunk summaries say WHICH chunk holds an
// element's last present / last absent / first present read: lanes hold the summaries of 64 chunks each, a ballot finds
// the deciding chunk, and that chunk is walked again with lane = row (64 rows loaded at once, one ballot per wanted bit
// finds the row).  No atomics, no serial chain of loads.  Lane b < 32 keeps element b's three results in registers and writes
// them once, in their final form (no index: TBC_NO_OP; known: the earlier of the add's ack and the first read that held it).
__device__ __forceinline__ uint32_t wave_min_u32_all(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
  return v;
}

// 64 rows of one word column requested AHEAD of the walk that uses them (lane l = row base + l < hi): the column's word, the row's
// prefix and read_invoke (read_ok for the walk of `known`).  The three indices of a column are three chains of dependent trips; the
// first trip of each is known as soon as the summaries are, and the three go out together.
struct RowsAhead { uint32_t base, hi, word, pv, third; };
__device__ __forceinline__ RowsAhead rows_ahead(const uint32_t* __restrict__ M, const uint32_t* __restrict__ P, const uint32_t* __restrict__ third,
                                                uint32_t PITCH, uint32_t w, uint32_t base, uint32_t hi, uint32_t lane) {
  RowsAhead a; a.base = base; a.hi = hi;
  const uint32_t r = base + lane;
  const bool in = r < hi;
  a.word = in ? M[(uint64_t)r * PITCH + w] : 0u; a.pv = in ? P[r] : 0u; a.third = in ? third[r] : 0u;
  return a;
}

// walk chunk c from its latest row down, lane = row: for every bit of `want` find the latest row where the bit is present
// (present = true) or absent; lane b keeps read_invoke + 1 of bit b's row in `res`; returns the bits found
__device__ __forceinline__ uint32_t setfull_last_in_chunk(const uint32_t* __restrict__ M, const uint32_t* __restrict__ P,
                                                          const uint32_t* __restrict__ read_invoke, uint32_t PITCH, uint32_t w, uint32_t full,
                                                          uint32_t r0, uint32_t r1, uint32_t want, bool present, uint32_t& res, uint32_t lane,
                                                          uint32_t& loaded, const RowsAhead& ah) {
  uint32_t found = 0;
  if (!(r1 > r0)) return found;
  // the rows of a step are requested while the step before is resolved (the first: with the summaries, if the caller did); word, prefix
  // and read_invoke of a row come in ONE trip (not waiting for P[r] to say whether the row counts)
  RowsAhead cur = ah;
  {
    const uint32_t base = r1 - r0 > 64u ? r1 - 64u : r0;
    if (!(ah.base == base && ah.hi == r1)) cur = rows_ahead(M, P, read_invoke, PITCH, w, base, r1, lane);
  }
  for (uint32_t hi = r1; hi > r0 && (want & ~found); hi = hi - r0 > 64u ? hi - 64u : r0) {
    const uint32_t base = hi - r0 > 64u ? hi - 64u : r0;       // rows [base, hi), lane l = row base + l
    const uint32_t r = base + lane;
    const bool in = r < hi;
    RowsAhead nxt = cur;
    if (base > r0) nxt = rows_ahead(M, P, read_invoke, PITCH, w, base - r0 > 64u ? base - 64u : r0, base, lane);
    const uint32_t word = cur.word;
    const uint32_t valid = in ? prefix_mask(cur.pv, w) & full : 0u;
    const uint32_t inv1 = in ? cur.third + 1u : 0u;
    cur = nxt;
    loaded += valid ? 1u : 0u;
    const uint32_t x = (present ? word : ~word) & valid;
    // row by row, not bit by bit: the latest row that has ANY wanted bit settles all the bits it has (ten instructions), and a group's
    // wanted bits mostly sit in one or two rows -- the last read holds every element but the lost ones; the row before an add lacks all
    // the later elements.  (Rounds 2 - 5 took the bits one at a time, ten instructions each: 2,570 vector instructions a wavefront,
    // 36 us of a SIMD's issue in a 57 us kernel -- profiles/r06_setfull_pmc.txt.)  Never more turns than wanted bits.
    uint32_t todo = want & ~found;
    uint64_t rows = __ballot((x & todo) != 0u);
    while (rows) {
      const uint32_t l = 63u - (uint32_t)__builtin_clzll(rows);
      const uint32_t xl = (uint32_t)__builtin_amdgcn_readlane((int)x, l) & todo;
      const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)inv1, l);
      if (lane < 32u && ((xl >> lane) & 1u)) res = v;
      found |= xl; todo &= ~xl;
      rows = __ballot((x & todo) != 0u) & ((1ull << l) - 1ull);
    }
  }
  return found;
}

#ifndef SF_RESOLVE_MIN_WAVES
#define SF_RESOLVE_MIN_WAVES 8          /* 43 registers: every one of the 8,192 wavefronts of 262,144 elements resident at once */
#endif
__global__ __launch_bounds__(256, SF_RESOLVE_MIN_WAVES) void setfull_resolve_kernel(const SfKeyPlan* __restrict__ plan, const uint32_t* __restrict__ first,
                                                              uint32_t n_keys, const uint32_t* __restrict__ M_all, const uint32_t* __restrict__ P_all,
                                                              const uint32_t* __restrict__ read_invoke_all, const uint32_t* __restrict__ read_ok_all,
                                                              const uint32_t* __restrict__ any_p_all, const uint32_t* __restrict__ any_a_all,
                                                              const uint32_t* __restrict__ add_ok_all, uint32_t* lp_all, uint32_t* la_all, uint32_t* known_all,
                                                              unsigned long long* words_loaded) {
  const uint32_t* f = first + kFirstResolve * (n_keys + 1u);
  const uint32_t key = sf_find_key(f, n_keys, blockIdx.x);
  const SfKeyPlan& p = plan[key];
  const uint32_t nb = (p.WPR + 3u) / 4u, bx = blockIdx.x - f[key];
  // (a key of a multiple of eight workgroups starts on a multiple of eight -- the XCD-contiguous order below holds -- and the tiles
  // skipped to get there belong to the key before, past its last workgroup)
  if (bx >= nb) return;
  // the results go straight into the caller's layout (key after key, n_elements each)
  const uint32_t* __restrict__ add_ok = add_ok_all + p.elem_base;
  uint32_t* lp = lp_all + p.elem_base; uint32_t* la = la_all + p.elem_base; uint32_t* known = known_all + p.elem_base;
  const uint32_t E = p.E, R = p.R, WPR = p.WPR, PITCH = p.PITCH, rows_per_chunk = p.rows_per_chunk, chunks = p.chunks, SP = p.PITCH;
  const uint32_t lane = threadIdx.x & 63u;
  if (R == 0u) {            // a key without reads: nothing was seen, known = the add's ack
    const uint32_t e = 32u * (bx * 4u + (threadIdx.x >> 6)) + lane;
    if (lane < 32u && e < E) { lp[e] = kNoneU; la[e] = kNoneU; known[e] = add_ok[e]; }
    return;
  }
  const uint32_t* __restrict__ M = M_all + p.m_off;
  const uint32_t* __restrict__ P = P_all + p.row_base;
  const uint32_t* __restrict__ read_invoke = read_invoke_all + p.row_base;
  const uint32_t* __restrict__ read_ok = read_ok_all + p.row_base;
  const uint32_t* __restrict__ any_p = any_p_all + p.sum_off;
  const uint32_t* __restrict__ any_a = any_a_all + p.sum_off;
  // workgroup b runs on XCD b % 8 (observed): the eight XCDs take eight contiguous ranges of the columns, so that the lines four
  // neighbouring workgroups read 16 B each of -- the summaries' and the matrix rows' -- are fetched into ONE L2 instead of eight
  const uint32_t bb = nb % 8u == 0u ? (bx % 8u) * (nb / 8u) + bx / 8u : bx;
  const uint32_t wv_ = threadIdx.x >> 6;
  const uint32_t w = __builtin_amdgcn_readfirstlane(bb * 4u + wv_);
  uint32_t loaded = 0;
  // the chunk summaries, 64 chunks (one per lane) at a time; any number of chunks
  const uint32_t G = (chunks + 63u) / 64u;
  // up to 256 chunks (what tbc_setfull_create makes of up to 524,288 reads): the summaries of the workgroup's FOUR columns are fetched
  // once, thread t the 16 B of chunk t (chunk-major: its four columns lie side by side), and handed to the four wavefronts through LDS
  // -- a wavefront reading its own column's 256 words asked for 8 x 64 lines, half of all the lines this kernel asks its L1 for
  const bool pre = G <= 4u;
  __shared__ uint4 s_sp[256], s_sa[256];
  if (pre) {
    const uint32_t cl = threadIdx.x;
    const bool in = cl < chunks && bb * 4u < WPR;                     // (SP is a multiple of four: the 16 B lie inside the chunk's row)
    s_sp[cl] = in ? *reinterpret_cast<const uint4*>(any_p + (uint64_t)cl * SP + bb * 4u) : make_uint4(0u, 0u, 0u, 0u);
    s_sa[cl] = in ? *reinterpret_cast<const uint4*>(any_a + (uint64_t)cl * SP + bb * 4u) : make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
  }
  if (w < WPR) {
    const uint32_t full = E - 32u * w >= 32u ? 0xFFFFFFFFu : (1u << (E - 32u * w)) - 1u;
    uint32_t sp[4], sa[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t cl = lane + 64u * k;
      sp[k] = pre ? reinterpret_cast<const uint32_t*>(&s_sp[cl])[wv_] : 0u;
      sa[k] = pre ? reinterpret_cast<const uint32_t*>(&s_sa[cl])[wv_] : 0u;
    }
    const auto pick = [](const uint32_t (&r)[4], uint32_t gi) -> uint32_t { return gi == 0u ? r[0] : gi == 1u ? r[1] : gi == 2u ? r[2] : r[3]; };
    // the first trip of each of the three walks below, requested now (up to 256 chunks: the summaries are in registers)
    RowsAhead ah_p = {kNoneU, 0u, 0u, 0u, 0u}, ah_a = ah_p, ah_k = ah_p;
    if (pre) {
      uint32_t top_p = kNoneU, top_a = kNoneU, low_p = kNoneU;
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) {
        const uint64_t bp = __ballot((sp[k] & full) != 0u), ba = __ballot((sa[k] & full) != 0u);
        if (bp) { top_p = 63u - (uint32_t)__builtin_clzll(bp) + 64u * k; if (low_p == kNoneU) low_p = (uint32_t)__builtin_ctzll(bp) + 64u * k; }
        if (ba) top_a = 63u - (uint32_t)__builtin_clzll(ba) + 64u * k;
      }
      const auto top_rows = [&](uint32_t c, uint32_t& base, uint32_t& hi) {
        const uint32_t r0 = min(c * rows_per_chunk, R); hi = min(r0 + rows_per_chunk, R); base = hi - r0 > 64u ? hi - 64u : r0;
      };
      uint32_t b_, h_;
      if (top_p != kNoneU) { top_rows(top_p, b_, h_); ah_p = rows_ahead(M, P, read_invoke, PITCH, w, b_, h_, lane); }
      if (top_a != kNoneU) { top_rows(top_a, b_, h_); ah_a = rows_ahead(M, P, read_invoke, PITCH, w, b_, h_, lane); }
      if (low_p != kNoneU) { b_ = low_p * rows_per_chunk; ah_k = rows_ahead(M, P, read_ok, PITCH, w, b_, min(b_ + 64u, R), lane); }
    }
    // last present / last absent: the latest chunk that has the bit decides; inside it, the latest row
    uint32_t res_p = 0u, res_a = 0u;          // read_invoke + 1 of the element's last present / last absent read, 0 = none
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
      const uint32_t* __restrict__ any = pass == 0 ? any_p : any_a;
      uint32_t& res = pass == 0 ? res_p : res_a;
      uint32_t need = full;
      for (uint32_t gi = G; gi-- > 0 && need;) {
        const uint32_t cl = lane + 64u * gi;
        const uint32_t mine = pre ? pick(pass == 0 ? sp : sa, gi) : (cl < chunks ? any[(uint64_t)cl * SP + w] : 0u);
        uint64_t cand = __ballot((mine & need) != 0u);
        while (cand && need) {
          const uint32_t l = 63u - (uint32_t)__builtin_clzll(cand);
          const uint32_t c = l + 64u * gi;
          const uint32_t mc = (uint32_t)__builtin_amdgcn_readlane((int)mine, l) & need;
          const uint32_t r0 = min(c * rows_per_chunk, R), r1 = min(r0 + rows_per_chunk, R);
          (void)setfull_last_in_chunk(M, P, read_invoke, PITCH, w, full, r0, r1, mc, pass == 0, res, lane, loaded, pass == 0 ? ah_p : ah_a);
          need &= ~mc;
          cand = __ballot((mine & need) != 0u) & ((1ull << l) - 1ull);
        }
      }
    }
    // known: min read_ok over the reads containing the element.  The earliest chunk that has a bit of the column holds
    // the first containing read (in invocation order) of some element; a read invoked before that one completed may still
    // complete earlier, so the walk goes on, 64 rows at a time, while rows were invoked before `until` (the latest first
    // completion seen).
    uint32_t ever = 0, first_c = chunks;
    for (uint32_t gi = 0; gi < G; gi++) {
      const uint32_t cl = lane + 64u * gi;
      uint32_t o = (pre ? pick(sp, gi) : (cl < chunks ? any_p[(uint64_t)cl * SP + w] : 0u)) & full;
      const uint64_t bl = __ballot(o != 0u);
      if (bl && first_c == chunks) first_c = (uint32_t)__builtin_ctzll(bl) + 64u * gi;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) o |= (uint32_t)__shfl_xor((int)o, d);
      ever |= o;
    }
    uint32_t best = 0xFFFFFFFFu;                                // lane b < 32 keeps element b's minimum
    if (ever) {
      uint32_t seen = 0, until = 0;
      // a step's rows (word, prefix, read_ok -- and read_invoke, which says whether the walk goes on) are requested while the step before is
      // resolved: one trip a step where there were two (read_invoke first, the rest only if the walk went on)
      const uint32_t base0 = first_c * rows_per_chunk;
      RowsAhead cur = ah_k.base == base0 ? ah_k : rows_ahead(M, P, read_ok, PITCH, w, base0, min(base0 + 64u, R), lane);
      uint32_t cur_inv = base0 + lane < R ? read_invoke[base0 + lane] : 0xFFFFFFFFu;
      for (uint32_t base = base0; base < R; base += 64u) {
        const uint32_t r = base + lane;
        const bool in = r < R;
        const uint32_t inv_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur_inv);
        if (seen == ever && inv_first > until) break;
        RowsAhead nxt = cur; uint32_t nxt_inv = 0xFFFFFFFFu;
        if (base + 64u < R) {
          nxt = rows_ahead(M, P, read_ok, PITCH, w, base + 64u, min(base + 128u, R), lane);
          nxt_inv = base + 64u + lane < R ? read_invoke[base + 64u + lane] : 0xFFFFFFFFu;
        }
        const uint32_t word = cur.word;
        const uint32_t valid = in ? prefix_mask(cur.pv, w) & full : 0u;
        const uint32_t ok = in ? cur.third : 0xFFFFFFFFu;
        cur = nxt; cur_inv = nxt_inv;
        loaded += valid ? 1u : 0u;
        const uint32_t hits = word & valid;
        uint32_t any_hits = hits;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) any_hits |= (uint32_t)__shfl_xor((int)any_hits, d);
        // row by row here too: the row that completes first among those holding a still-open bit gives its read_ok to every open bit
        // it holds; a turn or two settle nearly every group
        uint32_t open_ = any_hits;
        for (int turn = 0; turn < 8 && open_; turn++) {
          const uint32_t m = wave_min_u32_all((hits & open_) ? ok : 0xFFFFFFFFu);
          const uint64_t who = __ballot((hits & open_) != 0u && ok == m);
          const uint32_t xl = (uint32_t)__builtin_amdgcn_readlane((int)hits, (uint32_t)__builtin_ctzll(who)) & open_;
          if (lane < 32u && ((xl >> lane) & 1u)) best = min(best, m);
          if (xl & ~seen) until = max(until, m);              // (the first batch's minimum bounds the first containing read's completion)
          open_ &= ~xl;
        }
        while (open_) {                                         // (what eight turns leave -- hardly ever anything -- bit by bit)
          const uint32_t b = (uint32_t)__builtin_ctz(open_);
          open_ &= open_ - 1u;
          const uint32_t m = wave_min_u32_all(((hits >> b) & 1u) ? ok : 0xFFFFFFFFu);
          if (lane == b) best = min(best, m);
          if (!((seen >> b) & 1u)) until = max(until, m);
        }
        seen |= any_hits;
      }
    }
    const uint32_t e = 32u * w + lane;
    if (lane < 32u && e < E) {
      lp[e] = res_p ? res_p - 1u : kNoneU;
      la[e] = res_a ? res_a - 1u : kNoneU;
      known[e] = min(best, add_ok[e]);
    }
  }
  unsigned long long tot = loaded;
  for (int d = 32; d >= 1; d >>= 1) tot += __shfl_xor(tot, d);
  if ((threadIdx.x & 63u) == 0 && tot) atomicAdd(words_loaded + 16u * (blockIdx.x % kWordCounters), tot);
}

#define SF_TRY(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
      return e_ == hipErrorOutOfMemory ? TBC_ERR_OOM : TBC_ERR_HIP;                          \
    }                                                                                        \
  } while (0)

constexpr size_t kCounterBytes = (size_t)kWordCounters * 128;

}  // namespace

#include "set_full_results.h"
#include "set_full_encode.h"

// One object behind all three entry points: a single key (tbc_setfull) is a keyed object with n_keys = 1.
struct SfObject {
  int device = 0;
  uint32_t n_keys = 0, sumE = 0, sumR = 0;
  uint32_t tiles_any = 0, tiles_resolve = 0;
  uint64_t bytes_matrix = 0;
  SfKeyPlan* d_plan = nullptr;
  uint32_t *d_first = nullptr, *d_add_ok = nullptr, *d_read_invoke = nullptr, *d_read_ok = nullptr, *d_M = nullptr, *d_P = nullptr;
  uint32_t *d_pmax = nullptr, *d_anyp = nullptr, *d_anya = nullptr, *d_out = nullptr;     // d_out: known | lp | la, each in the caller's layout
  unsigned long long* d_words = nullptr;
  unsigned long long h_words[kWordCounters * 16] = {};
  void* arena = nullptr;            // ONE allocation holds every array above and the inputs: one hipMalloc, one hipFree
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // tbc_setfull_results: the greatest op index among each key's inputs (-1: none), recorded at create; the results' own arena (made by
  // the first call, again when a call brings more times than it holds) and events
  std::vector<int64_t> key_max;
  uint32_t tiles_select = 0;
  void* res_arena = nullptr;
  uint64_t res_times = 0;
  hipEvent_t ev2 = nullptr, ev3 = nullptr;
  // tbc_setfull_keys_create_ops: the plan the host made of the ops (what tbc_setfull_keys_encoding hands back), what the encoding kernels
  // found, their events, and the reads' raw values on the device -- an allocation of its own, freed before create returns (8 B a value
  // where the matrix has a bit)
  bool from_ops = false;
  sfenc::Plan enc;
  std::vector<uint32_t> dup_max, dup_count;
  std::vector<uint64_t> unknown;
  uint64_t ns_encode = 0;
  uint32_t h_repeats = 0;
  void* d_vals = nullptr;
  hipEvent_t ev_e0 = nullptr, ev_e1 = nullptr, ev_d0 = nullptr, ev_d1 = nullptr;
  ~SfObject() {
    if (arena) (void)hipFree(arena);
    if (d_vals) (void)hipFree(d_vals);
    for (hipEvent_t e : {ev_e0, ev_e1, ev_d0, ev_d1}) if (e) (void)hipEventDestroy(e);
    if (res_arena) (void)hipFree(res_arena);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev2) (void)hipEventDestroy(ev2);
    if (ev3) (void)hipEventDestroy(ev3);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
// (the C handles tbc_setfull and tbc_setfull_keys stay incomplete types: two names of a pointer to this object)
SfObject* sf_obj(tbc_setfull* h) { return reinterpret_cast<SfObject*>(h); }
SfObject* sf_obj(tbc_setfull_keys* h) { return reinterpret_cast<SfObject*>(h); }

namespace {

tbc_status sf_check_device(uint32_t device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || (int)device >= ndev) {
    set_error("no usable HIP device; libtbcheck has no CPU fallback");
    return TBC_ERR_NO_DEVICE;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, (int)device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_error("device %u is not a gfx950 (MI355X) device", device);
    return TBC_ERR_NO_DEVICE;
  }
  return TBC_OK;
}

// Every rule of one key's inputs, on the host (the kernels trust them): the prefix search per row and "the latest row" rest on the
// documented orders; every offset and element number of the compact reads is checked (top == nullptr: the dense entry, no compact reads).
// exc_off and the rows' arrays start at the key's first read; `where` names the entry point (and the key).
bool sf_key_is_valid(const char* where, uint32_t E, uint32_t R, const uint32_t* add_invoke, const uint32_t* read_invoke, const uint32_t* top,
                     const uint64_t* exc_off, const uint32_t* exc, std::vector<uint32_t>& tmp) {
  for (uint32_t e = 1; e < E; e++)
    if (add_invoke[e] <= add_invoke[e - 1]) { set_error("%s: add_invoke must be strictly ascending (element %u)", where, e); return false; }
  for (uint32_t r = 0; r < R; r++) {
    if (r && read_invoke[r] <= read_invoke[r - 1]) { set_error("%s: read_invoke must be strictly ascending (read %u)", where, r); return false; }
    if (!top) continue;
    if (top[r] > E || exc_off[r + 1] < exc_off[r]) { set_error("%s read %u: bad top / exc_off (top %u, n_elements %u)", where, r, top[r], E); return false; }
    bool ascending = true;
    for (uint64_t i = exc_off[r]; i < exc_off[r + 1]; i++) {
      if (exc[i] >= E) { set_error("%s read %u: exception names element %u of %u", where, r, exc[i], E); return false; }
      if (i > exc_off[r] && exc[i] <= exc[i - 1]) ascending = false;
    }
    // each element at most once per read: the rows kernel FLIPS the listed bits, a duplicate would flip one back silently.  A strictly
    // ascending list (what the in-repo encoders write) is seen to be duplicate-free in one pass; a list in any other order is sorted
    // aside and looked at again (the header allows any order)
    if (ascending) continue;
    tmp.assign(exc + exc_off[r], exc + exc_off[r + 1]);
    std::sort(tmp.begin(), tmp.end());
    for (size_t i = 1; i < tmp.size(); i++)
      if (tmp[i] == tmp[i - 1]) { set_error("%s read %u lists element %u twice (each element at most once per read)", where, r, tmp[i]); return false; }
  }
  return true;
}

// enough chunks to fill the GPU with wavefronts that each stream a good stretch of rows; short chunks: what pass 2 walks again is one chunk
uint32_t sf_chunks(uint32_t WPR, uint32_t R) {
  const uint32_t col_blocks = std::max(1u, (WPR + 255) / 256);
  uint32_t chunks = std::max(1u, std::min(256u, 8192u / col_blocks));
  while (chunks > 1 && R / chunks < 64) chunks >>= 1;
  while ((R + chunks - 1) / chunks > kSetFullRows) chunks <<= 1;
  return chunks;
}

// The create behind all three entry points.  `in`: the keys' arrays end to end (tbc_setfull_keys_in; the single-key entries point it at
// their own one key), sumE / sumR its totals; `keyed`: name the key in a message.  `dense` (tbc_setfull_create only, one key): the
// caller's matrix is copied into the key's pitch where the other entries build the matrix from top / exc.  `ops`
// (tbc_setfull_keys_create_ops only): `in` holds what the host plan made of the ops (S->enc; no top / exc_off / exc), and the matrix is
// built from the reads' raw values `vals` by the kernels of set_full_encode.h -- in place of top / exc_off / exc the arena holds the
// element values, the rows' value slices, the keys' tables and the duplicate counters.
tbc_status sf_create(const char* fn, bool keyed, const tbc_setfull_keys_in* in, uint32_t sumE, uint32_t sumR, const tbc_setfull_in* dense, SfObject* S,
                     const int64_t* ops_vals = nullptr) {
  const uint32_t n = in->n_keys;
  const bool ops = S->from_ops;
  // ---- every rule, key by key, before any device call
  if (!dense && !ops && in->exc_off[0] != 0) { set_error("%s: exc_off[0] must be 0", fn); return TBC_ERR_INVALID_ARG; }
  {
    std::vector<uint32_t> tmp;
    char where[64];
    uint32_t e0 = 0, r0 = 0;
    for (uint32_t k = 0; k < n; e0 += in->n_elements[k], r0 += in->n_reads[k], k++) {
      if (keyed) std::snprintf(where, sizeof where, "%s: key %u", fn, k); else std::snprintf(where, sizeof where, "%s", fn);
      if (!sf_key_is_valid(where, in->n_elements[k], in->n_reads[k], in->add_invoke + e0, in->read_invoke + r0, dense || ops ? nullptr : in->top + r0,
                           dense || ops ? nullptr : in->exc_off + r0, in->exc, tmp))
        return TBC_ERR_INVALID_ARG;
    }
  }
  const tbc_status dev = sf_check_device(in->device);
  if (dev != TBC_OK) return dev;
  S->device = (int)in->device; S->n_keys = n; S->sumE = sumE; S->sumR = sumR;
  // ---- the plan: per key its chunking (a key of a few reads is one chunk) and its place in the arena's regions; per grid the first tile
  // of every key
  std::vector<SfKeyPlan> plan(n);
  std::vector<uint32_t> first((size_t)kFirsts * (n + 1), 0u);
  uint64_t m_words = 0, sum_words = 0, pmax_words = 0, tiles[kFirsts] = {};
  const auto up = [](uint64_t x, uint64_t a) { return (x + a - 1) / a * a; };
  uint32_t eb = 0, rb = 0;
  std::vector<SfEncKey> enc_keys;
  uint64_t tab_slots = 0;
  try { S->key_max.assign(n, -1); if (ops) enc_keys.assign(n, SfEncKey{}); } catch (const std::bad_alloc&) { set_error("%s: host memory", fn); return TBC_ERR_OOM; }
  for (uint32_t k = 0; k < n; k++) {
    SfKeyPlan& p = plan[k];
    p = SfKeyPlan{};
    p.E = in->n_elements[k]; p.R = in->n_reads[k]; p.elem_base = eb; p.row_base = rb;
    // (PITCH: the words between two rows in device memory.  A pitch padded off the power of two was measured -- 16 .. 1,088 words: the
    // same scan within 3 % either way, profiles/r06_setfull_pad_scan.txt -- so it is the words of a row, rounded up to four)
    p.WPR = (p.E + 31u) / 32u; p.PITCH = (p.WPR + 3u) / 4u * 4u;
    const bool scan = p.E && p.R;
    p.chunks = scan ? sf_chunks(p.WPR, p.R) : 1u; p.rows_per_chunk = std::max(1u, (p.R + p.chunks - 1) / p.chunks);
    p.any_gy = (p.PITCH / 4u + 255u) / 256u;
    m_words = up(m_words, 64); p.m_off = m_words; m_words += (uint64_t)p.R * p.PITCH;
    sum_words = up(sum_words, 64); p.sum_off = sum_words; sum_words += scan ? (uint64_t)p.chunks * p.PITCH : 0;
    p.pmax_off = (uint32_t)pmax_words; pmax_words += 2ull * p.chunks;
    const uint32_t nb = (p.WPR + 3u) / 4u;        // resolve: every key that has elements (one without reads: "nothing seen" is written there)
    first[kFirstRows * (n + 1) + k] = rb;
    first[kFirstPrefix * (n + 1) + k] = (uint32_t)tiles[kFirstPrefix]; tiles[kFirstPrefix] += scan ? (p.R + 255u) / 256u : 0u;
    first[kFirstAny * (n + 1) + k] = (uint32_t)tiles[kFirstAny]; tiles[kFirstAny] += scan ? (uint64_t)p.chunks * p.any_gy : 0u;
    if (nb && nb % 8u == 0u) tiles[kFirstResolve] = up(tiles[kFirstResolve], 8);
    first[kFirstResolve * (n + 1) + k] = (uint32_t)tiles[kFirstResolve]; tiles[kFirstResolve] += nb;
    first[kFirstSelect * (n + 1) + k] = (uint32_t)tiles[kFirstSelect]; tiles[kFirstSelect] += (p.E + kSelTile - 1u) / kSelTile;
    {   // (add_invoke and read_invoke ascend: their last entries are their greatest; add_ok may be TBC_NO_OP)
      int64_t mx = -1;
      if (p.E) mx = std::max<int64_t>(mx, in->add_invoke[eb + p.E - 1u]);
      for (uint32_t e = 0; e < p.E; e++) if (in->add_ok[eb + e] != kNoneU) mx = std::max<int64_t>(mx, in->add_ok[eb + e]);
      if (p.R) mx = std::max<int64_t>(mx, in->read_invoke[rb + p.R - 1u]);
      for (uint32_t r = 0; r < p.R; r++) mx = std::max<int64_t>(mx, in->read_ok[rb + r]);
      S->key_max[k] = mx;
    }
    S->bytes_matrix += (uint64_t)p.R * (dense ? dense->words_per_row : p.WPR) * 4;
    if (ops) {
      const uint64_t cap = sfenc::table_slots(p.E);
      enc_keys[k].tab_off = tab_slots; enc_keys[k].mask = cap ? (uint32_t)(cap - 1u) : 0u;
      tab_slots += cap;
    }
    eb += p.E; rb += p.R;
  }
  first[kFirstRows * (n + 1) + n] = rb;
  for (int g = kFirstPrefix; g < kFirsts; g++) first[(size_t)g * (n + 1) + n] = (uint32_t)tiles[g];
  if (pmax_words >= 0xFFFFFFFFull || tiles[kFirstAny] >= 0x7FFFFFFFull || tiles[kFirstResolve] >= 0x7FFFFFFFull) {
    set_error("%s: too many elements for one object", fn); return TBC_ERR_INVALID_ARG;
  }
  S->tiles_any = (uint32_t)tiles[kFirstAny]; S->tiles_resolve = (uint32_t)tiles[kFirstResolve]; S->tiles_select = (uint32_t)tiles[kFirstSelect];
  // ---- one arena (round 6: fourteen hipMalloc and as many hipFree -- each of which waits for the device -- were most of a caller's 5 ms
  // around a 0.16 ms scan; the reference checks one history per call site, set_full.clj:157, so create + run + destroy IS its time to
  // verdict): what the host makes (plan, first tiles, the prefix extremes' start values), the caller's arrays, then what the device makes
  const uint64_t ne = dense || ops ? 0 : in->exc_off[sumR];
  const size_t top4 = dense || ops ? 0 : (size_t)sumR * 4, off8 = dense || ops ? 0 : ((size_t)sumR + 1) * 8;
  size_t cursor = 0;
  const auto take = [&](size_t bytes) { const size_t at = cursor; cursor += (bytes + 255) & ~(size_t)255; return at; };
  const size_t o_plan = take(sizeof(SfKeyPlan) * n), o_first = take(first.size() * 4), o_pm = take(pmax_words * 4);
  const size_t o_enc = take(sizeof(SfEncKey) * enc_keys.size());
  const size_t head_bytes = cursor;
  const size_t o_ai = take((size_t)sumE * 4), o_ao = take((size_t)sumE * 4), o_ri = take((size_t)sumR * 4), o_ro = take((size_t)sumR * 4),
               o_top = take(top4), o_off = take(off8), o_exc = take(ne * 4);
  const size_t o_M = take(m_words * 4), o_P = take((size_t)sumR * 4), o_any = take(sum_words * 8);
  const size_t o_out = take((size_t)sumE * 12), o_w = take(kCounterBytes);
  // (tbc_setfull_keys_create_ops) the element values and the rows' value slices; then what starts as zeros, side by side: the tables, the
  // rows' and keys' flags, the unknown counts, the repeat counter, cnt, dup_max, dup_count
  const size_t o_el = take(ops ? (size_t)sumE * 8 : 0), o_vlo = take(ops ? (size_t)sumR * 8 : 0), o_vhi = take(ops ? (size_t)sumR * 8 : 0);
  const size_t o_slots = take(tab_slots * sizeof(SfEncSlot)), o_rflag = take(ops ? sumR : 0), o_kflag = take(ops ? (size_t)n * 4 : 0),
               o_unk = take(ops ? (size_t)n * 8 : 0), o_rep = take(ops ? 4 : 0), o_cnt = take(ops ? (size_t)sumE * 4 : 0),
               o_dmax = take(ops ? (size_t)sumE * 4 : 0), o_dcnt = take(ops ? (size_t)n * 4 : 0);
  const size_t enc_zero_bytes = cursor - o_slots;
  std::vector<unsigned char> img;
  try { img.assign(head_bytes, 0); } catch (const std::bad_alloc&) { set_error("%s: host memory", fn); return TBC_ERR_OOM; }
  std::memcpy(img.data() + o_plan, plan.data(), sizeof(SfKeyPlan) * n);
  std::memcpy(img.data() + o_first, first.data(), first.size() * 4);
  if (ops) std::memcpy(img.data() + o_enc, enc_keys.data(), sizeof(SfEncKey) * n);
  for (uint32_t k = 0; k < n; k++)        // the chunks' greatest prefixes start at 0, their least at ~0 (the minima lie behind the maxima)
    std::memset(img.data() + o_pm + ((size_t)plan[k].pmax_off + plan[k].chunks) * 4, 0xFF, (size_t)plan[k].chunks * 4);
  SF_TRY(hipSetDevice(S->device));
  SF_TRY(hipMalloc(&S->arena, std::max<size_t>(cursor, 256)));
  char* const A0 = static_cast<char*>(S->arena);
  S->d_plan = (SfKeyPlan*)(A0 + o_plan); S->d_first = (uint32_t*)(A0 + o_first); S->d_pmax = (uint32_t*)(A0 + o_pm); S->d_add_ok = (uint32_t*)(A0 + o_ao);
  S->d_read_invoke = (uint32_t*)(A0 + o_ri); S->d_read_ok = (uint32_t*)(A0 + o_ro); S->d_M = (uint32_t*)(A0 + o_M); S->d_P = (uint32_t*)(A0 + o_P);
  S->d_anyp = (uint32_t*)(A0 + o_any); S->d_anya = S->d_anyp + sum_words;
  S->d_out = (uint32_t*)(A0 + o_out); S->d_words = (unsigned long long*)(A0 + o_w);
  SF_TRY(hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking));
  SF_TRY(hipEventCreate(&S->ev0)); SF_TRY(hipEventCreate(&S->ev1));
  // Each of the caller's arrays straight to its place in the arena: eight copies whatever n_keys is.  (Packing them into the host image
  // first -- one H2D -- gains 0.04-0.09 ms on objects below ~1 MB and loses from ~1.5 MB on, 0.8 ms at the bench key's 13 MB and 3 ms at
  // 256 keys x 2k ops; the direct copies alone hold the parent's end-to-end time at every shape measured: DESIGN.md K7.)  The copies
  // read pageable memory of the caller's: the synchronise below ends them before create returns.
  const auto put = [&](size_t at, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(A0 + at, src, bytes, hipMemcpyHostToDevice, S->stream) : hipSuccess;
  };
  SF_TRY(put(o_ai, in->add_invoke, (size_t)sumE * 4)); SF_TRY(put(o_ao, in->add_ok, (size_t)sumE * 4));
  SF_TRY(put(o_ri, in->read_invoke, (size_t)sumR * 4)); SF_TRY(put(o_ro, in->read_ok, (size_t)sumR * 4));
  SF_TRY(put(o_top, in->top, top4)); SF_TRY(put(o_off, in->exc_off, off8)); SF_TRY(put(o_exc, in->exc, ne * 4));
  SF_TRY(hipMemcpyAsync(A0, img.data(), img.size(), hipMemcpyHostToDevice, S->stream));
  if (sum_words) SF_TRY(hipMemsetAsync(S->d_anyp, 0, sum_words * 8, S->stream));     // (the tiles below the diagonal never write theirs)
  // ---- the matrix: the caller's, copied into the key's pitch (its padding zeroed: no word the scan loads is left unset; words of the
  // caller's rows past the key's are ignored), or built from the compact reads
  if (dense && plan[0].R && plan[0].WPR) {
    const SfKeyPlan& p = plan[0];
    if (p.PITCH > p.WPR) SF_TRY(hipMemset2DAsync(S->d_M + p.WPR, (size_t)p.PITCH * 4, 0, (size_t)(p.PITCH - p.WPR) * 4, p.R, S->stream));
    SF_TRY(hipMemcpy2DAsync(S->d_M, (size_t)p.PITCH * 4, dense->present, (size_t)dense->words_per_row * 4, (size_t)p.WPR * 4, p.R, hipMemcpyHostToDevice, S->stream));
  } else if (ops) {
    SfEncArgs E;
    E.plan = S->d_plan; E.first = S->d_first; E.enc = (const SfEncKey*)(A0 + o_enc); E.n_keys = n; E.R_all = sumR; E.E_all = sumE;
    E.grid = std::min<uint32_t>(sumR, 16384u);
    E.element = (const long long*)(A0 + o_el); E.slots = (SfEncSlot*)(A0 + o_slots);
    E.val_lo = (const unsigned long long*)(A0 + o_vlo); E.val_hi = (const unsigned long long*)(A0 + o_vhi);
    E.M = S->d_M; E.row_flag = (uint8_t*)(A0 + o_rflag); E.key_flag = (uint32_t*)(A0 + o_kflag); E.unknown = (unsigned long long*)(A0 + o_unk);
    E.repeats = (uint32_t*)(A0 + o_rep); E.cnt = (uint32_t*)(A0 + o_cnt); E.dup_max = (uint32_t*)(A0 + o_dmax); E.dup_count = (uint32_t*)(A0 + o_dcnt);
    const uint64_t nv = S->enc.n_values;
    if (nv) SF_TRY(hipMalloc(&S->d_vals, nv * 8));
    E.vals = (const long long*)S->d_vals;
    SF_TRY(hipEventCreate(&S->ev_e0)); SF_TRY(hipEventCreate(&S->ev_e1));
    SF_TRY(put(o_el, S->enc.element.data(), (size_t)sumE * 8));
    SF_TRY(put(o_vlo, S->enc.val_lo.data(), (size_t)sumR * 8)); SF_TRY(put(o_vhi, S->enc.val_hi.data(), (size_t)sumR * 8));
    if (nv) SF_TRY(hipMemcpyAsync(S->d_vals, ops_vals, nv * 8, hipMemcpyHostToDevice, S->stream));
    SF_TRY(hipMemsetAsync(A0 + o_slots, 0, enc_zero_bytes, S->stream));
    SF_TRY(hipEventRecord(S->ev_e0, S->stream));
    if (sumE) hipLaunchKernelGGL(sf_table_build_kernel, dim3((sumE + 255u) / 256u), dim3(256), 0, S->stream, E);
    if (sumR) hipLaunchKernelGGL(sf_values_kernel<TBC_SETFULL_ENCODE_WINDOW_WORDS>, dim3(E.grid), dim3(256), 0, S->stream, E);
    SF_TRY(hipGetLastError());
    SF_TRY(hipEventRecord(S->ev_e1, S->stream));
    // the repeat counter back: only a history with a duplicated element pays for the exact pass
    SF_TRY(hipMemcpyAsync(&S->h_repeats, E.repeats, 4, hipMemcpyDeviceToHost, S->stream));
    SF_TRY(hipStreamSynchronize(S->stream));
    float ms = 0, ms_d = 0;
    SF_TRY(hipEventElapsedTime(&ms, S->ev_e0, S->ev_e1));
    if (S->h_repeats) {
      SF_TRY(hipEventCreate(&S->ev_d0)); SF_TRY(hipEventCreate(&S->ev_d1));
      SF_TRY(hipEventRecord(S->ev_d0, S->stream));
      hipLaunchKernelGGL(sf_dups_kernel, dim3(n), dim3(256), 0, S->stream, E);
      SF_TRY(hipGetLastError());
      SF_TRY(hipEventRecord(S->ev_d1, S->stream));
    }
    try { S->dup_max.assign(sumE, 0u); S->dup_count.assign(n, 0u); S->unknown.assign(n, 0ull); }
    catch (const std::bad_alloc&) { set_error("%s: host memory", fn); return TBC_ERR_OOM; }
    if (S->h_repeats) {
      if (sumE) SF_TRY(hipMemcpyAsync(S->dup_max.data(), E.dup_max, (size_t)sumE * 4, hipMemcpyDeviceToHost, S->stream));
      SF_TRY(hipMemcpyAsync(S->dup_count.data(), E.dup_count, (size_t)n * 4, hipMemcpyDeviceToHost, S->stream));
    }
    SF_TRY(hipMemcpyAsync(S->unknown.data(), E.unknown, (size_t)n * 8, hipMemcpyDeviceToHost, S->stream));
    SF_TRY(hipStreamSynchronize(S->stream));
    if (S->h_repeats) SF_TRY(hipEventElapsedTime(&ms_d, S->ev_d0, S->ev_d1));
    S->ns_encode = (uint64_t)((ms + ms_d) * 1e6);
    if (S->d_vals) { SF_TRY(hipFree(S->d_vals)); S->d_vals = nullptr; }
  } else if (!dense && sumR) {
    hipLaunchKernelGGL(setfull_rows_kernel, dim3(std::min<uint32_t>(sumR, 16384u)), dim3(256), 0, S->stream, S->d_plan, S->d_first, n, sumR,
                       (const uint32_t*)(A0 + o_top), (const unsigned long long*)(A0 + o_off), (const uint32_t*)(A0 + o_exc), S->d_M);
  }
  // p[r] (how many elements had been invoked when read r completed) and the chunks' extremes depend on the inputs only
  if (tiles[kFirstPrefix])
    hipLaunchKernelGGL(setfull_prefix_kernel, dim3((uint32_t)tiles[kFirstPrefix]), dim3(256), 0, S->stream, S->d_plan, S->d_first, n,
                       (const uint32_t*)(A0 + o_ai), S->d_read_ok, S->d_P, S->d_pmax);
  SF_TRY(hipGetLastError());
  SF_TRY(hipStreamSynchronize(S->stream));
  return TBC_OK;
}

template <class Handle>
tbc_status sf_new(const char* fn, bool keyed, const tbc_setfull_keys_in* in, uint32_t sumE, uint32_t sumR, const tbc_setfull_in* dense, Handle** handle) {
  SfObject* S = new (std::nothrow) SfObject();
  if (!S) return TBC_ERR_OOM;
  const tbc_status st = sf_create(fn, keyed, in, sumE, sumR, dense, S);
  if (st != TBC_OK) { delete S; return st; }
  *handle = reinterpret_cast<Handle*>(S);
  return TBC_OK;
}

// The run behind both: the scan's two launches between the events, then the results (n_elements each, key after key) and the counters back,
// each array straight into the caller's
// the scan's two launches between its events (ev0, ev1), on the object's stream: what run and results share
tbc_status sf_scan(SfObject* S) {
  hipStream_t s = S->stream;
  const uint32_t n = S->n_keys;
  uint32_t* const d_known = S->d_out; uint32_t* const d_lp = S->d_out + S->sumE; uint32_t* const d_la = S->d_out + 2ull * S->sumE;
  SF_TRY(hipMemsetAsync(S->d_words, 0, kCounterBytes, s));
  SF_TRY(hipEventRecord(S->ev0, s));
  if (S->tiles_any)
    hipLaunchKernelGGL(setfull_any_kernel, dim3(S->tiles_any), dim3(256), 0, s, S->d_plan, S->d_first, n, S->d_M, S->d_P, S->d_pmax,
                       S->d_anyp, S->d_anya, S->d_words);
  if (S->tiles_resolve)
    hipLaunchKernelGGL(setfull_resolve_kernel, dim3(S->tiles_resolve), dim3(256), 0, s, S->d_plan, S->d_first, n, S->d_M, S->d_P, S->d_read_invoke,
                       S->d_read_ok, S->d_anyp, S->d_anya, S->d_add_ok, d_lp, d_la, d_known, S->d_words);
  SF_TRY(hipGetLastError());
  SF_TRY(hipEventRecord(S->ev1, s));
  return TBC_OK;
}

tbc_status sf_run(SfObject* S, uint32_t* known, uint32_t* last_present, uint32_t* last_absent, uint64_t* ns_scan, uint64_t* bytes_scanned, uint64_t* bytes_matrix) {
  SF_TRY(hipSetDevice(S->device));
  hipStream_t s = S->stream;
  const size_t e4 = (size_t)S->sumE * 4;
  uint32_t* const d_known = S->d_out; uint32_t* const d_lp = S->d_out + S->sumE; uint32_t* const d_la = S->d_out + 2ull * S->sumE;
  { const tbc_status st = sf_scan(S); if (st != TBC_OK) return st; }
  if (e4) {
    SF_TRY(hipMemcpyAsync(known, d_known, e4, hipMemcpyDeviceToHost, s));
    SF_TRY(hipMemcpyAsync(last_present, d_lp, e4, hipMemcpyDeviceToHost, s));
    SF_TRY(hipMemcpyAsync(last_absent, d_la, e4, hipMemcpyDeviceToHost, s));
  }
  SF_TRY(hipMemcpyAsync(S->h_words, S->d_words, kCounterBytes, hipMemcpyDeviceToHost, s));
  SF_TRY(hipStreamSynchronize(s));
  float ms = 0;
  SF_TRY(hipEventElapsedTime(&ms, S->ev0, S->ev1));
  unsigned long long words = 0;
  for (uint32_t k = 0; k < kWordCounters; k++) words += S->h_words[16u * k];
  *ns_scan = (uint64_t)(ms * 1e6);
  *bytes_scanned = (uint64_t)words * 4;
  *bytes_matrix = S->bytes_matrix;
  return TBC_OK;
}

// The results behind both handles: every rule of the call on the host first; then the times up, the scan, the deciding passes
// (set_full_results.h) between their own events, and the arrays and summaries back, each straight into the caller's.
tbc_status sf_results(const char* fn, SfObject* S, const tbc_setfull_times* times, tbc_setfull_results_out* out) {
  if (!S || !times || !out || !out->summary || (S->sumE && (!out->outcome || !out->stable_latency || !out->lost_latency)) ||
      (times->op_time && !times->time_off)) {
    set_error("%s: null argument", fn);
    return TBC_ERR_INVALID_ARG;
  }
  if (times->unit == 0) { set_error("%s: unit is 0", fn); return TBC_ERR_INVALID_ARG; }
  if (times->reserved0 != 0 || (times->flags & ~TBC_SETFULL_F_LINEARIZABLE)) { set_error("%s: unknown flags / reserved0 not 0", fn); return TBC_ERR_INVALID_ARG; }
  const uint32_t n = S->n_keys;
  uint64_t T = 0;
  if (times->op_time) {
    for (uint32_t k = 0; k < n; k++) {
      const uint64_t a = times->time_off[k], b = times->time_off[k + 1];
      if (b < a || (S->key_max[k] >= 0 && b - a <= (uint64_t)S->key_max[k])) {
        set_error("%s: key %u: %llu times, but the key's inputs name op %lld", fn, k, (unsigned long long)(b < a ? 0 : b - a), (long long)S->key_max[k]);
        return TBC_ERR_INVALID_ARG;
      }
    }
    if (times->time_off[0] != 0) { set_error("%s: key 0: time_off[0] must be 0", fn); return TBC_ERR_INVALID_ARG; }
    T = times->time_off[n];
  }
  SF_TRY(hipSetDevice(S->device));
  hipStream_t s = S->stream;
  const size_t sumE = S->sumE;
  // ---- the results' arena: accumulators, select state, histograms, summaries | offsets, per-element arrays, times
  size_t cursor = 0;
  const auto take = [&](size_t bytes) { const size_t at = cursor; cursor += (bytes + 255) & ~(size_t)255; return at; };
  const size_t o_acc = take(sizeof(SfKeyAcc) * n), o_sel = take(sizeof(SfSel) * kSelTargets * n), o_hist = take((size_t)4 * kSelTargets * kSelBins * n),
               o_sum = take(sizeof(tbc_setfull_key_summary) * n), o_toff = take((size_t)8 * (n + 1)), o_oc = take(sumE), o_sl = take(sumE * 8),
               o_ll = take(sumE * 8), o_time = take((size_t)std::max<uint64_t>(T, S->res_times) * 8);
  if (!S->res_arena || T > S->res_times) {
    if (S->res_arena) { SF_TRY(hipStreamSynchronize(s)); SF_TRY(hipFree(S->res_arena)); S->res_arena = nullptr; }
    SF_TRY(hipMalloc(&S->res_arena, std::max<size_t>(cursor, 256)));
    S->res_times = std::max<uint64_t>(T, S->res_times);
    SF_TRY(hipMemsetAsync(S->res_arena, 0, o_toff, s));         // (select state and histograms start at zero; every pick leaves its histogram zeroed)
    if (!S->ev2) { SF_TRY(hipEventCreate(&S->ev2)); SF_TRY(hipEventCreate(&S->ev3)); }
  }
  char* const R0 = static_cast<char*>(S->res_arena);
  SfResArgs A;
  A.plan = S->d_plan; A.first = S->d_first; A.n_keys = n; A.flags = times->flags;
  A.known = S->d_out; A.lp = S->d_out + S->sumE; A.la = S->d_out + 2ull * S->sumE;
  A.op_time = times->op_time ? (const long long*)(R0 + o_time) : nullptr;
  A.time_off = (const unsigned long long*)(R0 + o_toff);
  A.unit = times->op_time ? times->unit : 1ull;
  A.outcome = (uint8_t*)(R0 + o_oc); A.slat = (long long*)(R0 + o_sl); A.llat = (long long*)(R0 + o_ll);
  A.acc = (SfKeyAcc*)(R0 + o_acc); A.sel = (SfSel*)(R0 + o_sel); A.hist = (uint32_t*)(R0 + o_hist); A.summary = (tbc_setfull_key_summary*)(R0 + o_sum);
  if (times->op_time) {
    SF_TRY(hipMemcpyAsync(R0 + o_toff, times->time_off, (size_t)8 * (n + 1), hipMemcpyHostToDevice, s));
    if (T) SF_TRY(hipMemcpyAsync(R0 + o_time, times->op_time, (size_t)T * 8, hipMemcpyHostToDevice, s));
  }
  { const tbc_status st = sf_scan(S); if (st != TBC_OK) return st; }
  SF_TRY(hipEventRecord(S->ev2, s));
  const uint32_t key_blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(sf_results_init_kernel, dim3(key_blocks), dim3(256), 0, s, A);
  if (S->tiles_select) {
    hipLaunchKernelGGL(sf_decide_kernel, dim3(S->tiles_select), dim3(256), 0, s, A);
    for (uint32_t level = 8; level-- > 0;) {
      hipLaunchKernelGGL(sf_select_hist_kernel, dim3(S->tiles_select), dim3(256), 0, s, A, level);
      hipLaunchKernelGGL(sf_select_pick_kernel, dim3(n), dim3(kSelTargets * 64), 0, s, A, level);
    }
    hipLaunchKernelGGL(sf_worst_collect_kernel, dim3(S->tiles_select), dim3(256), 0, s, A);
  }
  hipLaunchKernelGGL(sf_results_final_kernel, dim3(key_blocks), dim3(256), 0, s, A);
  SF_TRY(hipGetLastError());
  SF_TRY(hipEventRecord(S->ev3, s));
  if (sumE) {
    SF_TRY(hipMemcpyAsync(out->outcome, A.outcome, sumE, hipMemcpyDeviceToHost, s));
    SF_TRY(hipMemcpyAsync(out->stable_latency, A.slat, sumE * 8, hipMemcpyDeviceToHost, s));
    SF_TRY(hipMemcpyAsync(out->lost_latency, A.llat, sumE * 8, hipMemcpyDeviceToHost, s));
    if (out->known) SF_TRY(hipMemcpyAsync(out->known, A.known, sumE * 4, hipMemcpyDeviceToHost, s));
    if (out->last_present) SF_TRY(hipMemcpyAsync(out->last_present, A.lp, sumE * 4, hipMemcpyDeviceToHost, s));
    if (out->last_absent) SF_TRY(hipMemcpyAsync(out->last_absent, A.la, sumE * 4, hipMemcpyDeviceToHost, s));
  }
  SF_TRY(hipMemcpyAsync(out->summary, A.summary, sizeof(tbc_setfull_key_summary) * n, hipMemcpyDeviceToHost, s));
  SF_TRY(hipMemcpyAsync(S->h_words, S->d_words, kCounterBytes, hipMemcpyDeviceToHost, s));
  SF_TRY(hipStreamSynchronize(s));
  float ms_scan = 0, ms_res = 0;
  SF_TRY(hipEventElapsedTime(&ms_scan, S->ev0, S->ev1));
  SF_TRY(hipEventElapsedTime(&ms_res, S->ev2, S->ev3));
  unsigned long long words = 0;
  for (uint32_t k = 0; k < kWordCounters; k++) words += S->h_words[16u * k];
  out->ns_scan = (uint64_t)(ms_scan * 1e6);
  out->ns_results = (uint64_t)(ms_res * 1e6);
  out->bytes_scanned = (uint64_t)words * 4;
  out->bytes_matrix = S->bytes_matrix;
  return TBC_OK;
}

void sf_destroy(SfObject* S) {
  if (!S) return;
  (void)hipSetDevice(S->device);
  delete S;
}

}  // namespace

extern "C" {

tbc_status tbc_setfull_create(const tbc_setfull_in* in, tbc_setfull** handle) {
  const char* fn = "tbc_setfull_create";
  if (!in || !handle || (in->n_elements && (!in->add_invoke || !in->add_ok)) ||
      (in->n_reads && (!in->read_invoke || !in->read_ok || !in->present))) {
    set_error("%s: null argument", fn);
    return TBC_ERR_INVALID_ARG;
  }
  if ((uint64_t)in->words_per_row * 32 < in->n_elements) { set_error("%s: words_per_row too small for n_elements", fn); return TBC_ERR_INVALID_ARG; }
  const tbc_setfull_keys_in one = {1u, in->device, &in->n_elements, &in->n_reads, in->add_invoke, in->add_ok, in->read_invoke, in->read_ok, nullptr, nullptr, nullptr};
  return sf_new(fn, false, &one, in->n_elements, in->n_reads, in, handle);
}

tbc_status tbc_setfull_create_rows(const tbc_setfull_rows* in, tbc_setfull** handle) {
  const char* fn = "tbc_setfull_create_rows";
  if (!in || !handle || (in->n_elements && (!in->add_invoke || !in->add_ok)) ||
      (in->n_reads && (!in->read_invoke || !in->read_ok || !in->top)) || !in->exc_off || (in->exc_off[in->n_reads] && !in->exc) || in->reserved0 != 0) {
    set_error("%s: null argument", fn);
    return TBC_ERR_INVALID_ARG;
  }
  const tbc_setfull_keys_in one = {1u, in->device, &in->n_elements, &in->n_reads, in->add_invoke, in->add_ok, in->read_invoke, in->read_ok, in->top, in->exc_off, in->exc};
  return sf_new(fn, false, &one, in->n_elements, in->n_reads, nullptr, handle);
}

tbc_status tbc_setfull_keys_create(const tbc_setfull_keys_in* in, tbc_setfull_keys** handle) {
  const char* fn = "tbc_setfull_keys_create";
  if (!in || !handle) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  if (in->n_keys == 0) { set_error("%s: n_keys is 0", fn); return TBC_ERR_INVALID_ARG; }
  if (!in->n_elements || !in->n_reads || !in->exc_off) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  uint64_t sumE = 0, sumR = 0;
  for (uint32_t k = 0; k < in->n_keys; k++) { sumE += in->n_elements[k]; sumR += in->n_reads[k]; }
  if (sumE >= 0xFFFFFFFFull || sumR >= 0xFFFFFFFFull) { set_error("%s: more than 2^32 - 2 elements or reads in one object", fn); return TBC_ERR_INVALID_ARG; }
  if ((sumE && (!in->add_invoke || !in->add_ok)) || (sumR && (!in->read_invoke || !in->read_ok || !in->top)) || (in->exc_off[sumR] && !in->exc)) {
    set_error("%s: null argument", fn);
    return TBC_ERR_INVALID_ARG;
  }
  return sf_new(fn, true, in, (uint32_t)sumE, (uint32_t)sumR, nullptr, handle);
}

tbc_status tbc_setfull_run(tbc_setfull* handle, tbc_setfull_out* out) {
  SfObject* const S = sf_obj(handle);
  if (!S || !out || (S->sumE && (!out->known || !out->last_present || !out->last_absent))) { set_error("tbc_setfull_run: null argument"); return TBC_ERR_INVALID_ARG; }
  return sf_run(S, out->known, out->last_present, out->last_absent, &out->ns_scan, &out->bytes_scanned, &out->bytes_matrix);
}

tbc_status tbc_setfull_keys_run(tbc_setfull_keys* handle, tbc_setfull_keys_out* out) {
  SfObject* const S = sf_obj(handle);
  if (!S || !out || (S->sumE && (!out->known || !out->last_present || !out->last_absent))) { set_error("tbc_setfull_keys_run: null argument"); return TBC_ERR_INVALID_ARG; }
  return sf_run(S, out->known, out->last_present, out->last_absent, &out->ns_scan, &out->bytes_scanned, &out->bytes_matrix);
}

tbc_status tbc_setfull_results(tbc_setfull* handle, const tbc_setfull_times* times, tbc_setfull_results_out* out) {
  return sf_results("tbc_setfull_results", sf_obj(handle), times, out);
}
tbc_status tbc_setfull_keys_results(tbc_setfull_keys* handle, const tbc_setfull_times* times, tbc_setfull_results_out* out) {
  return sf_results("tbc_setfull_keys_results", sf_obj(handle), times, out);
}

tbc_status tbc_setfull_keys_create_ops(const tbc_setfull_ops_in* in, tbc_setfull_keys** handle) {
  const char* fn = "tbc_setfull_keys_create_ops";
  if (!in || !handle) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  if (in->n_keys == 0) { set_error("%s: n_keys is 0", fn); return TBC_ERR_INVALID_ARG; }
  if (!in->op_off || !in->index || !in->type || !in->f || !in->process || !in->value || !in->val_off || !in->vals) {
    set_error("%s: null argument (every pointer of tbc_setfull_ops_in must be set)", fn);
    return TBC_ERR_INVALID_ARG;
  }
  SfObject* S = new (std::nothrow) SfObject();
  if (!S) return TBC_ERR_OOM;
  tbc_status st = TBC_OK;
  try {
    std::string err;
    if (!sfenc::validate(fn, in, err)) { set_error("%s", err.c_str()); st = TBC_ERR_INVALID_ARG; }
    if (st == TBC_OK) {
      sfenc::plan(in, S->enc);
      if (S->enc.element.size() >= 0xFFFFFFFFull || S->enc.read_ok.size() >= 0xFFFFFFFFull) {
        set_error("%s: more than 2^32 - 2 elements or reads in one object", fn); st = TBC_ERR_INVALID_ARG;
      }
    }
  } catch (const std::bad_alloc&) { set_error("%s: host memory", fn); st = TBC_ERR_OOM; }
  if (st == TBC_OK) {
    const sfenc::Plan& P = S->enc;
    S->from_ops = true;
    const tbc_setfull_keys_in made = {in->n_keys, in->device, P.n_elements.data(), P.n_reads.data(), P.add_invoke.data(), P.add_ok.data(),
                                      P.read_invoke.data(), P.read_ok.data(), nullptr, nullptr, nullptr};
    st = sf_create(fn, true, &made, (uint32_t)P.element.size(), (uint32_t)P.read_ok.size(), nullptr, S, in->vals);
  }
  if (st != TBC_OK) { delete S; return st; }
  *handle = reinterpret_cast<tbc_setfull_keys*>(S);
  return TBC_OK;
}

tbc_status tbc_setfull_keys_shape(tbc_setfull_keys* h, uint64_t* sum_elements, uint64_t* sum_reads) {
  SfObject* const S = sf_obj(h);
  if (!S || !sum_elements || !sum_reads) { set_error("tbc_setfull_keys_shape: null argument"); return TBC_ERR_INVALID_ARG; }
  *sum_elements = S->sumE; *sum_reads = S->sumR;
  return TBC_OK;
}

tbc_status tbc_setfull_keys_encoding(tbc_setfull_keys* h, tbc_setfull_encoding* out) {
  SfObject* const S = sf_obj(h);
  if (!S || !out) { set_error("tbc_setfull_keys_encoding: null argument"); return TBC_ERR_INVALID_ARG; }
  if (!S->from_ops) {
    set_error("tbc_setfull_keys_encoding: the object was not made from ops (tbc_setfull_keys_create_ops): its caller has the encoding");
    return TBC_ERR_INVALID_ARG;
  }
  const sfenc::Plan& P = S->enc;
  const auto give = [](auto* dst, const auto& src) { if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(src[0])); };
  give(out->n_elements, P.n_elements); give(out->n_reads, P.n_reads); give(out->element, P.element);
  give(out->add_invoke, P.add_invoke); give(out->add_ok, P.add_ok); give(out->read_invoke, P.read_invoke); give(out->read_ok, P.read_ok);
  give(out->dup_max, S->dup_max); give(out->dup_count, S->dup_count); give(out->unknown_values, S->unknown);
  out->ns_encode = S->ns_encode;
  return TBC_OK;
}

void tbc_setfull_destroy(tbc_setfull* handle) { sf_destroy(sf_obj(handle)); }
void tbc_setfull_keys_destroy(tbc_setfull_keys* handle) { sf_destroy(sf_obj(handle)); }

}  // extern "C"
