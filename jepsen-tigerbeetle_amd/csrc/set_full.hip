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
// fills a sliver of the GPU.  Every launch goes through the plan table (set_full_plan.h); create = rows + prefix, run = any + resolve, whatever
// n_keys is.
//
// This unit holds the scan kernels and the four functions that launch them (set_full_scan.h), and nothing else: the object, create, run,
// results and the C entry points are set_full_host.hip, the plan every launch goes through is made by set_full_plan.h.  (bench.py quotes
// measured HBM traffic only for the very bytes of this file they were taken on: host changes do not touch it.)
#include <hip/hip_runtime.h>
#include <cstdint>
#include "set_full_plan.h"
#include "set_full_scan.h"

namespace {

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

}  // namespace

void sf_launch_prefix(hipStream_t s, uint32_t grid, const void* plan, const uint32_t* first, uint32_t n_keys, const uint32_t* add_invoke,
                      const uint32_t* read_ok, uint32_t* P, uint32_t* pmax) {
  hipLaunchKernelGGL(setfull_prefix_kernel, dim3(grid), dim3(256), 0, s, (const SfKeyPlan*)plan, first, n_keys, add_invoke, read_ok, P, pmax);
}

void sf_launch_rows(hipStream_t s, uint32_t grid, const void* plan, const uint32_t* first, uint32_t n_keys, uint32_t R_all, const uint32_t* top,
                    const unsigned long long* exc_off, const uint32_t* exc, uint32_t* M) {
  hipLaunchKernelGGL(setfull_rows_kernel, dim3(grid), dim3(256), 0, s, (const SfKeyPlan*)plan, first, n_keys, R_all, top, exc_off, exc, M);
}

void sf_launch_any(hipStream_t s, uint32_t grid, const void* plan, const uint32_t* first, uint32_t n_keys, const uint32_t* M, const uint32_t* P,
                   const uint32_t* pmax, uint32_t* any_p, uint32_t* any_a, unsigned long long* words_loaded) {
  hipLaunchKernelGGL(setfull_any_kernel, dim3(grid), dim3(256), 0, s, (const SfKeyPlan*)plan, first, n_keys, M, P, pmax, any_p, any_a, words_loaded);
}

void sf_launch_resolve(hipStream_t s, uint32_t grid, const void* plan, const uint32_t* first, uint32_t n_keys, const uint32_t* M, const uint32_t* P,
                       const uint32_t* read_invoke, const uint32_t* read_ok, const uint32_t* any_p, const uint32_t* any_a, const uint32_t* add_ok,
                       uint32_t* lp, uint32_t* la, uint32_t* known, unsigned long long* words_loaded) {
  hipLaunchKernelGGL(setfull_resolve_kernel, dim3(grid), dim3(256), 0, s, (const SfKeyPlan*)plan, first, n_keys, M, P, read_invoke, read_ok, any_p, any_a,
                     add_ok, lp, la, known, words_loaded);
}
