// perf_kernels.h -- the O(ops) part of tbc_perf_series on the MI355X (gfx950): the kernel bodies.  perf.hip compiles them into
// libtbcheck.so; their launches are pf::sequence at the end of this file; the host plan (the partner column, t_max, the cell
// numbering, the chunks, the arena) is perf_plan.h.
// In launch order -- the kernel boundary is the only ordering between them, no kernel holds an agent-scope fence, none uses scratch:
//
//   pf_classify_kernel      lane = op (grid-stride).  Outcome (an invocation's: its partner's type; a completion's: its own), latency
//                           (partner's time - own, matched invocations only), the bucket of the op's own time.  Stores op_latency and
//                           op_outcome; counts the rate cells (f, type, bucket of a completion) and the sizes of the quantile cells
//                           (f, bucket of a matched invocation): per wavefront the lanes of one cell are counted by ballot + popcount
//                           and their first lane adds them, ONE atomic per wavefront and distinct cell -- a wavefront of 64 consecutive
//                           ops mostly sits in one second and a handful of f's.
//   the open scan           the running count per class (f, outcome) in history order, +1 at an invocation, -1 at a completion.  A
//                           WORKGROUP SCAN WITH CARRIED PER-CLASS TOTALS, not a decoupled look-back: a look-back spins on its
//                           predecessors' flags behind agent-scope fences, which on eight XCDs write an L2 back each, and the classes
//                           make its flag a row of n_class words.  Instead the history is cut into chunks of whole wavefronts, a
//                           wavefront-sized workgroup per chunk (grid-stride), and the kernel boundary orders three passes:
//     pf_open_totals_kernel   per chunk and class the chunk's net change, into the chunk's row of `carry` (per step and distinct class
//                             of the wavefront: two ballots, one atomic)
//     pf_open_carry_kernel    a workgroup per class (grid-stride): its column of `carry` scanned exclusively down the chunks, 256 a step
//     pf_open_scan_kernel     per chunk again, 64 ops a step: per distinct class the first lane takes the class's carried total and
//                             adds the step's net change (one atomic with return on the chunk's own row), every lane of the class
//                             adds the popcounts of the invocations and completions at or below it: op_open_after.  The LAST op per
//                             (class, bucket) is kept by one 64-bit atomic max of (op number + 1) << 32 | the count's 32 bits: the op
//                             number alone decides, 0 = no op.
//   the cell gather         pf_cell_sum_kernel (per 256 cells their sum, and the greatest cell), pf_tile_scan_kernel (ONE workgroup:
//                           the tiles' sums scanned, 256 a step with a carried base), pf_cell_offsets_kernel (each tile scanned again
//                           from its base: q_off, and a cursor per cell), pf_gather_kernel (lane = op: a matched invocation claims the
//                           next place of its cell and stores its latency there as an order-preserving unsigned key -- a counting
//                           sort; the order inside a cell is whatever the atomics give and does not matter)
//   pf_select_kernel        a workgroup per non-empty cell (grid-stride): the four ranks min(n - 1, floor(n q)) exactly.  A cell of at
//                           most kPfTile latencies is loaded into LDS, padded to a power of two and sorted there (bitonic, a barrier a
//                           stage); a larger one goes through the most-significant-digit-first radix select of radix_select.h, eight
//                           levels, the four targets' histograms in LDS and a wavefront per target picking (rs_pick, the code
//                           set_full_results.h runs).
//   pf_fill_kernel          a wavefront per class (grid-stride), 64 buckets a step: open_last out of the packed words, and its forward
//                           fill over the plotted buckets (a lane takes the value of the nearest lane at or below it that has an op -- one
//                           lane shuffle --, else what the step before carried on)
//   pf_summary_kernel       one thread: the counts, n_f, nb_all, n_plot, t_max
// Ballots, lane reads, the workgroup barrier and index / thread go through wave_env.h / wave_env_wg.h; the atomics (on LDS words and on
// global memory) and the lane shuffles (rs_pick's, the fill's) are plain HIP, which tests/emu/oneshot_emu.h and tests/emu/emu_perf.cpp state for the host emulator -- these very
// kernels run there lane by lane, with a tile of 32 latencies, against the host statement of jepsen/perf.py (tests/test_perf_emu.py).
#pragma once
#include "wave_env_wg.h"
#include "perf_plan.h"
#include "radix_select.h"
#include "wg_scan.h"

namespace {

using pf::PfArgs;

// signed order as unsigned order, and back
__device__ __forceinline__ unsigned long long pf_key(long long v) { return (unsigned long long)v ^ 0x8000000000000000ull; }
__device__ __forceinline__ long long pf_unkey(unsigned long long k) { return (long long)(k ^ 0x8000000000000000ull); }
__device__ __forceinline__ uint32_t pf_bucket(long long t) { return (uint32_t)((unsigned long long)t / (unsigned long long)pf::kPfSecond); }
__device__ __forceinline__ double pf_quantile(uint32_t j) { return j == 0u ? 0.5 : (j == 1u ? 0.95 : (j == 2u ? 0.99 : 1.0)); }

// every lane that `has` counts 1 for `cell`: one atomic per wavefront and distinct cell.  (Called by whole wavefronts.)
__device__ __forceinline__ void pf_wave_count(uint32_t* counts, bool has, uint32_t cell, uint32_t lane) {
  unsigned long long rem = wv::ballot(has);
  while (rem) {                                                             // (uniform)
    const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
    const uint32_t c = wv::readlane(cell, lead);
    const unsigned long long m = wv::ballot(has && cell == c);
    if (lane == lead) atomicAdd(&counts[c], (uint32_t)__popcll(m));
    rem &= ~m;
  }
}

__global__ __launch_bounds__(256) void pf_classify_kernel(PfArgs A) {
  const uint32_t t = wv::wg_thread(), lane = t & 63u;
  const unsigned long long stride = (unsigned long long)A.grid * 256u;
  uint32_t c_client = 0, c_inv = 0, c_match = 0, c_comp = 0;
  // (every lane of a wavefront makes the same number of trips: the ballots below are wavefront-uniform)
  for (unsigned long long base = (unsigned long long)wv::wg_index() * 256u + (t & ~63u); base < A.n_ops; base += stride) {
    const unsigned long long i = base + lane;
    const bool in = i < A.n_ops;
    bool client = false;
    uint32_t ty = 0, f = 0, part = pf::kPfNone;
    long long tm = 0;
    if (in) {
      client = A.process[i] != TBC_PERF_NO_PROCESS;
      if (client) { ty = A.type[i]; tm = A.time[i]; f = A.f[i]; part = A.partner[i]; }
    }
    const bool inv = client && ty == TBC_PERF_T_INVOKE, comp = client && ty != TBC_PERF_T_INVOKE, matched = inv && part != pf::kPfNone;
    uint32_t outcome = comp ? ty : TBC_PERF_O_NONE;
    long long lat = INT64_MIN;
    if (matched) { outcome = A.type[part]; lat = A.time[part] - tm; }
    if (in) { A.op_latency[i] = lat; A.op_outcome[i] = (uint8_t)outcome; }
    const uint32_t b = pf_bucket(tm);
    pf_wave_count(A.rate_count, comp, comp ? (f * 3u + ty - 1u) * A.nb_all + b : 0u, lane);
    pf_wave_count(A.q_count, matched, matched ? f * A.nb_all + b : 0u, lane);
    c_client += (uint32_t)__popcll(wv::ballot(client)); c_inv += (uint32_t)__popcll(wv::ballot(inv));
    c_match += (uint32_t)__popcll(wv::ballot(matched)); c_comp += (uint32_t)__popcll(wv::ballot(comp));
  }
  if (lane == 0u) {
    if (c_client) atomicAdd(&A.acc->n_client, c_client);
    if (c_inv) atomicAdd(&A.acc->n_invocations, c_inv);
    if (c_match) atomicAdd(&A.acc->n_matched, c_match);
    if (c_comp) atomicAdd(&A.acc->n_completions, c_comp);
  }
}

// op i of the open scan: does it count (a client op with an outcome), for which class, up or down, in which bucket
__device__ __forceinline__ bool pf_open_op(const PfArgs& A, unsigned long long i, bool in, uint32_t& cls, bool& up, uint32_t& b) {
  cls = 0u; up = false; b = 0u;
  if (!in) return false;
  const uint32_t outcome = A.op_outcome[i];
  if (outcome == TBC_PERF_O_NONE) return false;                             // (not a client's, or an invocation nothing completes)
  cls = (uint32_t)A.f[i] * 3u + outcome - 1u;
  up = A.type[i] == TBC_PERF_T_INVOKE;
  b = pf_bucket(A.time[i]);
  return true;
}

__global__ __launch_bounds__(64) void pf_open_totals_kernel(PfArgs A) {
  const uint32_t lane = wv::wg_thread();
  for (uint32_t g = wv::wg_index(); g < A.n_chunks; g += A.grid) {
    const unsigned long long lo = (unsigned long long)g * A.chunk_ops, hi = lo + A.chunk_ops < A.n_ops ? lo + A.chunk_ops : A.n_ops;
    uint32_t* const row = A.carry + (unsigned long long)g * A.n_class;
    for (unsigned long long base = lo; base < hi; base += 64u) {
      uint32_t cls, b;
      bool up;
      const bool has = pf_open_op(A, base + lane, base + lane < hi, cls, up, b);
      unsigned long long rem = wv::ballot(has);
      while (rem) {                                                         // (uniform) a trip per distinct class of the 64 ops
        const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
        const uint32_t c = wv::readlane(cls, lead);
        const unsigned long long m_up = wv::ballot(has && cls == c && up), m_dn = wv::ballot(has && cls == c && !up);
        const uint32_t d = (uint32_t)__popcll(m_up) - (uint32_t)__popcll(m_dn);
        if (lane == lead && d) atomicAdd(&row[c], d);
        rem &= ~(m_up | m_dn);
      }
    }
  }
}

// exclusive prefix sums over the workgroup's 256 threads (s: 256 words of LDS); `total`: the sum of all
__device__ __forceinline__ uint32_t pf_wg_scan(uint32_t v, uint32_t* s, uint32_t t, uint32_t& total) {
  return wg_scan_excl(v, s, t, 0u, total, [](uint32_t a, uint32_t b) { return a + b; });
}

__global__ __launch_bounds__(256) void pf_open_carry_kernel(PfArgs A) {
  __shared__ uint32_t s_scan[256];
  const uint32_t t = wv::wg_thread();
  for (uint32_t c = wv::wg_index(); c < A.n_class; c += A.grid) {
    uint32_t run = 0;
    for (uint32_t g0 = 0; g0 < A.n_chunks; g0 += 256u) {
      const bool in = g0 + t < A.n_chunks;
      uint32_t* const p = A.carry + (unsigned long long)(g0 + t) * A.n_class + c;
      uint32_t total;
      const uint32_t ex = pf_wg_scan(in ? *p : 0u, s_scan, t, total);
      if (in) *p = run + ex;
      run += total;
    }
  }
}

__global__ __launch_bounds__(64) void pf_open_scan_kernel(PfArgs A) {
  const uint32_t lane = wv::wg_thread();
  const unsigned long long below = (2ull << lane) - 1ull;                   // the lanes at or below this one
  for (uint32_t g = wv::wg_index(); g < A.n_chunks; g += A.grid) {
    const unsigned long long lo = (unsigned long long)g * A.chunk_ops, hi = lo + A.chunk_ops < A.n_ops ? lo + A.chunk_ops : A.n_ops;
    uint32_t* const row = A.carry + (unsigned long long)g * A.n_class;
    for (unsigned long long base = lo; base < hi; base += 64u) {
      const unsigned long long i = base + lane;
      uint32_t cls, b;
      bool up;
      const bool has = pf_open_op(A, i, i < hi, cls, up, b);
      uint32_t after = 0u;
      unsigned long long rem = wv::ballot(has);
      while (rem) {                                                         // (uniform)
        const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
        const uint32_t c = wv::readlane(cls, lead);
        const unsigned long long m_up = wv::ballot(has && cls == c && up), m_dn = wv::ballot(has && cls == c && !up);
        uint32_t before = 0u;
        if (lane == lead) before = atomicAdd(&row[c], (uint32_t)__popcll(m_up) - (uint32_t)__popcll(m_dn));
        before = wv::readlane(before, lead);
        if (has && cls == c) after = before + (uint32_t)__popcll(m_up & below) - (uint32_t)__popcll(m_dn & below);
        rem &= ~(m_up | m_dn);
      }
      if (i < hi) A.op_open_after[i] = (int32_t)after;
      if (has) atomicMax(&A.open_word[(unsigned long long)cls * A.nb_all + b], ((i + 1ull) << 32) | (unsigned long long)after);
    }
  }
}

__global__ __launch_bounds__(256) void pf_cell_sum_kernel(PfArgs A) {
  __shared__ uint32_t s_sum, s_max;
  const uint32_t t = wv::wg_thread();
  for (uint32_t tile = wv::wg_index(); tile < A.n_scan_tiles; tile += A.grid) {
    if (t == 0u) { s_sum = 0u; s_max = 0u; }
    wv::wg_barrier();
    const unsigned long long cell = (unsigned long long)tile * pf::kPfScanTile + t;
    const uint32_t v = cell < A.n_cells ? A.q_count[cell] : 0u;
    if (v) { atomicAdd(&s_sum, v); atomicMax(&s_max, v); }
    wv::wg_barrier();
    if (t == 0u) {
      A.tile_sum[tile] = s_sum;
      if (s_max) atomicMax(&A.acc->max_cell, s_max);
    }
    wv::wg_barrier();
  }
}

__global__ __launch_bounds__(256) void pf_tile_scan_kernel(PfArgs A) {       // (one workgroup)
  __shared__ uint32_t s_scan[256];
  const uint32_t t = wv::wg_thread();
  uint32_t base = 0;
  for (uint32_t t0 = 0; t0 < A.n_scan_tiles; t0 += 256u) {
    const bool in = t0 + t < A.n_scan_tiles;
    uint32_t total;
    const uint32_t ex = pf_wg_scan(in ? A.tile_sum[t0 + t] : 0u, s_scan, t, total);
    if (in) A.tile_sum[t0 + t] = base + ex;
    base += total;
  }
}

__global__ __launch_bounds__(256) void pf_cell_offsets_kernel(PfArgs A) {
  __shared__ uint32_t s_scan[256];
  const uint32_t t = wv::wg_thread();
  for (uint32_t tile = wv::wg_index(); tile < A.n_scan_tiles; tile += A.grid) {
    const unsigned long long cell = (unsigned long long)tile * pf::kPfScanTile + t;
    const bool in = cell < A.n_cells;
    uint32_t total;
    const uint32_t off = A.tile_sum[tile] + pf_wg_scan(in ? A.q_count[cell] : 0u, s_scan, t, total);
    if (in) { A.q_off[cell] = off; A.q_cur[cell] = off; }
  }
}

__global__ __launch_bounds__(256) void pf_gather_kernel(PfArgs A) {
  const unsigned long long stride = (unsigned long long)A.grid * 256u;
  for (unsigned long long i = (unsigned long long)wv::wg_index() * 256u + wv::wg_thread(); i < A.n_ops; i += stride) {
    const long long lat = A.op_latency[i];
    if (lat == INT64_MIN) continue;
    const uint32_t at = atomicAdd(&A.q_cur[(uint32_t)A.f[i] * A.nb_all + pf_bucket(A.time[i])], 1u);
    A.lat_cell[at] = pf_key(lat);
  }
}

__global__ __launch_bounds__(256) void pf_select_kernel(PfArgs A) {
  __shared__ unsigned long long s_v[pf::kPfTile];
  __shared__ uint32_t s_hist[TBC_PERF_QUANTILES * kSelBins];
  __shared__ unsigned long long s_prefix[TBC_PERF_QUANTILES];
  __shared__ uint32_t s_k[TBC_PERF_QUANTILES];
  const uint32_t t = wv::wg_thread();
  for (uint32_t cell = wv::wg_index(); cell < A.n_cells; cell += A.grid) {
    const uint32_t n = A.q_count[cell];                                     // (uniform: the branches below are the whole workgroup's)
    long long* const out = A.q_value + (unsigned long long)cell * TBC_PERF_QUANTILES;
    if (n == 0u) {
      if (t < TBC_PERF_QUANTILES) out[t] = 0;
      continue;
    }
    const unsigned long long* __restrict__ src = A.lat_cell + A.q_off[cell];
    if (n <= pf::kPfTile) {
      uint32_t P = 1;
      while (P < n) P <<= 1;
      for (uint32_t i = t; i < P; i += 256u) s_v[i] = i < n ? src[i] : ~0ull;           // (no latency's key is all ones: times are below 2^52)
      wv::wg_barrier();
      for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
          for (uint32_t i = t; i < P; i += 256u) {
            const uint32_t p = i ^ j;
            if (p > i) {
              const unsigned long long a = s_v[i], b = s_v[p];
              if ((a > b) == ((i & k) == 0u)) { s_v[i] = b; s_v[p] = a; }
            }
          }
          wv::wg_barrier();
        }
      if (t < TBC_PERF_QUANTILES) out[t] = pf_unkey(s_v[sf_rank(n, pf_quantile(t))]);
      wv::wg_barrier();                                                     // (the tile is loaded again only when the ranks are read)
      continue;
    }
    // ---- a cell of more than a tile: a wavefront per target, eight bits a level from the top
    const uint32_t wave = t >> 6, lane = t & 63u;
    if (lane == 0u) { s_prefix[wave] = 0ull; s_k[wave] = sf_rank(n, pf_quantile(wave)); }
    for (uint32_t level = 8; level-- > 0u;) {
      for (uint32_t i = t; i < TBC_PERF_QUANTILES * kSelBins; i += 256u) s_hist[i] = 0u;
      wv::wg_barrier();
      unsigned long long hi[TBC_PERF_QUANTILES];                            // the bits above this level's digit that a value must share with the target
      for (uint32_t q = 0; q < TBC_PERF_QUANTILES; q++) hi[q] = level < 7u ? s_prefix[q] >> (8u * (level + 1u)) : 0ull;
      for (uint32_t i = t; i < n; i += 256u) {
        const unsigned long long v = src[i];
        const unsigned long long above = level < 7u ? v >> (8u * (level + 1u)) : 0ull;
        const uint32_t digit = (uint32_t)(v >> (8u * level)) & 255u;
        for (uint32_t q = 0; q < TBC_PERF_QUANTILES; q++)
          if (above == hi[q]) atomicAdd(&s_hist[q * kSelBins + digit], 1u);
      }
      wv::wg_barrier();
      const uint32_t* const h4 = &s_hist[wave * kSelBins + 4u * lane];
      const uint4 h = make_uint4(h4[0], h4[1], h4[2], h4[3]);
      const uint32_t k = s_k[wave];
      uint32_t bin = 0u, left = 0u;
      if (rs_pick(h, lane, k, bin, left)) { s_prefix[wave] |= (unsigned long long)bin << (8u * level); s_k[wave] = left; }
      wv::wg_barrier();
    }
    if (t < TBC_PERF_QUANTILES) out[t] = pf_unkey(s_prefix[t]);
    wv::wg_barrier();
  }
}

__global__ __launch_bounds__(64) void pf_fill_kernel(PfArgs A) {
  const uint32_t lane = wv::wg_thread();
  const unsigned long long below = (2ull << lane) - 1ull;                   // the lanes at or below this one
  for (uint32_t c = wv::wg_index(); c < A.n_class; c += A.grid) {
    const unsigned long long* __restrict__ w = A.open_word + (unsigned long long)c * A.nb_all;
    int32_t* const last = A.open_last + (unsigned long long)c * A.nb_all;
    int32_t* const fill = A.open_fill + (unsigned long long)c * A.n_plot;
    uint32_t cur = 0u;                                                      // the value carried into this step (uniform)
    for (uint32_t b0 = 0; b0 < A.nb_all; b0 += 64u) {
      const uint32_t b = b0 + lane;
      const unsigned long long x = b < A.nb_all ? w[b] : 0ull;
      const uint32_t v = (uint32_t)x;
      if (b < A.nb_all) last[b] = x ? (int32_t)v : INT32_MIN;
      // forward fill: the value of the nearest bucket at or below this one that has an op, else what was carried in
      const unsigned long long m = wv::ballot(x != 0ull && b < A.n_plot), mine = m & below;
      const uint32_t from = (uint32_t)__shfl((int)v, mine ? 63 - (int)__builtin_clzll(mine) : (int)lane);
      const uint32_t filled = mine ? from : cur;
      if (m) cur = wv::readlane(v, 63u - (uint32_t)__builtin_clzll(m));     // (uniform) the last bucket of the 64 that has an op is carried on
      if (b < A.n_plot) fill[b] = (int32_t)filled;
    }
  }
}

__global__ __launch_bounds__(64) void pf_summary_kernel(PfArgs A) {
  if (wv::wg_thread() != 0u) return;
  const pf::PfAcc& a = *A.acc;
  tbc_perf_summary s{};
  s.n_ops = A.n_ops; s.n_client = a.n_client; s.n_invocations = a.n_invocations; s.n_matched = a.n_matched; s.n_completions = a.n_completions;
  s.n_f = A.n_f; s.nb_all = A.nb_all; s.n_plot = A.n_plot; s.max_cell = a.max_cell; s.t_max = A.t_max;
  *A.summary = s;
}

}  // namespace

namespace pf {

// Every kernel of the call in order, over a launcher (oneshot_plan.h): THE statement of the launches -- the library runs it over a
// stream (perf.hip), the tests over the emulator and over a recorder.  A kernel with nothing to do is not launched: no ops, no f's
// (no client op: no cells and no classes).  (The two single-workgroup kernels ask for one block under a cap of one: exact from any launcher.)
template <class Launcher>
void sequence(Launcher& go, PfArgs A) {
  const auto run = [&](void (*kernel)(PfArgs), uint64_t blocks, uint32_t cap, uint32_t threads) {
    if (!blocks) return;
    A.grid = go.grid(blocks, cap);
    go.launch(kernel, A.grid, threads, A);
  };
  const uint64_t op_blocks = ((uint64_t)A.n_ops + 255u) / 256u;
  run(pf_classify_kernel, op_blocks, 8192u, 256u);
  if (A.n_class) run(pf_open_totals_kernel, A.n_chunks, 4096u, 64u);
  run(pf_open_carry_kernel, A.n_chunks ? A.n_class : 0u, 16384u, 256u);
  run(pf_open_scan_kernel, A.n_chunks, 4096u, 64u);                         // (without a client op it writes the zeros of op_open_after)
  run(pf_cell_sum_kernel, A.n_scan_tiles, 8192u, 256u);
  run(pf_tile_scan_kernel, A.n_scan_tiles ? 1u : 0u, 1u, 256u);
  run(pf_cell_offsets_kernel, A.n_scan_tiles, 8192u, 256u);
  run(pf_gather_kernel, A.n_cells ? op_blocks : 0u, 8192u, 256u);
  run(pf_select_kernel, A.n_cells, 16384u, 256u);
  run(pf_fill_kernel, A.n_class, 16384u, 64u);
  run(pf_summary_kernel, 1u, 1u, 64u);
}

}  // namespace pf
