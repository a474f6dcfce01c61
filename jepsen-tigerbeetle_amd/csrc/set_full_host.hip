// set_full_host.hip -- the host side of jepsen.checker/set-full: the object behind tbc_setfull_* and tbc_setfull_keys_*, its create, run
// and results, and the C entry points.  The scan's kernels are set_full.hip (launched through set_full_scan.h); the kernels of the results
// (set_full_results.h) and of the op columns' encoding (set_full_encode.h) are compiled into this unit; where everything lies in the
// object's arena, and which tile of which grid is which key's, is sf_make_layout's to say (set_full_plan.h).
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include "tbc_internal.h"
#include "set_full_plan.h"
#include "set_full_scan.h"
#include "set_full_encode_plan.h"

using namespace tbc;

#define SF_TRY(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
      return e_ == hipErrorOutOfMemory ? TBC_ERR_OOM : TBC_ERR_HIP;                          \
    }                                                                                        \
  } while (0)

#include "set_full_results.h"
#include "set_full_encode.h"

// One object behind all three entry points: a single key (tbc_setfull) is a keyed object with n_keys = 1.
struct SfObject {
  int device = 0;
  uint32_t n_keys = 0, sumE = 0, sumR = 0, tiles_any = 0, tiles_resolve = 0, tiles_select = 0;
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
  void* res_arena = nullptr;
  uint64_t res_times = 0;
  hipEvent_t ev2 = nullptr, ev3 = nullptr;
  // tbc_setfull_keys_create_ops: the plan the host made of the ops (what tbc_setfull_keys_encoding hands back) and what the encoding
  // kernels found
  bool from_ops = false;
  sfenc::Plan enc;
  std::vector<uint32_t> dup_max, dup_count;
  std::vector<uint64_t> unknown;
  uint64_t ns_encode = 0;
  // (the stream first: a call that failed half way may have left a copy into one of the vectors above, or a kernel, in flight)
  ~SfObject() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : {arena, res_arena}) if (p) (void)hipFree(p);
    for (hipEvent_t e : {ev0, ev1, ev2, ev3}) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
// (the C handles tbc_setfull and tbc_setfull_keys stay incomplete types: two names of a pointer to this object)
SfObject* sf_obj(tbc_setfull* h) { return reinterpret_cast<SfObject*>(h); }
SfObject* sf_obj(tbc_setfull_keys* h) { return reinterpret_cast<SfObject*>(h); }

namespace {

// what one call makes on the device and must not outlive it
struct SfDevBuf { void* p = nullptr; ~SfDevBuf() { if (p) (void)hipFree(p); } };
struct SfEvent { hipEvent_t e = nullptr; ~SfEvent() { if (e) (void)hipEventDestroy(e); } };

// the scan's three results on the device, each n_elements per key, key after key
struct SfOut { uint32_t *known, *lp, *la; };
SfOut sf_out(const SfObject* S) { return {S->d_out, S->d_out + S->sumE, S->d_out + 2ull * S->sumE}; }

template <class T> T* sf_at(const SfObject* S, const SfRegion& r) { return reinterpret_cast<T*>(static_cast<char*>(S->arena) + r.at); }
// one of the host's arrays straight to its region of the arena, on the object's stream
hipError_t sf_put(const SfObject* S, const SfRegion& r, const void* src) {
  return r.bytes ? hipMemcpyAsync(sf_at<char>(S, r), src, r.bytes, hipMemcpyHostToDevice, S->stream) : hipSuccess;
}

tbc_status sf_check_device(uint32_t device) {
  int ndev = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || (int)device >= ndev) { set_error("no usable HIP device; libtbcheck has no CPU fallback"); return TBC_ERR_NO_DEVICE; }
  if (hipGetDeviceProperties(&prop, (int)device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_error("device %u is not a gfx950 (MI355X) device", device); return TBC_ERR_NO_DEVICE; }
  return TBC_OK;
}

// Every rule of one key's inputs, on the host (the kernels trust them): the prefix search per row and "the latest row" rest on the
// documented orders; every offset and element number of the compact reads is checked (top == nullptr: no compact reads).
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

// what the matrix is made from: Dense -- the caller's rows; Rows -- top / exc_off / exc of `in`; Ops -- the reads' raw values (S->enc: their plan)
struct SfFrom { SfSource source; const tbc_setfull_in* dense = nullptr; const int64_t* vals = nullptr; };

// ---- the matrix, three ways, on the object's stream.  Dense: the caller's, copied into the key's pitch (its padding zeroed: no word the
// scan loads is left unset; words of the caller's rows past the key's are ignored)
tbc_status sf_matrix_dense(SfObject* S, const SfKeyPlan& p, const tbc_setfull_in* dense) {
  if (!(p.R && p.WPR)) return TBC_OK;
  if (p.PITCH > p.WPR) SF_TRY(hipMemset2DAsync(S->d_M + p.WPR, (size_t)p.PITCH * 4, 0, (size_t)(p.PITCH - p.WPR) * 4, p.R, S->stream));
  SF_TRY(hipMemcpy2DAsync(S->d_M, (size_t)p.PITCH * 4, dense->present, (size_t)dense->words_per_row * 4, (size_t)p.WPR * 4, p.R, hipMemcpyHostToDevice, S->stream));
  return TBC_OK;
}
// Rows: built from the compact reads (setfull_rows_kernel)
tbc_status sf_matrix_rows(SfObject* S, const SfLayout& L) {
  if (L.sumR)
    sf_launch_rows(S->stream, std::min<uint32_t>(L.sumR, 16384u), S->d_plan, S->d_first, L.n_keys, L.sumR, sf_at<const uint32_t>(S, L.arena.top),
                   sf_at<const unsigned long long>(S, L.arena.exc_off), sf_at<const uint32_t>(S, L.arena.exc), S->d_M);
  return TBC_OK;
}
// Ops: built from the reads' raw values by the kernels of set_full_encode.h: the keys' tables, the values kernel, the repeat counter back -- only
// a history with a duplicated element pays for the exact pass -- then the counters back and ns_encode.  The raw values are an allocation
// of this call's own, gone when it returns (8 B a value where the matrix has a bit); the call ends synchronised.
tbc_status sf_matrix_values(SfObject* S, const SfLayout& L, const int64_t* vals) {
  const SfArena& A = L.arena;
  const uint32_t n = L.n_keys, sumE = L.sumE, sumR = L.sumR;
  SfDevBuf d_vals;
  SfEvent e0, e1, d0, d1;
  uint32_t h_repeats = 0;
  SfEncArgs E;
  E.plan = S->d_plan; E.first = S->d_first; E.enc = sf_at<const SfEncKey>(S, A.enc); E.n_keys = n; E.R_all = sumR; E.E_all = sumE;
  E.grid = std::min<uint32_t>(sumR, 16384u);
  E.element = sf_at<const long long>(S, A.element); E.slots = sf_at<SfEncSlot>(S, A.slots);
  E.val_lo = sf_at<const unsigned long long>(S, A.val_lo); E.val_hi = sf_at<const unsigned long long>(S, A.val_hi);
  E.M = S->d_M; E.row_flag = sf_at<uint8_t>(S, A.row_flag); E.key_flag = sf_at<uint32_t>(S, A.key_flag); E.unknown = sf_at<unsigned long long>(S, A.unknown);
  E.repeats = sf_at<uint32_t>(S, A.repeats); E.cnt = sf_at<uint32_t>(S, A.cnt); E.dup_max = sf_at<uint32_t>(S, A.dup_max); E.dup_count = sf_at<uint32_t>(S, A.dup_count);
  const uint64_t nv = S->enc.n_values;
  if (nv) SF_TRY(hipMalloc(&d_vals.p, nv * 8));
  E.vals = (const long long*)d_vals.p;
  SF_TRY(hipEventCreate(&e0.e)); SF_TRY(hipEventCreate(&e1.e));
  SF_TRY(sf_put(S, A.element, S->enc.element.data()));
  SF_TRY(sf_put(S, A.val_lo, S->enc.val_lo.data())); SF_TRY(sf_put(S, A.val_hi, S->enc.val_hi.data()));
  if (nv) SF_TRY(hipMemcpyAsync(d_vals.p, vals, nv * 8, hipMemcpyHostToDevice, S->stream));
  SF_TRY(hipMemsetAsync(sf_at<char>(S, A.slots), 0, A.enc_zero_bytes(), S->stream));
  SF_TRY(hipEventRecord(e0.e, S->stream));
  if (sumE) hipLaunchKernelGGL(sf_table_build_kernel, dim3((sumE + 255u) / 256u), dim3(256), 0, S->stream, E);
  if (sumR) hipLaunchKernelGGL(sf_values_kernel<TBC_SETFULL_ENCODE_WINDOW_WORDS>, dim3(E.grid), dim3(256), 0, S->stream, E);
  SF_TRY(hipGetLastError());
  SF_TRY(hipEventRecord(e1.e, S->stream));
  SF_TRY(hipMemcpyAsync(&h_repeats, E.repeats, 4, hipMemcpyDeviceToHost, S->stream));
  SF_TRY(hipStreamSynchronize(S->stream));
  float ms = 0, ms_d = 0;
  SF_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
  if (h_repeats) {
    SF_TRY(hipEventCreate(&d0.e)); SF_TRY(hipEventCreate(&d1.e));
    SF_TRY(hipEventRecord(d0.e, S->stream));
    hipLaunchKernelGGL(sf_dups_kernel, dim3(n), dim3(256), 0, S->stream, E);
    SF_TRY(hipGetLastError());
    SF_TRY(hipEventRecord(d1.e, S->stream));
  }
  S->dup_max.assign(sumE, 0u); S->dup_count.assign(n, 0u); S->unknown.assign(n, 0ull);
  if (h_repeats) {
    if (sumE) SF_TRY(hipMemcpyAsync(S->dup_max.data(), E.dup_max, (size_t)sumE * 4, hipMemcpyDeviceToHost, S->stream));
    SF_TRY(hipMemcpyAsync(S->dup_count.data(), E.dup_count, (size_t)n * 4, hipMemcpyDeviceToHost, S->stream));
  }
  SF_TRY(hipMemcpyAsync(S->unknown.data(), E.unknown, (size_t)n * 8, hipMemcpyDeviceToHost, S->stream));
  SF_TRY(hipStreamSynchronize(S->stream));
  if (h_repeats) SF_TRY(hipEventElapsedTime(&ms_d, d0.e, d1.e));
  S->ns_encode = (uint64_t)((ms + ms_d) * 1e6);
  return TBC_OK;
}

// The create behind every entry point.  `in`: the keys' arrays end to end (tbc_setfull_keys_in; the single-key entries point it at their
// own one key); `keyed`: name the key in a message.  Every rule is checked before any device call; a std::bad_alloc is sf_new's to report.
tbc_status sf_create(const char* fn, bool keyed, const tbc_setfull_keys_in* in, const SfFrom& from, SfObject* S) {
  const uint32_t n = in->n_keys;
  const bool rows = from.source == SfSource::Rows;
  if (rows && in->exc_off[0] != 0) { set_error("%s: exc_off[0] must be 0", fn); return TBC_ERR_INVALID_ARG; }
  uint64_t n_exc = 0;
  {
    std::vector<uint32_t> tmp;
    char where[64];
    size_t e0 = 0, r0 = 0;
    for (uint32_t k = 0; k < n; e0 += in->n_elements[k], r0 += in->n_reads[k], k++) {
      if (keyed) std::snprintf(where, sizeof where, "%s: key %u", fn, k); else std::snprintf(where, sizeof where, "%s", fn);
      if (!sf_key_is_valid(where, in->n_elements[k], in->n_reads[k], in->add_invoke + e0, in->read_invoke + r0, rows ? in->top + r0 : nullptr,
                           rows ? in->exc_off + r0 : nullptr, in->exc, tmp))
        return TBC_ERR_INVALID_ARG;
    }
    if (rows) n_exc = in->exc_off[r0];
  }
  const tbc_status dev = sf_check_device(in->device);
  if (dev != TBC_OK) return dev;
  // ---- the layout, and the head of the arena as the host makes it: the plan, the first tiles, the prefix extremes' start values
  const SfLayout L = sf_make_layout(n, in->n_elements, in->n_reads, from.source, from.dense ? from.dense->words_per_row : 0u, n_exc);
  const SfArena& A = L.arena;
  S->key_max = sf_key_max(L, in->add_invoke, in->add_ok, in->read_invoke, in->read_ok);
  if (!L.fits()) { set_error("%s: too many elements for one object", fn); return TBC_ERR_INVALID_ARG; }
  S->device = (int)in->device; S->n_keys = n; S->sumE = L.sumE; S->sumR = L.sumR; S->bytes_matrix = L.bytes_matrix;
  S->from_ops = from.source == SfSource::Ops;
  S->tiles_any = (uint32_t)L.tiles[kFirstAny]; S->tiles_resolve = (uint32_t)L.tiles[kFirstResolve]; S->tiles_select = (uint32_t)L.tiles[kFirstSelect];
  std::vector<unsigned char> img(A.head_bytes(), 0);
  std::memcpy(img.data() + A.plan.at, L.plan.data(), A.plan.bytes);
  std::memcpy(img.data() + A.first.at, L.first.data(), A.first.bytes);
  if (A.enc.bytes) std::memcpy(img.data() + A.enc.at, L.enc_keys.data(), A.enc.bytes);
  for (const SfKeyPlan& p : L.plan)       // the chunks' greatest prefixes start at 0, their least at ~0 (the minima lie behind the maxima)
    std::memset(img.data() + A.pmax.at + ((size_t)p.pmax_off + p.chunks) * 4, 0xFF, (size_t)p.chunks * 4);
  // ---- one allocation, the stream, the scan's events
  SF_TRY(hipSetDevice(S->device));
  SF_TRY(hipMalloc(&S->arena, std::max<size_t>(A.bytes, 256)));
  S->d_plan = sf_at<SfKeyPlan>(S, A.plan); S->d_first = sf_at<uint32_t>(S, A.first); S->d_pmax = sf_at<uint32_t>(S, A.pmax);
  S->d_add_ok = sf_at<uint32_t>(S, A.add_ok); S->d_read_invoke = sf_at<uint32_t>(S, A.read_invoke); S->d_read_ok = sf_at<uint32_t>(S, A.read_ok);
  S->d_M = sf_at<uint32_t>(S, A.M); S->d_P = sf_at<uint32_t>(S, A.P); S->d_anyp = sf_at<uint32_t>(S, A.any); S->d_anya = S->d_anyp + L.sum_words;
  S->d_out = sf_at<uint32_t>(S, A.out); S->d_words = sf_at<unsigned long long>(S, A.words);
  SF_TRY(hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking));
  SF_TRY(hipEventCreate(&S->ev0)); SF_TRY(hipEventCreate(&S->ev1));
  // ---- each of the caller's arrays straight to its place in the arena: a handful of copies whatever n_keys is.  (Packing them into the
  // host image first -- one H2D -- gains 0.04-0.09 ms on objects below ~1 MB and loses from ~1.5 MB on, 0.8 ms at the bench key's 13 MB
  // and 3 ms at 256 keys x 2k ops; the direct copies alone hold the parent's end-to-end time at every shape measured: DESIGN.md K7.)
  // The copies read pageable memory of the caller's: the synchronise below ends them before create returns.
  SF_TRY(sf_put(S, A.add_invoke, in->add_invoke)); SF_TRY(sf_put(S, A.add_ok, in->add_ok));
  SF_TRY(sf_put(S, A.read_invoke, in->read_invoke)); SF_TRY(sf_put(S, A.read_ok, in->read_ok));
  SF_TRY(sf_put(S, A.top, in->top)); SF_TRY(sf_put(S, A.exc_off, in->exc_off)); SF_TRY(sf_put(S, A.exc, in->exc));
  SF_TRY(hipMemcpyAsync(S->arena, img.data(), img.size(), hipMemcpyHostToDevice, S->stream));
  if (L.sum_words) SF_TRY(hipMemsetAsync(S->d_anyp, 0, L.sum_words * 8, S->stream));     // (the tiles below the diagonal never write theirs)
  // ---- the matrix
  tbc_status st = TBC_OK;
  switch (from.source) {
    case SfSource::Dense: st = sf_matrix_dense(S, L.plan[0], from.dense); break;
    case SfSource::Rows: st = sf_matrix_rows(S, L); break;
    case SfSource::Ops: st = sf_matrix_values(S, L, from.vals); break;
  }
  if (st != TBC_OK) return st;
  // ---- p[r] (how many elements had been invoked when read r completed) and the chunks' extremes depend on the inputs only
  if (L.tiles[kFirstPrefix])
    sf_launch_prefix(S->stream, (uint32_t)L.tiles[kFirstPrefix], S->d_plan, S->d_first, n, sf_at<const uint32_t>(S, A.add_invoke), S->d_read_ok,
                     S->d_P, S->d_pmax);
  SF_TRY(hipGetLastError());
  SF_TRY(hipStreamSynchronize(S->stream));
  return TBC_OK;
}

// a new object, filled by `create`, into *handle -- or nothing left behind
template <class Handle, class Create>
tbc_status sf_new(const char* fn, Handle** handle, Create create) {
  SfObject* S = new (std::nothrow) SfObject();
  if (!S) return TBC_ERR_OOM;
  tbc_status st;
  try { st = create(S); } catch (const std::bad_alloc&) { set_error("%s: host memory", fn); st = TBC_ERR_OOM; }
  if (st != TBC_OK) { delete S; return st; }
  *handle = reinterpret_cast<Handle*>(S);
  return TBC_OK;
}

// the scan's two launches between its events (ev0, ev1), on the object's stream: what run and results share
tbc_status sf_scan(SfObject* S) {
  hipStream_t s = S->stream;
  const SfOut o = sf_out(S);
  SF_TRY(hipMemsetAsync(S->d_words, 0, kCounterBytes, s));
  SF_TRY(hipEventRecord(S->ev0, s));
  if (S->tiles_any) sf_launch_any(s, S->tiles_any, S->d_plan, S->d_first, S->n_keys, S->d_M, S->d_P, S->d_pmax, S->d_anyp, S->d_anya, S->d_words);
  if (S->tiles_resolve)
    sf_launch_resolve(s, S->tiles_resolve, S->d_plan, S->d_first, S->n_keys, S->d_M, S->d_P, S->d_read_invoke, S->d_read_ok, S->d_anyp, S->d_anya,
                      S->d_add_ok, o.lp, o.la, o.known, S->d_words);
  SF_TRY(hipGetLastError());
  SF_TRY(hipEventRecord(S->ev1, s));
  return TBC_OK;
}

// ... and how such a call ends: the word counters back, the stream synchronised (whatever else the call queued arrives too), time and sum
tbc_status sf_scan_stats(SfObject* S, uint64_t* ns_scan, uint64_t* bytes_scanned, uint64_t* bytes_matrix) {
  SF_TRY(hipMemcpyAsync(S->h_words, S->d_words, kCounterBytes, hipMemcpyDeviceToHost, S->stream));
  SF_TRY(hipStreamSynchronize(S->stream));
  float ms = 0;
  SF_TRY(hipEventElapsedTime(&ms, S->ev0, S->ev1));
  unsigned long long words = 0;
  for (uint32_t k = 0; k < kWordCounters; k++) words += S->h_words[16u * k];
  *ns_scan = (uint64_t)(ms * 1e6);
  *bytes_scanned = (uint64_t)words * 4;
  *bytes_matrix = S->bytes_matrix;
  return TBC_OK;
}

// The run behind both handles (Out: tbc_setfull_out or tbc_setfull_keys_out): the scan, then the results (n_elements each, key after key),
// each array straight into the caller's
template <class Out>
tbc_status sf_run_out(const char* fn, SfObject* S, Out* out) {
  if (!S || !out || (S->sumE && (!out->known || !out->last_present || !out->last_absent))) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  SF_TRY(hipSetDevice(S->device));
  const size_t e4 = (size_t)S->sumE * 4;
  const SfOut o = sf_out(S);
  { const tbc_status st = sf_scan(S); if (st != TBC_OK) return st; }
  if (e4) {
    SF_TRY(hipMemcpyAsync(out->known, o.known, e4, hipMemcpyDeviceToHost, S->stream));
    SF_TRY(hipMemcpyAsync(out->last_present, o.lp, e4, hipMemcpyDeviceToHost, S->stream));
    SF_TRY(hipMemcpyAsync(out->last_absent, o.la, e4, hipMemcpyDeviceToHost, S->stream));
  }
  return sf_scan_stats(S, &out->ns_scan, &out->bytes_scanned, &out->bytes_matrix);
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
  SfCursor c;
  const size_t o_acc = c.take(sizeof(SfKeyAcc) * n).at, o_sel = c.take(sizeof(SfSel) * kSelTargets * n).at,
               o_hist = c.take((size_t)4 * kSelTargets * kSelBins * n).at, o_sum = c.take(sizeof(tbc_setfull_key_summary) * n).at,
               o_toff = c.take((size_t)8 * (n + 1)).at, o_oc = c.take(sumE).at, o_sl = c.take(sumE * 8).at, o_ll = c.take(sumE * 8).at,
               o_time = c.take((size_t)std::max<uint64_t>(T, S->res_times) * 8).at;
  if (!S->res_arena || T > S->res_times) {
    if (S->res_arena) { SF_TRY(hipStreamSynchronize(s)); SF_TRY(hipFree(S->res_arena)); S->res_arena = nullptr; }
    SF_TRY(hipMalloc(&S->res_arena, std::max<size_t>(c.at, 256)));
    S->res_times = std::max<uint64_t>(T, S->res_times);
    SF_TRY(hipMemsetAsync(S->res_arena, 0, o_toff, s));         // (select state and histograms start at zero; every pick leaves its histogram zeroed)
    if (!S->ev2) { SF_TRY(hipEventCreate(&S->ev2)); SF_TRY(hipEventCreate(&S->ev3)); }
  }
  char* const R0 = static_cast<char*>(S->res_arena);
  const SfOut o = sf_out(S);
  SfResArgs A;
  A.plan = S->d_plan; A.first = S->d_first; A.n_keys = n; A.flags = times->flags;
  A.known = o.known; A.lp = o.lp; A.la = o.la;
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
  { const tbc_status st = sf_scan_stats(S, &out->ns_scan, &out->bytes_scanned, &out->bytes_matrix); if (st != TBC_OK) return st; }
  float ms_res = 0;
  SF_TRY(hipEventElapsedTime(&ms_res, S->ev2, S->ev3));
  out->ns_results = (uint64_t)(ms_res * 1e6);
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
  return sf_new(fn, handle, [&](SfObject* S) { return sf_create(fn, false, &one, SfFrom{SfSource::Dense, in}, S); });
}

tbc_status tbc_setfull_create_rows(const tbc_setfull_rows* in, tbc_setfull** handle) {
  const char* fn = "tbc_setfull_create_rows";
  if (!in || !handle || (in->n_elements && (!in->add_invoke || !in->add_ok)) ||
      (in->n_reads && (!in->read_invoke || !in->read_ok || !in->top)) || !in->exc_off || (in->exc_off[in->n_reads] && !in->exc) || in->reserved0 != 0) {
    set_error("%s: null argument", fn);
    return TBC_ERR_INVALID_ARG;
  }
  const tbc_setfull_keys_in one = {1u, in->device, &in->n_elements, &in->n_reads, in->add_invoke, in->add_ok, in->read_invoke, in->read_ok, in->top, in->exc_off, in->exc};
  return sf_new(fn, handle, [&](SfObject* S) { return sf_create(fn, false, &one, SfFrom{SfSource::Rows}, S); });
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
  return sf_new(fn, handle, [&](SfObject* S) { return sf_create(fn, true, in, SfFrom{SfSource::Rows}, S); });
}

tbc_status tbc_setfull_keys_create_ops(const tbc_setfull_ops_in* in, tbc_setfull_keys** handle) {
  const char* fn = "tbc_setfull_keys_create_ops";
  if (!in || !handle) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  if (in->n_keys == 0) { set_error("%s: n_keys is 0", fn); return TBC_ERR_INVALID_ARG; }
  if (!in->op_off || !in->index || !in->type || !in->f || !in->process || !in->value || !in->val_off || !in->vals) {
    set_error("%s: null argument (every pointer of tbc_setfull_ops_in must be set)", fn);
    return TBC_ERR_INVALID_ARG;
  }
  return sf_new(fn, handle, [&](SfObject* S) {
    std::string err;                 // the host plan of the ops (S->enc), then the create of a keyed input over what it made
    if (!sfenc::validate(fn, in, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
    sfenc::plan(in, S->enc);
    const sfenc::Plan& P = S->enc;
    if (P.element.size() >= 0xFFFFFFFFull || P.read_ok.size() >= 0xFFFFFFFFull) {
      set_error("%s: more than 2^32 - 2 elements or reads in one object", fn); return TBC_ERR_INVALID_ARG;
    }
    const tbc_setfull_keys_in made = {in->n_keys, in->device, P.n_elements.data(), P.n_reads.data(), P.add_invoke.data(), P.add_ok.data(),
                                      P.read_invoke.data(), P.read_ok.data(), nullptr, nullptr, nullptr};
    return sf_create(fn, true, &made, SfFrom{SfSource::Ops, nullptr, in->vals}, S);
  });
}

tbc_status tbc_setfull_run(tbc_setfull* handle, tbc_setfull_out* out) { return sf_run_out("tbc_setfull_run", sf_obj(handle), out); }
tbc_status tbc_setfull_keys_run(tbc_setfull_keys* handle, tbc_setfull_keys_out* out) { return sf_run_out("tbc_setfull_keys_run", sf_obj(handle), out); }

tbc_status tbc_setfull_results(tbc_setfull* h, const tbc_setfull_times* times, tbc_setfull_results_out* out) { return sf_results("tbc_setfull_results", sf_obj(h), times, out); }
tbc_status tbc_setfull_keys_results(tbc_setfull_keys* h, const tbc_setfull_times* times, tbc_setfull_results_out* out) { return sf_results("tbc_setfull_keys_results", sf_obj(h), times, out); }

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
