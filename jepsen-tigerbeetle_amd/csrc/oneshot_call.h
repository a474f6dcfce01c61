// oneshot_call.h -- the host call frame of the one-shot entry points that take op columns (tbc_ledger_check, tbc_ledger_realtime,
// tbc_ledger_snapshots, tbc_ledger_journal, tbc_ledger_cycles, tbc_perf_series): the HIP error macro, the extern "C" wrapper, and
// OneShotCall -- what one call makes on the device (ONE arena laid out by the plan, a stream and two events of its own; for the cycle
// search a second allocation) and the steps every such call takes, released on every path out.  One-shot and re-entrant: nothing
// outlives the call.  Each checker's LIST of steps is the `steps` template of its plan header, written against THE FRAME INTERFACE
// (oneshot_plan.h) that this struct and the emulator's arena of tests/emu/oneshot_emu.h both meet; a host unit validates, plans, opens
// the frame and calls it.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>
#include "oneshot_plan.h"
#include "tbc_internal.h"

#define TBC_ONESHOT_TRY(expr)                                                                     \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      tbc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
      return e_ == hipErrorOutOfMemory ? TBC_ERR_OOM : TBC_ERR_HIP;                               \
    }                                                                                             \
  } while (0)

namespace tbc {

// One call's frame.  The FIRST step that fails sets `status` (and the error text, through TBC_ONESHOT_TRY); every step after it does
// nothing and returns that status, so a step list reads as a list and looks at the status where it must: before it reads what a `sync`
// brought back.  The copies read and write pageable memory of the caller's, of the plan's and of the step list's: it lives until the
// next `sync`, which waits for the stream on a failed call too -- a step list returns only after one.
struct OneShotCall {
  using Region = oneshot::Region;
  tbc_status status = TBC_OK;
  uint64_t bytes_in = 0;                                    // what `put` and `image` have copied in
  int device_before = -1;                                   // the calling thread's current device, put back on the way out
  void *arena = nullptr, *extra = nullptr;                  // (`extra`: what `more` made)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool section_open = false;                                // ev0 .. ev1 are recorded and not yet added to ms
  double ms = 0;

  // released in this order whichever way the call ends
  ~OneShotCall() {
    if (stream) (void)hipStreamSynchronize(stream);       // (a call that failed half way may have left a copy or a kernel in flight)
    if (extra) (void)hipFree(extra);
    if (arena) (void)hipFree(arena);
    for (hipEvent_t e : {ev0, ev1}) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (device_before >= 0) (void)hipSetDevice(device_before);
  }

  template <class Step>
  tbc_status step(Step s) { return status == TBC_OK ? (status = s()) : status; }

  // the device is a gfx950 and becomes the thread's current one; the arena (256 B at least), the stream, the events
  tbc_status open(uint32_t device, size_t arena_bytes) {
    return step([&]() -> tbc_status {
      int ndev = 0;
      hipDeviceProp_t prop;
      if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || (int)device >= ndev) { set_error("no usable HIP device; libtbcheck has no CPU fallback"); return TBC_ERR_NO_DEVICE; }
      if (hipGetDeviceProperties(&prop, (int)device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_error("device %u is not a gfx950 (MI355X) device", device); return TBC_ERR_NO_DEVICE; }
      TBC_ONESHOT_TRY(hipGetDevice(&device_before));
      TBC_ONESHOT_TRY(hipSetDevice((int)device));
      TBC_ONESHOT_TRY(hipMalloc(&arena, std::max<size_t>(arena_bytes, 256)));
      TBC_ONESHOT_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      TBC_ONESHOT_TRY(hipEventCreate(&ev0)); TBC_ONESHOT_TRY(hipEventCreate(&ev1));
      return TBC_OK;
    });
  }
  // a second allocation that lives as long as the frame (one a call; null once the call has failed)
  char* more(size_t bytes) {
    step([&]() -> tbc_status { TBC_ONESHOT_TRY(hipMalloc(&extra, bytes)); return TBC_OK; });
    return static_cast<char*>(extra);
  }
  // the call ends here, with `st` and this message
  template <class... A>
  tbc_status fail(tbc_status st, const char* fmt, const A&... a) {
    return step([&]() -> tbc_status { set_error(fmt, a...); return st; });
  }
  char* base() const { return static_cast<char*>(arena); }
  char* at(const Region& r) const { return base() + r.at; }

  // `src` to region `r`; an image of the plan's to the arena's start, or `at` bytes past it
  tbc_status put(const Region& r, const void* src) { return copy_in(at(r), src, r.bytes); }
  tbc_status image(const std::vector<unsigned char>& img, size_t at = 0) { return copy_in(base() + at, img.data(), img.size()); }
  // `bytes` from the start of region `first` on (several regions in a row) set to 0x00 or 0xFF
  tbc_status fill(const Region& first, int byte, size_t bytes) {
    return step([&]() -> tbc_status {
      if (bytes) TBC_ONESHOT_TRY(hipMemsetAsync(at(first), byte, bytes, stream));
      return TBC_OK;
    });
  }
  // `launches` between the two events; the sections of one call add up in ns_device
  template <class Launches>
  tbc_status timed(Launches launches) {
    return step([&]() -> tbc_status {
      TBC_ONESHOT_TRY(hipEventRecord(ev0, stream));
      launches();
      TBC_ONESHOT_TRY(hipGetLastError());
      TBC_ONESHOT_TRY(hipEventRecord(ev1, stream));
      section_open = true;
      return TBC_OK;
    });
  }
  // an array the caller asked for (not null, not empty) out of region `r`
  tbc_status get(void* dst, const Region& r, size_t bytes) {
    return step([&]() -> tbc_status {
      if (dst && bytes) TBC_ONESHOT_TRY(hipMemcpyAsync(dst, at(r), bytes, hipMemcpyDeviceToHost, stream));
      return TBC_OK;
    });
  }
  tbc_status get(void* dst, const Region& r) { return get(dst, r, r.bytes); }
  // everything so far is done: the copies have arrived, a timed section is measured (a failed call: whatever is still in flight has landed)
  tbc_status sync() {
    if (status != TBC_OK && stream) (void)hipStreamSynchronize(stream);
    return step([&]() -> tbc_status {
      TBC_ONESHOT_TRY(hipStreamSynchronize(stream));
      if (section_open) {
        float section = 0;
        TBC_ONESHOT_TRY(hipEventElapsedTime(&section, ev0, ev1));
        ms += (double)section;
        section_open = false;
      }
      return TBC_OK;
    });
  }
  uint64_t ns_device() const { return (uint64_t)(ms * 1e6); }

 private:
  tbc_status copy_in(void* dst, const void* src, size_t bytes) {
    return step([&]() -> tbc_status {
      bytes_in += bytes;
      if (bytes) TBC_ONESHOT_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
      return TBC_OK;
    });
  }
};

// the extern "C" entry point around `body(fn, in, out)`: null arguments refused, the host's bad_alloc as TBC_ERR_OOM
template <class In, class Out, class Body>
tbc_status oneshot_entry(const char* fn, const In* in, Out* out, Body body) {
  if (!in || !out) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  try {
    return body(fn, in, out);
  } catch (const std::bad_alloc&) {
    set_error("%s: host memory", fn);
    return TBC_ERR_OOM;
  }
}

}  // namespace tbc
