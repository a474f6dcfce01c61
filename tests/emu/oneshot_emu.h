// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  oneshot_emu.h: what the emulator programs of the one-shot checkers share (emu_ledger.cpp,
// emu_ledger_rt.cpp, emu_ledger_snap.cpp, emu_ledger_journal.cpp, emu_ledger_cycles.cpp, emu_perf.cpp): the qualifiers and the atomics
// the kernel headers use, stated for the host (between two rendezvous the emulator runs one lane at a time; the emulator headers have
// ballots, lane reads and the workgroup barrier), the two launchers the tests run the library's own launch sequences over
// (csrc/oneshot_plan.h, "the launcher convention"), and the call frame the tests run the library's own step lists over (the same
// header, "the frame interface") -- everything the step list does not write a pattern, so that what a kernel does not write shows;
// every copy held to the arena's and its region's bounds.  Include it BEFORE the kernels header.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "tbcheck.h"
#define TBC_EMU 1
#include "wave_env_emu.h"
#include "wave_env_wg_emu.h"
#include "oneshot_plan.h"

#define __global__
#define __launch_bounds__(...)
#define __forceinline__ inline
#define __shared__ static
#define __popcll(x) __builtin_popcountll(x)
#define __popc(x) __builtin_popcount(x)
static inline uint32_t atomicCAS(uint32_t* p, uint32_t expected, uint32_t desired) { const uint32_t o = *p; if (o == expected) *p = desired; return o; }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p |= v; return o; }
static inline uint32_t atomicMin(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v < o) *p = v; return o; }
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) { const uint32_t o = *p; if (v > o) *p = v; return o; }
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; if (v < o) *p = v; return o; }
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; if (v > o) *p = v; return o; }

namespace emu {

// Runs nothing: the device's caps, and each launch written down as (kernel, grid, threads)
struct Recorder {
  using Kernel = void (*)();
  struct Launch {
    Kernel kernel; uint32_t grid, threads;
    bool operator==(const Launch& o) const { return kernel == o.kernel && grid == o.grid && threads == o.threads; }
  };
  std::vector<Launch> launches;
  uint32_t grid(uint64_t blocks, uint32_t cap) const { return oneshot::capped_grid(blocks, cap); }
  template <class... P, class... A>
  void launch(void (*kernel)(P...), uint32_t grid, uint32_t threads, const A&...) { launches.push_back(Launch{of(kernel), grid, threads}); }
  // a kernel as the record names it: of(lg_si_kernel), of(rt_carry_kernel<true>)
  template <class... P>
  static Kernel of(void (*kernel)(P...)) { return reinterpret_cast<Kernel>(kernel); }
  // the record is `want`, launch for launch; if not, where they part is printed
  bool is(const std::vector<Launch>& want) const {
    for (size_t k = 0; k < std::max(launches.size(), want.size()); k++) {
      if (k < launches.size() && k < want.size() && launches[k] == want[k]) continue;
      std::printf("launch %zu of %zu (want %zu):", k, launches.size(), want.size());
      if (k < launches.size()) std::printf(" got %s kernel, grid %u x %u threads;", k < want.size() && launches[k].kernel == want[k].kernel ? "the right" : "another", launches[k].grid, launches[k].threads);
      if (k < want.size()) std::printf(" want grid %u x %u threads", want[k].grid, want[k].threads);
      std::printf("\n");
      return false;
    }
    return true;
  }
};

// Runs every workgroup of a launch under the wavefront / workgroup emulator, one after the other.  A strided grid is capped at
// `grid_cap` workgroups as well as at the sequence's own cap, so that the strides run; the waves of a workgroup are its threads / 64; the
// schedule's seed moves on with every launch and workgroup.  What it ran is in `ran`.
struct Launcher {
  uint32_t grid_cap;
  uint64_t seed;
  Recorder ran;
  Launcher(uint32_t cap, uint64_t s) : grid_cap(cap ? cap : 1u), seed(s) {}
  uint32_t grid(uint64_t blocks, uint32_t cap) const { return oneshot::capped_grid(blocks, std::min(cap, grid_cap)); }
  template <class... P, class... A>
  void launch(void (*kernel)(P...), uint32_t grid, uint32_t threads, const A&... args) {
    std::function<void()> body = [&] { kernel(static_cast<P>(args)...); };
    for (uint32_t b = 0; b < grid; b++) wv::run_workgroup(trampoline, &body, (int)((threads + 63u) / 64u), b, seed + 1000u * ran.launches.size() + b);
    ran.launch(kernel, grid, threads);
  }
  static void trampoline(void* arg, uint32_t) { (*static_cast<std::function<void()>*>(arg))(); }
};

// The call frame on the CPU (csrc/oneshot_plan.h, "the frame interface"; the library's is OneShotCall of csrc/oneshot_call.h): the arena,
// and the second allocation, 0xA5 all over and 256 B past their ends, then what the step list writes.  It checks what a device cannot:
// every put, fill and get lies inside the arena, no get is longer than its region, and -- `close`, at the end of the call -- the 256 B
// behind either allocation are still 0xA5.  A violation does not abort: it is the call's status, TBC_ERR_HIP, and its message in `err`
// (the program's error string, which `fail` writes as the library writes tbc_last_error).
struct Arena {
  using Region = oneshot::Region;
  std::string& err;
  tbc_status status = TBC_OK;
  uint64_t bytes_in = 0;
  size_t bytes = 0;                                          // the arena's, without its guard
  std::vector<unsigned char> mem, extra;
  explicit Arena(std::string& e) : err(e) {}

  template <class... A>
  tbc_status fail(tbc_status st, const char* fmt, const A&... a) {
    if (status != TBC_OK) return status;
    char buf[512];
    std::snprintf(buf, sizeof buf, fmt, a...);
    err = buf;
    return status = st;
  }
  tbc_status open(uint32_t, size_t arena_bytes) { bytes = arena_bytes; mem.assign(bytes + 256, 0xA5); return status; }
  char* more(size_t n) { extra.assign(n + 256, 0xA5); return reinterpret_cast<char*>(extra.data()); }
  char* base() { return reinterpret_cast<char*>(mem.data()); }
  char* at(const Region& r) { return base() + r.at; }

  tbc_status put(const Region& r, const void* src) { return copy("put", at(r), src, r.at, r.bytes, r.bytes, true); }
  tbc_status image(const std::vector<unsigned char>& img, size_t first = 0) { return copy("image", base() + first, img.data(), first, img.size(), img.size(), true); }
  tbc_status fill(const Region& first, int byte, size_t n) {
    if (ok("fill", first.at, n, n) && n) std::memset(at(first), byte, n);
    return status;
  }
  template <class Launches>
  tbc_status timed(Launches launches) { if (status == TBC_OK) launches(); return status; }
  tbc_status get(void* dst, const Region& r, size_t n) { return copy("get", dst, at(r), r.at, n, r.bytes, false); }
  tbc_status get(void* dst, const Region& r) { return get(dst, r, r.bytes); }
  tbc_status sync() { return status; }
  uint64_t ns_device() const { return 0; }
  // the end of the call: the guards are as `open` and `more` left them, or THAT is what the call came to
  tbc_status close() {
    for (const std::vector<unsigned char>* m : {&mem, &extra})
      for (size_t k = 0; k < 256 && k < m->size(); k++)
        if ((*m)[m->size() - 256 + k] != 0xA5) {
          status = TBC_OK;
          return fail(TBC_ERR_HIP, "emu::Arena: byte %zu behind %s was written", k, m == &mem ? "the arena" : "the second allocation");
        }
    return status;
  }

 private:
  // the call has not failed, and `n` bytes at `first` are `most` at most and inside the arena
  bool ok(const char* what, size_t first, size_t n, size_t most) {
    if (n > most || first > bytes || n > bytes - first) fail(TBC_ERR_HIP, "emu::Arena: a %s of %zu bytes at %zu: its region has %zu, the arena %zu", what, n, first, most, bytes);
    return status == TBC_OK;
  }
  tbc_status copy(const char* what, void* dst, const void* src, size_t first, size_t n, size_t most, bool in) {
    if (!ok(what, first, n, most)) return status;
    if (in) bytes_in += n;
    if (dst && n) std::memcpy(dst, src, n);
    return status;
  }
};

}  // namespace emu
