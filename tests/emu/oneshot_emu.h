// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  oneshot_emu.h: what the emulator programs of the one-shot checkers share (emu_ledger.cpp,
// emu_ledger_rt.cpp, emu_ledger_snap.cpp, emu_perf.cpp): the qualifiers and the atomics the kernel headers use, stated for the host
// (between two rendezvous the emulator runs one lane at a time; the emulator headers have ballots, lane reads and the workgroup
// barrier), the two launchers the tests run the library's own launch sequences over (csrc/oneshot_plan.h, "the launcher convention"),
// and the arena as the host call frame fills it -- everything the host does not write a pattern, so that what a kernel does not
// write shows.  Include it BEFORE the kernels header.
#pragma once
#include <algorithm>
#include <cstdint>
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

// the arena of a call: 0xA5 all over and 256 B past its end, then what the host call frame writes
struct Arena {
  std::vector<unsigned char> mem;
  explicit Arena(size_t bytes) : mem(bytes + 256, 0xA5) {}
  char* base() { return reinterpret_cast<char*>(mem.data()); }
  char* at(const oneshot::Region& r) { return base() + r.at; }
  void put(const oneshot::Region& r, const void* src) { if (r.bytes) std::memcpy(at(r), src, r.bytes); }
  void image(const std::vector<unsigned char>& img) { if (!img.empty()) std::memcpy(base(), img.data(), img.size()); }
  void fill(const oneshot::Region& first, int byte, size_t bytes) { if (bytes) std::memset(at(first), byte, bytes); }
  void get(void* dst, const oneshot::Region& r, size_t bytes) { if (dst && bytes) std::memcpy(dst, at(r), bytes); }
  void get(void* dst, const oneshot::Region& r) { get(dst, r, r.bytes); }
};

}  // namespace emu
