// oneshot_plan.h -- what the host plans of the one-shot entry points that take op columns share (ledger_plan.h, ledger_rt_plan.h,
// ledger_snap_plan.h, ledger_journal_plan.h, ledger_cycles_plan.h, perf_plan.h): plain C++ with no HIP call in it, so the emulator
// programs and the stand-alone plan programs of tests/emu include it as the library does.  The arena's regions, the spans of the
// caller's columns that go into an image, the accounts' sorted order, the chunk size of a scan over whole wavefronts, what a call's
// summary says of its frame, and the one rule of a strided kernel's grid.
//
// THE LAUNCHER CONVENTION.  Each checker states its kernels' order, conditions, grids and block sizes ONCE, as a template at the end of
// its kernels header (lg::sequence, lgrt::sequence, lgsn::filter_sequence / rest_sequence, lgcy::prepare_sequence .. finish_sequence, pf::sequence), written against a launcher
// that names no HIP type:
//   go.launch(kernel, grid, threads, args...)   one launch of `grid` workgroups of `threads` threads
//   go.grid(blocks, cap)                        the workgroups of a kernel that STRIDES: the blocks wanted, `cap` at most
// A kernel that does not stride is given its exact grid.  The library's launcher (oneshot_launch.h) is hipLaunchKernelGGL on a stream and
// capped_grid; the tests' emulator launcher (tests/emu/oneshot_emu.h) runs each workgroup on the CPU and caps lower still, so that the
// strides run; their recording launcher runs nothing and writes the launches down.
//
// THE FRAME INTERFACE.  Each checker states the steps around its kernels ONCE as well -- what is copied in and what is filled, what is
// read back between two runs of kernels, which error ends the call, how many bytes of which region go to which array of the caller's
// -- as the `steps` template at the end of its plan header, written against a call frame `C` that is open and an object `run` with one
// method per sequence of kernels.  The FIRST step that fails sets C.status; every step after it does nothing and returns that status.
//   C.open(device, bytes)                       the arena (and whatever else the call owns)
//   C.base()  C.at(region)                      the arena's start; a region's
//   C.image(img)  C.image(img, at)              an image the plan made to the arena's start, or `at` bytes past it
//   C.put(region, src)                          the caller's or the plan's `region.bytes` bytes to a region
//   C.fill(first, byte, bytes)                  `bytes` from the start of region `first` on set to `byte`
//   C.timed(f)                                  f() launches kernels; the sections of a call add up in C.ns_device()
//   C.get(dst, region[, bytes])                 a region (its first `bytes`) to `dst`, if `dst` is not null
//   C.sync()                                    everything so far is done, what `get` asked for has arrived
//   C.more(bytes)                               a second allocation, once a call, that lives as long as the frame
//   C.fail(status, fmt, ...)                    the call ends here, with this status and message
//   C.status  C.bytes_in  C.ns_device()         where the call stands; what put and image have copied in; the timed sections' sum
// The library's frame is OneShotCall (oneshot_call.h) and its `run` forwards to the checker's launch functions on the frame's stream.
// The tests' frame is emu::Arena (tests/emu/oneshot_emu.h), which checks what a device cannot -- every copy and fill inside the arena,
// no `get` longer than its region, the bytes behind the arena untouched -- and its `run` goes through the emulator's launcher.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace oneshot {

// a named part of a call's one arena; every region starts on a 256 B boundary
struct Region { size_t at = 0, bytes = 0; };
struct Cursor { size_t at = 0; Region take(size_t bytes) { const Region r{at, bytes}; at += (bytes + 255) & ~(size_t)255; return r; } };

// `src` copied to region `r` of an image of the arena's head
inline void put(std::vector<unsigned char>& img, const Region& r, const void* src) {
  if (r.bytes) std::copy((const unsigned char*)src, (const unsigned char*)src + r.bytes, img.begin() + r.at);
}

// micro-ops src .. src + n of the caller's columns lie at dst .. dst + n of the device's
struct Span { uint64_t src, dst, n; };

// the micro-ops the device gets, in the caller's order, neighbours merged
struct Spans {
  std::vector<Span> spans;
  uint64_t n_mops = 0;
  // the caller's lo .. lo + n come next; where they begin on the device
  uint64_t push(uint64_t lo, uint64_t n) {
    const uint64_t at = n_mops;
    if (n && !spans.empty() && spans.back().src + spans.back().n == lo) spans.back().n += n;
    else if (n) spans.push_back(Span{lo, n_mops, n});
    n_mops += n;
    return at;
  }
  // the caller's column `src` of `width`-byte values, gathered to region `r` of an image
  void gather(std::vector<unsigned char>& img, const Region& r, const void* src, size_t width) const {
    for (const Span& s : spans) std::copy((const unsigned char*)src + s.src * width, (const unsigned char*)src + (s.src + s.n) * width, img.begin() + r.at + s.dst * width);
  }
};

// the permutation that sorts the (distinct) accounts: accounts[perm[0]] < accounts[perm[1]] < ...
inline std::vector<uint32_t> sorted_accounts(const int64_t* accounts, uint32_t n) {
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return accounts[a] < accounts[b]; });
  return perm;
}

// the size of a chunk of `items`: whole wavefronts' worth, so that there are `chunks_max` chunks at most
inline uint32_t chunk_size(uint64_t items, uint64_t chunks_max) {
  const uint64_t waves = (items + 63u) / 64u;
  return (uint32_t)(64u * std::max<uint64_t>(1, (waves + chunks_max - 1u) / chunks_max));
}

// where a call stands, written into its summary: the sum of the frame's timed sections and what it has copied in
template <class Frame, class Summary>
void account(Frame& C, Summary& s) { s.ns_device = C.ns_device(); s.bytes_in = C.bytes_in; }

// the grid of a kernel that strides
inline uint32_t capped_grid(uint64_t blocks, uint32_t cap) { return (uint32_t)std::min<uint64_t>(blocks, cap); }

}  // namespace oneshot
