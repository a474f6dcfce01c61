// enc_table.h -- the open-addressing table of int64 values two encodings share: set-full's elements of a key (set_full_encode.h,
// sf_table_build_kernel: value -> column) and the ledger's invoked transfer ids (ledger_kernels.h: id -> number).  16 B slots
// {value, column + 1}, a capacity of the power of two at or above twice the values (sfenc::table_slots), linear probing; a slot is claimed
// by a CAS on its column word and the value written behind it, so the build's kernel boundary comes before every probe.  The slot is
// plain C++ (the planners size the tables); the probe is device code (and the emulator's).
#pragma once
#include <cstdint>

namespace {

constexpr uint32_t kNoneU = 0xFFFFFFFFu;

struct alignas(16) SfEncSlot { long long value; uint32_t col1, pad; };       // col1 = column + 1, 0 = free

#if defined(__HIPCC__) || defined(TBC_EMU)
__device__ __forceinline__ uint32_t sf_enc_hash(long long v) {               // (the finaliser of splitmix64)
  unsigned long long x = (unsigned long long)v;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return (uint32_t)x;
}

// the column of value v in a table, kNoneU if it holds no such value.  The table is at most half full: a probe sequence ends.
__device__ __forceinline__ uint32_t sf_enc_lookup(const SfEncSlot* __restrict__ tab, uint32_t mask, long long v) {
  uint32_t s = sf_enc_hash(v) & mask;
  for (;;) {
    const SfEncSlot e = tab[s];
    if (e.col1 == 0u) return kNoneU;
    if (e.value == v) return e.col1 - 1u;
    s = (s + 1u) & mask;
  }
}
#endif

}  // namespace
