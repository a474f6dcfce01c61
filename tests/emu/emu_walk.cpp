// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_walk.cpp: runs the front walk with lane = front, one chunk a wavefront from nothing
// (walk::walk_wave, csrc/open_walk_impl.h), on the CPU under the wavefront emulator of wave_env_emu.h and compares EVERY WORD it writes
// with the tables host_tables.h builds from the definitions.  The inputs, the outputs and the comparison are walk_harness.h's.  Built by
// tests/emu with g++; nothing under jepsen-tigerbeetle_amd/ links it.
#include "walk_harness.h"

namespace {

struct WalkCall { const PackOpenArgs* A; uint32_t wave; uint32_t* lds; };
template <int VCAP>
void walk_entry(void* p, uint32_t lane) {
  auto* c = (WalkCall*)p;
  walk::walk_wave<VCAP>(*c->A, c->wave, c->lds, lane);
}

}  // namespace

extern "C" {

// flags: walk_harness.h WalkFlags.
// Returns 0 when every word agrees; else a code (1 lst, 2 twn, 3 rdm, 4 look word 0, 5 look mask, 6 tmp, 9 bad input) with
// diag = {history, front, index, got, want}.
int emu_walk_check(uint32_t nh, const uint64_t* op_off, const uint32_t* n_process, const uint8_t* f, const int32_t* a, const int32_t* b,
                   const int32_t* process, const uint32_t* inv_pos, const uint32_t* ret_pos, uint32_t vpad, uint32_t flags, uint64_t* diag) {
  if (flags & 32u) return 9;          // (was: the lean formats -- deleted in round 5)
  WalkHarness H;
  if (!H.build(nh, op_off, n_process, f, a, b, process, inv_pos, ret_pos, vpad, WalkFlags(flags), false)) return 9;
  std::vector<uint32_t> lds = WalkHarness::fresh_lds();
  for (uint32_t w = 0; w < nh * H.A.chunks_per_hist; w++) {
    WalkHarness::poison_lds(lds);
    WalkCall c{&H.A, w, lds.data()};
    if (vpad <= 8) wv::run_wave(&walk_entry<8>, &c); else wv::run_wave(&walk_entry<32>, &c);
  }
  return H.compare(diag);
}

}  // extern "C"
