// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_walk_runs.cpp: the front walk in the form the kernel launches it -- a wavefront takes a
// RUN of consecutive chunks of one history, slot cursors carried from chunk to chunk (walk::walk_run, csrc/open_walk_impl.h) -- on the
// CPU under the wavefront emulator of wave_env_emu.h, against the tables host_tables.h builds from the definitions, word for word, as
// emu_walk.cpp does for the one-chunk form.  Also returns the schedule counts of the run (wv::stat): chunks that searched, chunks that
// took carried cursors, slot lanes whose carried cursor was not what the search finds.  Built by tests/emu/walk_runs.py with g++; with
// -DEMU_WALK_RUNS_MAIN it is a program of its own (for a sanitizer build) that reads the batch from a file.
#include "walk_harness.h"

namespace {

struct RunCall { const PackOpenArgs* A; uint32_t run_id; uint32_t* lds; };
template <int VCAP, uint32_t RUN>
void run_entry(void* p, uint32_t lane) {
  auto* c = (RunCall*)p;
  walk::walk_run<VCAP, RUN>(*c->A, c->run_id, c->lds, lane);
}
template <uint32_t RUN>
void run_all(const PackOpenArgs& A, uint32_t nh, uint32_t vpad) {
  const uint32_t rph = walk::walk_runs_per_hist(A.chunks_per_hist, RUN);
  std::vector<uint32_t> lds = WalkHarness::fresh_lds();
  for (uint32_t w = 0; w < nh * rph; w++) {
    WalkHarness::poison_lds(lds);
    RunCall c{&A, w, lds.data()};
    if (vpad <= 8) wv::run_wave(&run_entry<8, RUN>, &c); else wv::run_wave(&run_entry<32, RUN>, &c);
  }
}

// walk_run on a built harness, run chunks a wavefront.  counts = {searches, carried, cursor mismatches, (history, run) pairs that have a
// front, chunks that have fronts}; live_only, not_the_walks: WalkHarness::expected_counts, compare.
int check_runs(WalkHarness& H, uint32_t run, bool live_only, uint64_t not_the_walks, uint64_t* diag, uint64_t* counts) {
  uint64_t before[3];
  for (int i = 0; i < 3; i++) before[i] = wv::stats()[walk::kStatWalkSearch + i];
  if (run == walk::kWalkRun) run_all<walk::kWalkRun>(H.A, H.nh, H.vpad);
  else if (run == 2u) run_all<2u>(H.A, H.nh, H.vpad);
  else run_all<3u>(H.A, H.nh, H.vpad);
  for (int i = 0; i < 3; i++) counts[i] = wv::stats()[walk::kStatWalkSearch + i] - before[i];
  H.expected_counts(run, live_only, counts);
  return H.compare(diag, not_the_walks);
}

}  // namespace

extern "C" {

uint32_t emu_walk_run_length() { return walk::kWalkRun; }

// flags as emu_walk_check's (walk_harness.h WalkFlags).  run: chunks a wavefront takes (0 = the kernel's kWalkRun; 2, 3).
// Returns 0 when every word agrees; else a code (1 lst, 2 twn, 3 rdm, 4 look word 0, 5 look mask, 9 bad input) with diag = {history, front,
// index, got, want}.  counts = {searches, carried, cursor mismatches, (history, run) pairs that have a front, chunks that have fronts}.
int emu_walk_runs_check(uint32_t nh, const uint64_t* op_off, const uint32_t* n_process, const uint8_t* f, const int32_t* a, const int32_t* b,
                        const int32_t* process, const uint32_t* inv_pos, const uint32_t* ret_pos, uint32_t vpad, uint32_t flags, uint32_t run,
                        uint64_t* diag, uint64_t* counts) {
  if (run == 0u) run = walk::kWalkRun;
  if (run != walk::kWalkRun && run != 2u && run != 3u) return 9;
  WalkHarness H;
  if (!H.build(nh, op_off, n_process, f, a, b, process, inv_pos, ret_pos, vpad, WalkFlags(flags), false)) return 9;
  return check_runs(H, run, true, 0ull, diag, counts);
}

}  // extern "C"

#if defined(EMU_WALK_RUNS_MAIN)
// emu_walk_runs FILE: the batch tests/emu/walk_runs.py dump() wrote (u32 nh, vpad, flags, run; then op_off[nh + 1] u64, n_process[nh] u32, and
// per op f u8, a, b, process i32, inv_pos, ret_pos u32, each array padded to 8 bytes).  Exit status 0 = every word equal and no cursor mismatch.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) return 2;
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  for (size_t n; (n = fread(tmp, 1, sizeof tmp, fp)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
  fclose(fp);
  size_t at = 0;
  auto take = [&](size_t bytes) { const uint8_t* p = buf.data() + at; at += (bytes + 7) & ~(size_t)7; if (at > buf.size()) { fprintf(stderr, "short file\n"); exit(2); } return p; };
  uint32_t hd[4];
  memcpy(hd, take(16), 16);
  const uint32_t nh = hd[0];
  std::vector<uint64_t> op_off(nh + 1);
  memcpy(op_off.data(), take(8 * (nh + 1)), 8 * (nh + 1));
  const size_t total = op_off[nh];
  std::vector<uint32_t> npr(nh), inv(total), ret(total);
  std::vector<uint8_t> f(total);
  std::vector<int32_t> a(total), b(total), pr(total);
  memcpy(npr.data(), take(4 * nh), 4 * nh);
  memcpy(f.data(), take(total), total);
  memcpy(a.data(), take(4 * total), 4 * total); memcpy(b.data(), take(4 * total), 4 * total); memcpy(pr.data(), take(4 * total), 4 * total);
  memcpy(inv.data(), take(4 * total), 4 * total); memcpy(ret.data(), take(4 * total), 4 * total);
  uint64_t diag[8] = {0}, counts[8] = {0};
  const int rc = emu_walk_runs_check(nh, op_off.data(), npr.data(), f.data(), a.data(), b.data(), pr.data(), inv.data(), ret.data(), hd[1], hd[2], hd[3], diag, counts);
  printf("rc %d searches %llu carried %llu mismatches %llu runs %llu chunks %llu\n", rc, (unsigned long long)counts[0], (unsigned long long)counts[1],
         (unsigned long long)counts[2], (unsigned long long)counts[3], (unsigned long long)counts[4]);
  return rc != 0 || counts[2] != 0 || counts[0] != counts[3] || counts[0] + counts[1] != counts[4];
}
#endif
