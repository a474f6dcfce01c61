// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_walk_sparse.cpp: the run-form harness of emu_walk_runs.cpp once more, for the SPARSE form of
// the front walk's phase C (csrc/open_walk_impl.h: membership by prefix-XOR of toggle events, no loop over the candidates with lane =
// front).  It adds what that form's tests ask beyond the words: the schedule counts of the form (wv::stat: chunks that took it, chunks that
// took the dense loop, trips of the emission loop, steps down twin chains, value rounds, exact compares where the static twins are
// found) and a switch that sends every chunk through the dense loop.  tests/emu/walk_sparse.py builds it with g++, also with one of the
// planted mutations (-DTBC_WALK_OFF_AFTER=0u, -DTBC_WALK_TWIN_LE, -DTBC_WALK_NO_SELF_EXCLUSION), which the tests must see fail; with
// -DEMU_WALK_RUNS_MAIN it is a program of its own (for a sanitizer build) that reads the batch from a file, as emu_walk_runs.cpp's is.
#include "emu_walk_runs.cpp"

extern "C" {

// out[0 .. 10] = chunks on the sparse form, chunks on the dense loop, emission trips, twin-chain steps, value rounds, twin-find compares,
// chunks of at most 64 / of 65 .. walk::kSparseCand / of more candidates (the last keep the dense loop), the wavefront's steps of B2's
// bucket walk and of the twin chains (the longest lane's)
void emu_walk_sparse_stats(uint64_t* out, int reset) {
  for (int i = 0; i < 11; i++) {
    out[i] = wv::stats()[walk::kStatWalkSparse + i];
    if (reset) wv::stats()[walk::kStatWalkSparse + i] = 0;
  }
}

void emu_walk_force_dense(int on) { walk::emu_force_dense() = on != 0; }

// THE COUNT FORM (tbc_internal.h kHistCount; host_tables.h build_tables(count = true); the slots: walk_harness.h slot_of_op).  This is the
// input under which the sparse form's "one bit per word and index" argument has to hold with slots handed from one process to the next
// inside a chunk.  Arguments and result as emu_walk_runs_check's (run: 0 = the kernel's kWalkRun); word 0 of a lookahead record is compared
// without the bit count_fronts_kernel adds (bit 48: a crashed call of a class producing `need` is invoked by this rank), which is not the
// walk's, and the counts take every history.  Returns 9 for a history the count form refuses.
int emu_walk_sparse_count_check(uint32_t nh, const uint64_t* op_off, const uint32_t* n_process, const uint8_t* f, const int32_t* a, const int32_t* b,
                                const int32_t* process, const uint32_t* inv_pos, const uint32_t* ret_pos, uint32_t vpad, uint32_t flags, uint32_t run,
                                uint64_t* diag, uint64_t* counts) {
  if (run != 0u && run != walk::kWalkRun) return 9;
  WalkHarness H;
  if (!H.build(nh, op_off, n_process, f, a, b, process, inv_pos, ret_pos, vpad, WalkFlags(flags), true)) return 9;
  return check_runs(H, walk::kWalkRun, false, 1ull << 48, diag, counts);
}

}  // extern "C"
