// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  emu_walk_lines.cpp: the sparse-form harness of emu_walk_sparse.cpp once more, for what the sparse
// form's list stores with LANE = ENTRY add (csrc/open_walk_impl.h, sparse_lists: a chunk's entries taken 64 at a time, an entry lane finds
// its front by the marks of the fronts' first entries and its candidate as the k-th set bit of the front's words).  Beside the words of the
// run form it runs every chunk ONCE MORE from nothing (walk::walk_wave, over freshly poisoned lists) and holds, PER CHUNK, the form's counts
// (wv::stat) against the host-built tables: the passes of 64 entries a chunk makes against ceil(entries / 64), its entries against
// off[F_hi] - off[F_lo], and that no front's off[] is anywhere but at the running sum of the counts of the chunk's fronts before it.
// tests/emu/walk_lines.py builds it with g++, also with one of the planted mutations (-DTBC_WALK_RANK_OFF_BY_ONE, -DTBC_WALK_FRONT_LE), which
// the tests must see fail; with -DEMU_WALK_LINES_MAIN it is a program of its own (for a sanitizer build) that reads the batch from a file
// (tests/emu/walk_runs.py dump(); the run word's bit 8 = count form).
#include "emu_walk_sparse.cpp"

namespace {

struct ChunkCall { const PackOpenArgs* A; uint32_t wave; uint32_t* lds; };
void chunk_entry(void* p, uint32_t lane) {
  auto* c = (ChunkCall*)p;
  walk::walk_wave<8>(*c->A, c->wave, c->lds, lane);
}

}  // namespace

extern "C" {

// Arguments as emu_walk_runs_check's (rows of at most 8 entries; the kernel's run length), then count_form and what the lines form adds:
//   lines[0 .. 9] = chunks that have fronts, chunks on the sparse form, passes of 64 entries made, passes expected (the sum of
//                   ceil(entries / 64) over the sparse chunks), entries the sparse chunks counted, entries expected, chunks whose own passes
//                   or entries are not the expected ones, fronts whose off[] is not at the running sum, entries without a candidate,
//                   entries whose place is in the second set of 64
//   chunk_entries[i], chunk_sparse[i]: per chunk that has fronts, history by history (at most cap of them): its entries by off[], and
//                   whether it took the sparse form
// Returns 0 when every word agrees in both forms, else emu_walk_runs_check's codes (+ 16 when the difference is in the chunk-by-chunk form).
int emu_walk_lines_check(uint32_t nh, const uint64_t* op_off, const uint32_t* n_process, const uint8_t* f, const int32_t* a, const int32_t* b,
                         const int32_t* process, const uint32_t* inv_pos, const uint32_t* ret_pos, uint32_t vpad, uint32_t flags, uint32_t count_form,
                         uint64_t* diag, uint64_t* counts, uint64_t* lines, uint32_t* chunk_entries, uint8_t* chunk_sparse, uint32_t cap) {
  if (vpad > 8u) return 9;
  WalkHarness H;
  if (!H.build(nh, op_off, n_process, f, a, b, process, inv_pos, ret_pos, vpad, WalkFlags(flags), count_form != 0u)) return 9;
  const int rc = check_runs(H, walk::kWalkRun, count_form == 0u, count_form ? 1ull << 48 : 0ull, diag, counts);
  if (rc != 0) return rc;
  // every chunk once more, from nothing, over poisoned lists: the form's counts chunk by chunk
  std::fill(H.lst.begin(), H.lst.end(), OpRec{0xA5A5A5A5u, 0xA5A5A5A5u, (int32_t)0xA5A5A5A5, (int32_t)0xA5A5A5A5});
  std::fill(H.twn.begin(), H.twn.end(), 0xA5A5A5A5A5A5A5A5ull);
  for (int i = 0; i < 10; i++) lines[i] = 0;
  uint64_t* const st = wv::stats();
  std::vector<uint32_t> lds = WalkHarness::fresh_lds();
  for (uint32_t h = 0; h < nh; h++) {
    if (H.T.hist[h].status != 0 || H.T.bh[h].status != 0) continue;
    const uint32_t R = H.T.hist[h].n_ret;
    const uint32_t* off = H.T.off.data() + H.T.bh[h].off_off;
    for (uint32_t c = 0; c * 64u < R; c++) {
      const uint64_t sparse0 = st[walk::kStatWalkSparse], passes0 = st[walk::kStatWalkEmitTrips], entries0 = st[walk::kStatWalkEntries];
      const uint64_t apart0 = st[walk::kStatWalkNotContiguous], bad0 = st[walk::kStatWalkBadPlace], second0 = st[walk::kStatWalkSecondSet];
      WalkHarness::poison_lds(lds);
      ChunkCall call{&H.A, h * H.A.chunks_per_hist + c, lds.data()};
      wv::run_wave(&chunk_entry, &call);
      const bool sparse = st[walk::kStatWalkSparse] != sparse0;
      const uint32_t F_hi = c * 64u + 64u < R ? c * 64u + 64u : R;
      const uint64_t want_entries = off[F_hi] - off[c * 64u], want_passes = (want_entries + 63u) / 64u;
      const uint64_t passes = st[walk::kStatWalkEmitTrips] - passes0, entries = st[walk::kStatWalkEntries] - entries0;
      if (lines[0] < cap) { chunk_entries[lines[0]] = (uint32_t)want_entries; chunk_sparse[lines[0]] = sparse ? 1u : 0u; }
      lines[0]++;
      if (sparse) {
        lines[1]++; lines[2] += passes; lines[3] += want_passes; lines[4] += entries; lines[5] += want_entries;
        if (passes != want_passes || entries != want_entries) lines[6]++;
      } else if (passes != 0u || entries != 0u) lines[6]++;           // (the dense loop makes no pass)
      lines[7] += st[walk::kStatWalkNotContiguous] - apart0; lines[8] += st[walk::kStatWalkBadPlace] - bad0; lines[9] += st[walk::kStatWalkSecondSet] - second0;
    }
  }
  const int rc2 = H.compare(diag, count_form ? 1ull << 48 : 0ull);
  return rc2 ? rc2 + 16 : 0;
}

// one of the emulated run's schedule counts by its id (open_walk_impl.h kStatWalk...), as it stands
uint64_t emu_walk_stat(uint32_t id) { return wv::stats()[id & 63u]; }

}  // extern "C"

#if defined(EMU_WALK_LINES_MAIN)
// emu_walk_lines FILE: the batch tests/emu/walk_runs.py dump() wrote (see emu_walk_runs.cpp's main); bit 8 of its run word = count form.
// Exit status 0 = every word equal in both forms, no cursor mismatch, every chunk's passes and entries the expected ones.
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
  uint64_t diag[8] = {0}, counts[8] = {0}, lines[10] = {0};
  const uint32_t cap = (uint32_t)(total / 64 + nh + 1);
  std::vector<uint32_t> ce(cap);
  std::vector<uint8_t> cs(cap);
  const int rc = emu_walk_lines_check(nh, op_off.data(), npr.data(), f.data(), a.data(), b.data(), pr.data(), inv.data(), ret.data(), hd[1], hd[2], (hd[3] >> 8) & 1u,
                                      diag, counts, lines, ce.data(), cs.data(), cap);
  printf("rc %d mismatches %llu chunks %llu sparse %llu passes %llu of %llu entries %llu of %llu off %llu apart %llu no-candidate %llu\n", rc, (unsigned long long)counts[2],
         (unsigned long long)lines[0], (unsigned long long)lines[1], (unsigned long long)lines[2], (unsigned long long)lines[3], (unsigned long long)lines[4],
         (unsigned long long)lines[5], (unsigned long long)lines[6], (unsigned long long)lines[7], (unsigned long long)lines[8]);
  return rc != 0 || counts[2] != 0 || lines[2] != lines[3] || lines[4] != lines[5] || lines[6] != 0 || lines[7] != 0 || lines[8] != 0;
}
#endif
