// ledger_cycles_host.hip -- tbc_ledger_cycles, the entry point of the cycle search over a ledger's reads (include/tbcheck.h), over the
// call frame of oneshot_call.h: every rule of the input on the host, the plan (ledger_cycles_plan.h), the snapshot plan's image and this
// checker's head as two copies, the kernels that separate clean reads from the core (ledger_cycles.hip), the accumulators back -- the
// core's size decides whether the call goes on, and how large the two bit matrices are, which are allocated only now --, the
// descriptors and the matrix, one squaring per round with the changed flag read back after each, the rest of the kernels, the summary
// back, and then one copy per array the caller asked for.  Every run of kernels is a timed section; ns_device is their sum.
#include <cstddef>
#include <string>
#include <vector>
#include "oneshot_call.h"
#include "ledger_cycles_plan.h"

using namespace tbc;

namespace {

// the core's two matrices: released once the stream has run dry (declared after the call frame, so released before it)
struct Matrices {
  hipStream_t stream = nullptr;
  void* p = nullptr;
  ~Matrices() {
    if (!p) return;
    if (stream) (void)hipStreamSynchronize(stream);
    (void)hipFree(p);
  }
};

tbc_status cycles_check(const char* fn, const tbc_ledger_rt_in* in, tbc_ledger_cycles_out* out) {
  std::string err;
  lgcy::Plan P;
  if (!lgcy::validate(fn, in, err) || !lgcy::plan(fn, in, P, err)) { set_error("%s", err.c_str()); return TBC_ERR_INVALID_ARG; }
  const lgsn::SnArena& S = P.sn.arena;
  const lgcy::CyArena& L = P.arena;
  const std::vector<unsigned char> img = lgsn::image(&in->ledger, P.sn), head = lgcy::head_image(P);
  lgsn::SnAcc sn_acc{};
  lgcy::CyAcc acc{};
  uint32_t changed = 0;
  OneShotCall C;
  Matrices M;
  if (C.open(in->ledger.device, L.bytes) != TBC_OK) return C.status;
  C.image(img);
  C.put(oneshot::Region{L.head_at(), L.head_bytes()}, head.data());
  C.fill(S.val, 0, S.zero_bytes());
  lgcy::CyArgs A = lgcy::args(in, P, C.base());
  C.timed([&] { lgcy::launch_prepare(C.stream, A); });
  C.get(&sn_acc, S.acc, sizeof sn_acc);
  C.get(&acc, L.acc, sizeof acc);
  if (C.sync() != TBC_OK) return C.status;
  tbc_ledger_cycles_summary& s = out->summary;
  s = tbc_ledger_cycles_summary{};
  s.read_count = P.sn.n_reads; s.n_partial = sn_acc.n_partial; s.n_core = acc.n_core; s.bad_values = sn_acc.bad_values; s.n_checked = sn_acc.n_checked;
  s.first = s.largest = lgcy::kCyNone;
  s.ns_device = C.ns_device(); s.bytes_in = C.bytes_in;
  if (s.bad_values) {
    set_error("%s: %u reads hold counters whose magnitudes add up to 2^63 or more", fn, s.bad_values);
    return TBC_ERR_UNSUPPORTED;
  }
  if (s.n_core > TBC_LEDGER_CYCLES_MAX_CORE) {
    set_error("%s: %u reads are partial, skewed or contradicted by real time; the search takes %u at most", fn, s.n_core, TBC_LEDGER_CYCLES_MAX_CORE);
    return TBC_ERR_UNSUPPORTED;
  }
  uint32_t rounds = 0, final_side = 0;
  if (acc.n_core) {
    M.stream = C.stream;
    C.step([&]() -> tbc_status {
      TBC_ONESHOT_TRY(hipMalloc(&M.p, 2 * lgcy::matrix_bytes(acc.n_core)));
      return TBC_OK;
    });
    if (C.status != TBC_OK) return C.status;
    A = lgcy::with_matrix(A, acc.n_core, static_cast<char*>(M.p));
    for (;;) {
      C.timed([&] {
        if (!rounds) lgcy::launch_describe(C.stream, A);
        lgcy::launch_round(C.stream, A, rounds);
      });
      C.get(&changed, oneshot::Region{L.acc.at + offsetof(lgcy::CyAcc, changed) + 4u * rounds, 4u});
      if (C.sync() != TBC_OK) return C.status;
      final_side = (rounds & 1u) ^ 1u;
      rounds++;
      if (!changed) break;
      if (rounds == lgcy::kCyMaxRounds) { set_error("%s: the closure did not settle in %u rounds", fn, rounds); return TBC_ERR_HIP; }
    }
  }
  C.timed([&] { lgcy::launch_finish(C.stream, A, final_side, rounds); });
  C.get(&out->summary, L.summary, sizeof(tbc_ledger_cycles_summary));
  if (C.sync() != TBC_OK) return C.status;
  out->summary.ns_device = C.ns_device();
  out->summary.bytes_in = C.bytes_in;
  const size_t R = P.sn.n_reads;
  C.get(out->scc, L.scc, R * 4); C.get(out->cyc_flags, L.cyc_flags, R);
  return C.sync();
}

}  // namespace

extern "C" tbc_status tbc_ledger_cycles(const tbc_ledger_rt_in* in, tbc_ledger_cycles_out* out) { return oneshot_entry("tbc_ledger_cycles", in, out, cycles_check); }
