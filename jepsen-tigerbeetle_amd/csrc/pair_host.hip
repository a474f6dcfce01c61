// pair_host.hip -- tbc_pair_events_batch and tbc_pair_packed_batch (the same call over packed events: 8 B a row), the entry points
// of the pairing on the device (include/tbcheck.h), over the call frame of
// oneshot_call.h: every rule of the arguments on the host (before the device is looked for), the plan, the frame, and the steps of the
// call as pr::steps states them (pair_plan.h), the kernels those of pair.hip on the frame's stream.
#include <string>
#include "oneshot_call.h"
#include "pair_plan.h"

using namespace tbc;

namespace {

template <class In>
tbc_status pr_batch(const char* fn, const In* in, tbc_pair_out* out) {
  std::string err;
  const tbc_status st = pr::validate(fn, in, out, err);
  if (st != TBC_OK) { set_error("%s", err.c_str()); return st; }
  pr::Plan P;
  pr::plan(in, out, P);
  struct Run {
    void* stream;
    void pair(const pr::PrArgs& A) { pr::launch_pair(stream, A); }
    void emit(const pr::PrArgs& A) { pr::launch_emit(stream, A); }
  };
  OneShotCall C;
  if (C.open(in->device, P.arena.bytes) != TBC_OK) return C.status;
  return pr::steps(C, Run{C.stream}, fn, in, P, out);
}

}  // namespace

extern "C" tbc_status tbc_pair_events_batch(const tbc_event_batch* in, tbc_pair_out* out) {
  return oneshot_entry("tbc_pair_events_batch", in, out, pr_batch<tbc_event_batch>);
}

extern "C" tbc_status tbc_pair_packed_batch(const tbc_packed_event_batch* in, tbc_pair_out* out) {
  return oneshot_entry("tbc_pair_packed_batch", in, out, pr_batch<tbc_packed_event_batch>);
}
