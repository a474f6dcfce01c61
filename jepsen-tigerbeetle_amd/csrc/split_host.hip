// split_host.hip -- tbc_pair_keyed_events (include/tbcheck.h): one keyed event history split by key and paired per key on the device,
// over the call frame of oneshot_call.h: every rule of the arguments on the host (before the device is looked for), the plan, the
// frame, and the steps of the call as sp::steps states them (split_plan.h), the kernels those of split.hip and pair.hip on the frame's
// stream.
#include <new>
#include <string>
#include "oneshot_call.h"
#include "split_plan.h"

using namespace tbc;

extern "C" tbc_status tbc_pair_keyed_events(const tbc_keyed_events* in, tbc_split_out* split, tbc_pair_out* out) {
  const char* fn = "tbc_pair_keyed_events";
  if (!in || !split) { set_error("%s: null argument", fn); return TBC_ERR_INVALID_ARG; }
  try {
    std::string err;
    const tbc_status st = sp::validate(fn, in, split, out, err);
    if (st != TBC_OK) { set_error("%s", err.c_str()); return st; }
    sp::Plan P;
    sp::plan(in, split, out, P);
    struct Run {
      void* stream;
      void keys(const sp::SpArgs& A) { sp::launch_keys(stream, A); }
      void sort(const sp::SpArgs& A) { sp::launch_sort(stream, A); }
      void pair(const pr::PrArgs& A) { pr::launch_pair(stream, A); }
      void emit(const pr::PrArgs& A) { pr::launch_emit(stream, A); }
    };
    OneShotCall C;
    if (C.open(in->device, P.bytes) != TBC_OK) return C.status;
    return sp::steps(C, Run{C.stream}, fn, in, P, split, out);
  } catch (const std::bad_alloc&) {
    set_error("%s: host memory", fn);
    return TBC_ERR_OOM;
  }
}
