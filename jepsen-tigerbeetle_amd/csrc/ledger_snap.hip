// ledger_snap.hip -- the kernels of tbc_ledger_snapshots and the statement of their launches (ledger_snap_kernels.h), run here over the
// library's launcher; ledger_snap_host.hip (validation, plan, arena, copies) calls lgsn::launch_filter, reads the candidates' number back
// and calls lgsn::launch_rest.
#include "oneshot_launch.h"
#include "ledger_snap_kernels.h"

namespace lgsn {

void launch_filter(void* stream, const SnArgs& A) {
  oneshot::DeviceLauncher go(stream);
  filter_sequence(go, A);
}

void launch_rest(void* stream, const SnArgs& A, uint32_t n_candidates) {
  oneshot::DeviceLauncher go(stream);
  rest_sequence(go, A, n_candidates);
}

}  // namespace lgsn
