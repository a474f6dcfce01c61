// ledger_cycles.hip -- the kernels of tbc_ledger_cycles and the statement of their launches (ledger_cycles_kernels.h), run here over the
// library's launcher; ledger_cycles_host.hip (validation, plan, arena, matrices, copies) calls lgcy::launch_prepare, reads the core's
// size back, calls lgcy::launch_describe, then lgcy::launch_round until a round changes nothing, then lgcy::launch_finish.
#include "oneshot_launch.h"
// (the snapshot kernels header comes whole; its pair, key and summary kernels are tbc_ledger_snapshots' and are not launched here)
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "ledger_cycles_kernels.h"

namespace lgcy {

void launch_prepare(void* stream, const CyArgs& A) {
  oneshot::DeviceLauncher go(stream);
  prepare_sequence(go, A);
}

void launch_describe(void* stream, const CyArgs& A) {
  oneshot::DeviceLauncher go(stream);
  describe_sequence(go, A);
}

void launch_round(void* stream, const CyArgs& A, uint32_t round) {
  oneshot::DeviceLauncher go(stream);
  round_sequence(go, A, round);
}

void launch_finish(void* stream, const CyArgs& A, uint32_t final_side, uint32_t rounds) {
  oneshot::DeviceLauncher go(stream);
  finish_sequence(go, A, final_side, rounds);
}

}  // namespace lgcy
