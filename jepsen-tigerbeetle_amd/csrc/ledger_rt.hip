// ledger_rt.hip -- the kernels of tbc_ledger_realtime and the statement of their launches (ledger_rt_kernels.h), run here over the
// library's launcher; ledger_rt_host.hip (validation, plan, arena, copies) calls lgrt::launch.
#include "oneshot_launch.h"
#include "ledger_rt_kernels.h"

namespace lgrt {

void launch(void* stream, RtArgs A) {
  oneshot::DeviceLauncher go(stream);
  sequence(go, A);
}

}  // namespace lgrt
