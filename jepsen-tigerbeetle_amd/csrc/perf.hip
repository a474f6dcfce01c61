// perf.hip -- the kernels of tbc_perf_series and the statement of their launches (perf_kernels.h), run here over the library's launcher;
// perf_host.hip (validation, plan, arena, copies) calls pf::launch.
#include "oneshot_launch.h"
#include "perf_kernels.h"

namespace pf {

void launch(void* stream, PfArgs A) {
  oneshot::DeviceLauncher go(stream);
  sequence(go, A);
}

}  // namespace pf
