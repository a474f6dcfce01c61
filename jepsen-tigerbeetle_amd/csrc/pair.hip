// pair.hip -- the kernels of tbc_pair_events_batch and the statement of their launches (pair_kernels.h), run here over the library's
// launcher; pair_host.hip (validation, plan, arena, copies) calls pr::launch_pair and pr::launch_emit.
#include "oneshot_launch.h"
#include "pair_kernels.h"

namespace pr {

void launch_pair(void* stream, PrArgs A) {
  oneshot::DeviceLauncher go(stream);
  pair_sequence(go, A);
}

void launch_emit(void* stream, PrArgs A) {
  oneshot::DeviceLauncher go(stream);
  emit_sequence(go, A);
}

}  // namespace pr
