// split.hip -- the kernels of tbc_pair_keyed_events' split and the statement of their launches (split_kernels.h), run here over the
// library's launcher; split_host.hip (validation, plan, arena, copies) calls sp::launch_keys and sp::launch_sort.
#include "oneshot_launch.h"
#include "split_kernels.h"

namespace sp {

void launch_keys(void* stream, SpArgs A) {
  oneshot::DeviceLauncher go(stream);
  keys_sequence(go, A);
}

void launch_sort(void* stream, SpArgs A) {
  oneshot::DeviceLauncher go(stream);
  sort_sequence(go, A);
}

}  // namespace sp
