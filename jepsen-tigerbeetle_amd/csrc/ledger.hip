// ledger.hip -- the kernels of tbc_ledger_check and the statement of their launches (ledger_kernels.h), run here over the library's
// launcher; ledger_host.hip (validation, plan, arena, copies) calls lg::launch.
#include "oneshot_launch.h"
#include "ledger_kernels.h"

namespace lg {

void launch(void* stream, LgArgs A, unsigned long long fr_mops, unsigned long long fl_mops) {
  oneshot::DeviceLauncher go(stream);
  sequence<TBC_LEDGER_LOOKUP_WINDOW_WORDS>(go, A, fr_mops, fl_mops);
}

}  // namespace lg
