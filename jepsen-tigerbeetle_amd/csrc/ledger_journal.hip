// ledger_journal.hip -- the kernels of tbc_ledger_journal and the statement of their launches (ledger_journal_kernels.h), run here over
// the library's launcher; ledger_journal_host.hip (validation, plan, arena, copies) calls lgjn::launch.
#include "oneshot_launch.h"
#include "ledger_journal_kernels.h"

namespace lgjn {

void launch(void* stream, const JnArgs& A) {
  oneshot::DeviceLauncher go(stream);
  sequence<kJnWindowWords>(go, A);
}

}  // namespace lgjn
