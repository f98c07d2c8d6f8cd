// bm_sessions_inst.hip -- the build unit of the session table's kernels
// (bm_sessions.hpp), registered with the table's launcher (bm_aux.hip) at load time,
// the way bm_ledger_inst.hip registers the ledger's.  A unit of its own, compiled
// plain (no priority pass), so every other device unit holds what it always held.
#include "bm_sessions.hpp"

extern "C" void bm_register_sessions_kernels(const void* set, const void* tally, const void* retarget);

namespace {
struct Registrar {
    Registrar() {
        bm_register_sessions_kernels(reinterpret_cast<const void*>(&bm::sessions_set_kernel),
                                     reinterpret_cast<const void*>(&bm::sessions_tally_kernel),
                                     reinterpret_cast<const void*>(&bm::sessions_retarget_kernel));
    }
};
const Registrar registrar;
}  // namespace
