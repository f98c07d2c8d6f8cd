// bm_ledger_inst.hip -- the build unit of the ledger's kernels (bm_ledger.hpp),
// registered with bm_ledger_verify_jobs's launcher (bm_aux.hip) at load time, the way
// bm_share_set_inst.hip registers the share set's.  A unit of its own, compiled
// plain (no priority pass), so every other device unit holds what it always held.
#include "bm_ledger.hpp"

extern "C" void bm_register_ledger_kernels(const void* credit, const void* fill);

namespace {
struct Registrar {
    Registrar() {
        bm_register_ledger_kernels(reinterpret_cast<const void*>(&bm::ledger_credit_kernel),
                                   reinterpret_cast<const void*>(&bm::ledger_fill_kernel));
    }
};
const Registrar registrar;
}  // namespace
