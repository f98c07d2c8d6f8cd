// bm_share_set_inst.hip -- the build unit of the share set's kernels
// (bm_share_set.hpp), registered with bm_share_set_verify's launcher (bm_aux.hip) at
// load time, the way bm_pool_verify_inst.hip registers pool_verify_kernel.  A unit
// of its own, compiled plain (no priority pass), so every other device unit holds
// what it always held.
#include "bm_share_set.hpp"

extern "C" void bm_register_share_set_kernels(const void* insert, const void* resolve, const void* commit,
                                              const void* rollback);

namespace {
struct Registrar {
    Registrar() {
        bm_register_share_set_kernels(reinterpret_cast<const void*>(&bm::share_insert_kernel),
                                      reinterpret_cast<const void*>(&bm::share_resolve_kernel),
                                      reinterpret_cast<const void*>(&bm::share_commit_kernel),
                                      reinterpret_cast<const void*>(&bm::share_rollback_kernel));
    }
};
const Registrar registrar;
}  // namespace
