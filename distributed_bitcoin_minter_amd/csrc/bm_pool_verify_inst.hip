// bm_pool_verify_inst.hip -- pool_verify_kernel's build unit (bm_pool_verify.hpp),
// registered with bm_pool_verify_gpu's launcher (bm_aux.hip) at load time, the way
// bm_job_verify_inst.hip registers job_verify_kernel.  A unit of its own, compiled
// plain (no priority pass), so every other device unit holds what it always held.
#include "bm_pool_verify.hpp"

extern "C" void bm_register_pool_verify_kernel(const void* fn);

namespace {
struct Registrar {
    Registrar() { bm_register_pool_verify_kernel(reinterpret_cast<const void*>(&bm::pool_verify_kernel)); }
};
const Registrar registrar;
}  // namespace
