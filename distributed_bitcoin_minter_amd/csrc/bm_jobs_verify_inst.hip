// bm_jobs_verify_inst.hip -- jobs_verify_kernel's build unit (bm_jobs_verify.hpp),
// registered with bm_jobs_verify_gpu's launcher (bm_aux.hip) at load time, the way
// bm_pool_verify_inst.hip registers pool_verify_kernel.  A unit of its own, compiled
// plain (no priority pass), so every other device unit holds what it always held.
#include "bm_jobs_verify.hpp"

extern "C" void bm_register_jobs_verify_kernel(const void* fn);

namespace {
struct Registrar {
    Registrar() { bm_register_jobs_verify_kernel(reinterpret_cast<const void*>(&bm::jobs_verify_kernel)); }
};
const Registrar registrar;
}  // namespace
