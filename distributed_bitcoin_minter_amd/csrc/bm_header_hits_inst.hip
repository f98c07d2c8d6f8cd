// bm_header_hits_inst.hip -- header_hits_kernel's build unit (bm_header_kernels.hpp
// in hits mode), registered with the launcher (bm_search.cpp) at load time.  A
// unit of its own, so bm_header_inst.hip's code object holds what it always held.
#define BM_HEADER_HITS_UNIT 1
#include "bm_header_kernels.hpp"

extern "C" void bm_register_header_hits_kernel(const void* fn);

namespace {
struct Registrar {
    Registrar() { bm_register_header_hits_kernel(reinterpret_cast<const void*>(&bm::header_hits_kernel)); }
};
const Registrar registrar;
}  // namespace
