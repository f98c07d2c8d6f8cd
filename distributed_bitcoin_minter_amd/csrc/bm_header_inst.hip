// bm_header_inst.hip -- the block-header kernels' build unit: header_kernel
// and header_hash_kernel (bm_header_kernels.hpp), registered with the launcher
// (bm_search.cpp) at load time, the way bm_inst.hip registers the search kernels.
#include "bm_header_kernels.hpp"

extern "C" void bm_register_header_kernels(const void* search_fn, const void* hash_fn);

namespace {
struct Registrar {
    Registrar() {
        bm_register_header_kernels(reinterpret_cast<const void*>(&bm::header_kernel),
                                   reinterpret_cast<const void*>(&bm::header_hash_kernel));
    }
};
const Registrar registrar;
}  // namespace
