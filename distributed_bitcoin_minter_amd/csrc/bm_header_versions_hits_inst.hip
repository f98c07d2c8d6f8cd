// bm_header_versions_hits_inst.hip -- header_versions_hits_kernel<M>, M = 1, 2, 4:
// header_versions_kernel<M> in hits mode (bm_header_versions_body.inc with
// BM_VERSIONS_HITS 1), the kernel of bm_search_header_versions_hits_gpu, of
// bm_search_header_hits_gpu at M = 1, and its build unit, registered with the
// launcher (bm_search.cpp) at load time.  A unit of its own, so
// bm_header_versions_inst.hip's code object holds what it always held.
//
// A full scan: every (nonce, version index) pair of the launch's range whose
// hash meets the target takes the next index of the device's hit counter and,
// below hit_cap, writes {top 64 bits, (n << 32) | version index} into the
// device's buffer.  One counter and one buffer serve all of a call's group
// launches on a device, which may overlap on its streams: the atomicAdd is what
// keeps their slots distinct.  hit_buf holds hit_cap entries of 16 bytes,
// 16-byte aligned.
#include "bm_header_kernels.hpp"
#include "bm_header_versions.hpp"

namespace bm {

// Waves/SIMD asked for per M: the highest request whose per-nonce code holds no
// scratch or memory operation (tools/check_inner.py --header-versions-hits;
// DESIGN.md "Version-rolling share enumeration").
#ifndef BM_WAVES_VERSIONS_HITS_1
#define BM_WAVES_VERSIONS_HITS_1 8
#endif
#ifndef BM_WAVES_VERSIONS_HITS_2
#define BM_WAVES_VERSIONS_HITS_2 5
#endif
#ifndef BM_WAVES_VERSIONS_HITS_4
#define BM_WAVES_VERSIONS_HITS_4 5
#endif
constexpr int versions_hits_waves(int m) {
    return m == 1 ? BM_WAVES_VERSIONS_HITS_1 : m == 2 ? BM_WAVES_VERSIONS_HITS_2 : BM_WAVES_VERSIONS_HITS_4;
}

template <int M>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(versions_hits_waves(M), 8))) void
header_versions_hits_kernel(const HeaderVersionsArgs<M> A, Partial* __restrict__ part,
                            unsigned long long* __restrict__ counter, unsigned long long* __restrict__ hit_count,
                            Partial* __restrict__ hit_buf, const uint64_t hit_cap) {
#define BM_VERSIONS_HITS 1
#include "bm_header_versions_body.inc"
#undef BM_VERSIONS_HITS
}

template __global__ void header_versions_hits_kernel<1>(const HeaderVersionsArgs<1>, Partial*, unsigned long long*,
                                                        unsigned long long*, Partial*, const uint64_t);
template __global__ void header_versions_hits_kernel<2>(const HeaderVersionsArgs<2>, Partial*, unsigned long long*,
                                                        unsigned long long*, Partial*, const uint64_t);
template __global__ void header_versions_hits_kernel<4>(const HeaderVersionsArgs<4>, Partial*, unsigned long long*,
                                                        unsigned long long*, Partial*, const uint64_t);

}  // namespace bm

extern "C" void bm_register_header_versions_hits_kernel(int m, const void* fn);

namespace {
struct Registrar {
    Registrar() {
        bm_register_header_versions_hits_kernel(1, reinterpret_cast<const void*>(&bm::header_versions_hits_kernel<1>));
        bm_register_header_versions_hits_kernel(2, reinterpret_cast<const void*>(&bm::header_versions_hits_kernel<2>));
        bm_register_header_versions_hits_kernel(4, reinterpret_cast<const void*>(&bm::header_versions_hits_kernel<4>));
    }
};
const Registrar registrar;
}  // namespace
