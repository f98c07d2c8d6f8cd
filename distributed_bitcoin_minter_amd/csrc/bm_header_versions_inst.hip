// bm_header_versions_inst.hip -- header_versions_kernel<M>, M = 1, 2, 4: the
// kernel of bm_search_header_versions_gpu, of bm_search_header_gpu at M = 1,
// and its build unit, registered with the launcher (bm_search.cpp) at load
// time.  Built from the pieces of bm_header_kernels.hpp.  The body is
// bm_header_versions_body.inc, shared with header_versions_hits_kernel<M>
// (bm_header_versions_hits_inst.hip).
//
// A launch scans one nonce range for M versions of one header ("slots";
// bm_header_versions.hpp).  Per nonce n, with the task / inner counter split of
// W3 that bm_header_kernels.hpp describes:
//   * rounds 4..63 of block 2 for all M slots in lock-step over ONE schedule
//     window: each word (sched_word<HeaderBlock2, t>, and the four special
//     words 18, 19, 31, 32) is computed once and fed to sha_round<t> of every
//     slot's state.  The schedule costs the same whatever M is;
//   * then, slot by slot, the 61-round second hash and the hot-path compare
//     (bm_header_kernels.hpp), against one bh for all slots;
//   * rare path: the exact compare and the range check.  A pair is the key
//     (n << 32) | version index: a hit does one atomicMin of its key on the
//     device's hit word, and the running minimum carries the key in the
//     partial's nonce field, so lex_less, block_min and reduce_partials order
//     pairs as (top 64 bits, n, index).  Indices stay below 64, so no pair's
//     key is all-ones.
//   * early exit: at each dequeue lane 0 reads the hit word; a wave leaves
//     when its chunk's first nonce is above hit >> 32.  Only nonces strictly
//     above a recorded hit's nonce are ever skipped, so every pair at the
//     smallest hitting nonce is hashed, whatever the timing.  The hit word is
//     shared by all of a call's launches on the device and set once, before
//     the first, so a later group scans only up to the best hit so far.
#include "bm_header_kernels.hpp"
#include "bm_header_versions.hpp"

namespace bm {

// Waves/SIMD asked for per M: the highest request whose per-nonce code holds no
// scratch or memory operation (tools/check_inner.py --header-versions; DESIGN.md
// "Version rolling").
#ifndef BM_WAVES_VERSIONS_1
#define BM_WAVES_VERSIONS_1 8
#endif
#ifndef BM_WAVES_VERSIONS_2
#define BM_WAVES_VERSIONS_2 5
#endif
#ifndef BM_WAVES_VERSIONS_4
#define BM_WAVES_VERSIONS_4 5
#endif
constexpr int versions_waves(int m) {
    return m == 1 ? BM_WAVES_VERSIONS_1 : m == 2 ? BM_WAVES_VERSIONS_2 : BM_WAVES_VERSIONS_4;
}

template <int M>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(versions_waves(M), 8))) void
header_versions_kernel(const HeaderVersionsArgs<M> A, Partial* __restrict__ part,
                       unsigned long long* __restrict__ counter, unsigned long long* __restrict__ hit) {
#define BM_VERSIONS_HITS 0
#include "bm_header_versions_body.inc"
#undef BM_VERSIONS_HITS
}

template __global__ void header_versions_kernel<1>(const HeaderVersionsArgs<1>, Partial*, unsigned long long*,
                                                   unsigned long long*);
template __global__ void header_versions_kernel<2>(const HeaderVersionsArgs<2>, Partial*, unsigned long long*,
                                                   unsigned long long*);
template __global__ void header_versions_kernel<4>(const HeaderVersionsArgs<4>, Partial*, unsigned long long*,
                                                   unsigned long long*);

}  // namespace bm

extern "C" void bm_register_header_versions_kernel(int m, const void* fn);

namespace {
struct Registrar {
    Registrar() {
        bm_register_header_versions_kernel(1, reinterpret_cast<const void*>(&bm::header_versions_kernel<1>));
        bm_register_header_versions_kernel(2, reinterpret_cast<const void*>(&bm::header_versions_kernel<2>));
        bm_register_header_versions_kernel(4, reinterpret_cast<const void*>(&bm::header_versions_kernel<4>));
    }
};
const Registrar registrar;
}  // namespace
