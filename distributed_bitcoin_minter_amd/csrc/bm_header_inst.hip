// bm_header_inst.hip -- header_hash_kernel (bm_header_hash_gpu) and its build
// unit, registered with the launcher (bm_search.cpp) at load time, the way
// bm_inst.hip registers the search kernels.  The independent check of the
// device's sha256d: it shares nothing with the search kernels' shortcuts
// (bm_header_kernels.hpp, bm_header_versions_body.inc), only sha_compress.
#include "bm_header.hpp"
#include "bm_kernels.hpp"

namespace bm {

// One lane per nonce: the full double hash by the plain compression, from
// the midstate; out gets the 8 digest words of each nonce (big-endian words,
// digest byte order).
constexpr int kHeaderHashThreads = 64;

__global__ __launch_bounds__(kHeaderHashThreads) void header_hash_kernel(const HeaderHashArgs A,
                                                                   const uint32_t* __restrict__ nonces,
                                                                   uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kHeaderHashThreads + threadIdx.x;
    if (i >= A.n) return;
    uint32_t st[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = A.mid[k];
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = 0;
    w[0] = A.w[0];
    w[1] = A.w[1];
    w[2] = A.w[2];
    w[3] = __builtin_bswap32(nonces[i]);
    w[4] = 0x80000000u;
    w[15] = 640u;
    sha_compress(st, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = st[k];
    w[8] = 0x80000000u;
#pragma unroll
    for (int k = 9; k < 15; ++k) w[k] = 0;
    w[15] = 256u;
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = kIV256[k];
    sha_compress(st, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) out[8ull * i + k] = st[k];
}

}  // namespace bm

extern "C" void bm_register_header_hash_kernel(const void* fn);

namespace {
struct Registrar {
    Registrar() { bm_register_header_hash_kernel(reinterpret_cast<const void*>(&bm::header_hash_kernel)); }
};
const Registrar registrar;
}  // namespace
