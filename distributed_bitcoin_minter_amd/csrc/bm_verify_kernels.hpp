// bm_verify_kernels.hpp -- the device pieces the two share verifiers share
// (job_verify_kernel in bm_job_verify.hpp, pool_verify_kernel in
// bm_pool_verify.hpp): the second hash of a 32-byte digest over sha_compress
// (bm_kernels.hpp).  No kernel in here: each verifier's unit includes this.
#pragma once
#include "bm_header_kernels.hpp"

namespace bm {

// w[0..7] = d, then the padding of a 32-byte message: the second hash's block.
BM_DEV void digest_block(const uint32_t (&d)[8], uint32_t (&w)[16]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = d[k];
    w[8] = 0x80000000u;
#pragma unroll
    for (int k = 9; k < 15; ++k) w[k] = 0;
    w[15] = 256u;
}

BM_DEV void set_iv(uint32_t (&st)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = kIV256[k];
}

// st = SHA256 state of the 32 bytes st held as a digest: the second hash.
BM_DEV void hash_digest(uint32_t (&st)[8], uint32_t (&w)[16]) {
    digest_block(st, w);
    set_iv(st);
    sha_compress(st, w);
}

}  // namespace bm
