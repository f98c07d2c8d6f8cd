// bm_job_verify.hpp -- job_verify_kernel, the kernel of bm_job_verify_gpu: one
// lane per mining.submit tuple of one Stratum job.  Built from sha_compress
// (bm_kernels.hpp) and le256 (bm_header_kernels.hpp); nothing of the header search's
// shortcuts: every lane hashes its own coinbase tail, folds the merkle branch and
// double-hashes its own header, nb + 1 + 3 * depth + 3 plain compressions.
//
// The shape is the same for every lane (bm_job.hpp has the host part): the tail
// template, its block count, the three words extranonce2 can touch (j0 .. j0 + 2)
// and the branch are wave-uniform, so every loop is a wave-uniform loop, the
// template and the branch come through scalar loads, and selecting the three
// words is a compare of a compile-time k plus a uniform block index against j0:
// no per-lane array is indexed by a run-time value.
//
//   1. e0..e2 = the lane's extranonce2 shifted into the three words (en2_words);
//   2. st = mid; for each tail block: w[k] = tail[16 b + k] | (16 b + k == j0 + i
//      ? e_i : 0); compress;
//   3. root = SHA256(st) (one block from the IV);
//   4. per branch entry: compress(IV, root || entry), the constant padding block
//      of a 64-byte message, the 32-byte second hash;
//   5. header block 1 = bswap(version), prevhash, root words 0..6; block 2 = root
//      word 7, bswap(ntime), bswap(nbits), bswap(nonce), padding;
//   6. two compressions and the second hash;
//   7. both 256-bit compares;
//   8. ten ordinary vector stores: the hash, most significant byte first, the
//      status and a zero (bm_job_verdict_t's layout).
// A lane whose extranonce2 does not fit its field runs along (its words are
// masked to nothing) and stores the INVALID verdict instead.
#pragma once
#include "bm_job.hpp"
#include "bm_verify_kernels.hpp"  // digest_block, set_iv, hash_digest: pool_verify_kernel's too

namespace bm {

constexpr int kJobVerifyThreads = 64;

__global__ __launch_bounds__(kJobVerifyThreads) void job_verify_kernel(const JobVerifyArgs A,
                                                                        const uint32_t* __restrict__ tail,
                                                                        const uint32_t* __restrict__ branch,
                                                                        const bm_job_submit_t* __restrict__ submits,
                                                                        uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kJobVerifyThreads + threadIdx.x;
    if (i >= A.n) return;
    const bm_job_submit_t sub = submits[i];
    const bool fits = A.size >= 8 || (sub.extranonce2 >> (8 * A.size)) == 0;
    uint32_t e0, e1, e2;
    en2_words(fits ? sub.extranonce2 : 0ull, A.size, A.boff, e0, e1, e2);

    uint32_t st[8], w[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = A.mid[k];
    const uint32_t j0 = A.j0;
    for (uint32_t b = 0; b < A.nb; ++b) {  // wave-uniform
        const uint32_t* t = tail + 16ull * b;
        const uint32_t base = 16u * b;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t idx = base + (uint32_t)k;
            uint32_t x = t[k];
            x |= idx == j0 ? e0 : 0u;
            x |= idx == j0 + 1u ? e1 : 0u;
            x |= idx == j0 + 2u ? e2 : 0u;
            w[k] = x;
        }
        sha_compress(st, w);
    }
    hash_digest(st, w);  // the root, as the digest's big-endian words

    for (uint32_t d = 0; d < A.depth; ++d) {  // wave-uniform
        const uint32_t* e = branch + 8ull * d;
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = st[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[8 + k] = e[k];
        set_iv(st);
        sha_compress(st, w);
        w[0] = 0x80000000u;  // the padding block of a 64-byte message
#pragma unroll
        for (int k = 1; k < 15; ++k) w[k] = 0;
        w[15] = 512u;
        sha_compress(st, w);
        hash_digest(st, w);
    }

    // the header: block 1, block 2, the second hash
    const uint32_t root7 = st[7];
    w[0] = __builtin_bswap32(sub.version);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[1 + k] = A.prev[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) w[9 + k] = st[k];
    set_iv(st);
    sha_compress(st, w);
    w[0] = root7;
    w[1] = __builtin_bswap32(sub.ntime);
    w[2] = __builtin_bswap32(A.nbits);
    w[3] = __builtin_bswap32(sub.nonce);
    w[4] = 0x80000000u;
#pragma unroll
    for (int k = 5; k < 15; ++k) w[k] = 0;
    w[15] = 640u;
    sha_compress(st, w);
    hash_digest(st, w);

    uint32_t hw[8];  // the hash, most significant word first
#pragma unroll
    for (int k = 0; k < 8; ++k) hw[k] = __builtin_bswap32(st[7 - k]);
    uint32_t status = le256(hw, A.tgt) ? BM_SUBMIT_SHARE : 0u;
    if (A.has_block && le256(hw, A.btgt)) status |= BM_SUBMIT_BLOCK;
    if (!fits) status = BM_SUBMIT_INVALID;

    // hash byte 4k..4k+3 = hw[k] most significant byte first = the little-endian
    // store of digest word 7 - k
    uint32_t* o = out + (size_t)kVerdictWords * i;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = fits ? st[7 - k] : 0xFFFFFFFFu;
    o[8] = status;
    o[9] = 0;
}

}  // namespace bm
