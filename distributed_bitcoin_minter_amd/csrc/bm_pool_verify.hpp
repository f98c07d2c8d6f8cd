// bm_pool_verify.hpp -- pool_verify_kernel, the kernel of bm_pool_verify_gpu: one
// lane per mining.submit tuple of one Stratum job, the submissions coming from
// many sessions.  job_verify_kernel's algorithm (bm_job_verify.hpp) with two
// per-lane inputs where that kernel has uniform ones: extranonce1 and the share
// target come from the lane's entry of a session table.
//
// The shape is still the same for every lane (bm_job.hpp has the host part): the
// tail template (both extranonce fields zero), its block count, the five words
// the field extranonce1 || extranonce2 can touch (j0 .. j0 + 4) and the branch are
// wave-uniform, so every loop is a wave-uniform loop, the template and the branch
// come through scalar loads, and selecting the five words is a compare of a
// compile-time k plus a uniform block index against j0: no per-lane array is
// indexed by a run-time value.
//
//   1. the lane's submission, then its session: ten words at a 40-byte stride (a
//      divergent vector load); an index past the table is replaced by 0, so an
//      INVALID lane reads inside the table (the host stages at least one entry);
//   2. e0..e4 = the lane's field shifted into the five words (field_words);
//   3. st = mid; for each tail block: w[k] = tail[16 b + k] | (16 b + k == j0 + i
//      ? e_i : 0); compress;
//   4. the root, the branch fold, the header's two blocks and the second hash, as
//      in job_verify_kernel;
//   5. the 256-bit compare against the lane's own target words (VGPRs) and against
//      the uniform block target, then the ntime window;
//   6. ten ordinary vector stores: the hash, most significant byte first, the
//      status and a zero (bm_job_verdict_t's layout).
// A lane whose extranonce2 does not fit its field, or whose session index is past
// the table, runs along (its extranonce2 is masked to nothing) and stores the
// INVALID verdict instead.  No LDS, no atomics, no cross-lane operation.
#pragma once
#include "bm_job.hpp"
#include "bm_verify_kernels.hpp"

namespace bm {

constexpr int kPoolVerifyThreads = 64;

__global__ __launch_bounds__(kPoolVerifyThreads) void pool_verify_kernel(const PoolVerifyArgs A,
                                                                          const uint32_t* __restrict__ tail,
                                                                          const uint32_t* __restrict__ branch,
                                                                          const uint32_t* __restrict__ sessions,
                                                                          const bm_pool_submit_t* __restrict__ submits,
                                                                          uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kPoolVerifyThreads + threadIdx.x;
    if (i >= A.n) return;
    const bm_pool_submit_t sub = submits[i];
    const bool known = sub.session < A.nsessions;
    const bool valid = known && (A.size2 >= 8 || (sub.extranonce2 >> (8 * A.size2)) == 0);
    // the session: extranonce1's eight bytes and the target, most significant word first
    const uint32_t* ses = sessions + (size_t)kSessionWords * (known ? sub.session : 0u);
    const uint64_t en1 = ((uint64_t)__builtin_bswap32(ses[0]) << 32) | __builtin_bswap32(ses[1]);
    uint32_t tgt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) tgt[k] = __builtin_bswap32(ses[2 + k]);
    uint32_t e[kFieldWords];
    field_words(en1, A.size1, valid ? sub.extranonce2 : 0ull, A.size2, A.boff, e);

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
#pragma unroll
            for (int f = 0; f < kFieldWords; ++f) x |= idx == j0 + (uint32_t)f ? e[f] : 0u;
            w[k] = x;
        }
        sha_compress(st, w);
    }
    hash_digest(st, w);  // the root, as the digest's big-endian words

    for (uint32_t d = 0; d < A.depth; ++d) {  // wave-uniform
        const uint32_t* en = branch + 8ull * d;
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = st[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[8 + k] = en[k];
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
    uint32_t status = le256(hw, tgt) ? BM_SUBMIT_SHARE : 0u;
    if (A.has_block && le256(hw, A.btgt)) status |= BM_SUBMIT_BLOCK;
    if (sub.ntime < A.ntime_lo || sub.ntime > A.ntime_hi) status |= BM_SUBMIT_NTIME;
    if (!valid) status = BM_SUBMIT_INVALID;

    // hash byte 4k..4k+3 = hw[k] most significant byte first = the little-endian
    // store of digest word 7 - k
    uint32_t* o = out + (size_t)kVerdictWords * i;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = valid ? st[7 - k] : 0xFFFFFFFFu;
    o[8] = status;
    o[9] = 0;
}

}  // namespace bm
