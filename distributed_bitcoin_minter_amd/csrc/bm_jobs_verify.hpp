// bm_jobs_verify.hpp -- jobs_verify_kernel, the kernel of bm_jobs_verify_gpu: one
// lane per mining.submit tuple of a batch that mixes several Stratum jobs, the
// submissions coming from many sessions.  pool_verify_kernel's algorithm
// (bm_pool_verify.hpp) with the job per workgroup where that kernel has it per
// launch.
//
// pool_verify_kernel rests on every loop being wave-uniform (the tail's block
// count, the words the field touches, the branch depth), and lanes of different
// jobs would break that.  So the host (bm_job.hpp: jobs_plan, jobs_stage) groups
// the batch by job while it stages it, and cuts every group into workgroups of at
// most 64 records, listed in a block table: (job or kJobsNone, first staged record,
// count).  No workgroup spans two jobs.  A staged record is the caller's 32-byte
// submission with its original index where the caller's has `job`.
//
//   1. the workgroup's block-table entry and its job's descriptor (JobsVerifyDesc:
//      PoolVerifyArgs' per-job fields, the window, the offsets of the job's tail and
//      branch in the words array): their addresses depend on blockIdx only, so they
//      are scalar loads and nb, j0, boff, size1, size2 and depth are wave-uniform;
//   2. lanes past `count` return; a kJobsNone workgroup stores INVALID verdicts and
//      hashes nothing;
//   3. the lane's staged record, then its session, as in pool_verify_kernel;
//   4. that kernel's steps 2 to 5 with the descriptor's fields;
//   5. ten ordinary vector stores at out + 10 * original index: the verdicts are in
//      the caller's order, whatever the grouping.
// No LDS, no atomics, no cross-lane operation.
#pragma once
#include "bm_job.hpp"
#include "bm_verify_kernels.hpp"

namespace bm {

__global__ __launch_bounds__(kJobsVerifyThreads) void jobs_verify_kernel(const JobsVerifyDesc* __restrict__ desc,
                                                                          const uint32_t* __restrict__ words,
                                                                          const uint32_t* __restrict__ sessions,
                                                                          const uint32_t nsessions,
                                                                          const bm_jobs_submit_t* __restrict__ submits,
                                                                          const JobsVerifyBlock* __restrict__ blocks,
                                                                          uint32_t* __restrict__ out) {
    const JobsVerifyBlock blk = blocks[blockIdx.x];  // wave-uniform
    if (threadIdx.x >= blk.count) return;
    const bm_jobs_submit_t sub = submits[blk.first + threadIdx.x];
    uint32_t* o = out + (size_t)kVerdictWords * sub.job;  // sub.job: the submission's index in the caller's batch
    if (blk.job == kJobsNone) {  // wave-uniform
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = 0xFFFFFFFFu;
        o[8] = BM_SUBMIT_INVALID;
        o[9] = 0;
        return;
    }
    const JobsVerifyDesc& D = desc[blk.job];
    const uint32_t size1 = D.size1, size2 = D.size2, j0 = D.j0, nb = D.nb, depth = D.depth;
    const bool known = sub.session < nsessions;
    const bool valid = known && (size2 >= 8 || (sub.extranonce2 >> (8 * size2)) == 0);
    // the session: extranonce1's eight bytes and the target, most significant word first
    const uint32_t* ses = sessions + (size_t)kSessionWords * (known ? sub.session : 0u);
    const uint64_t en1 = ((uint64_t)__builtin_bswap32(ses[0]) << 32) | __builtin_bswap32(ses[1]);
    uint32_t tgt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) tgt[k] = __builtin_bswap32(ses[2 + k]);
    uint32_t e[kFieldWords];
    field_words(en1, size1, valid ? sub.extranonce2 : 0ull, size2, D.boff, e);

    uint32_t st[8], w[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = D.mid[k];
    const uint32_t* tail = words + D.tail_off;
    for (uint32_t b = 0; b < nb; ++b) {  // wave-uniform
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

    const uint32_t* branch = words + D.branch_off;
    for (uint32_t d = 0; d < depth; ++d) {  // wave-uniform
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
    for (int k = 0; k < 8; ++k) w[1 + k] = D.prev[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) w[9 + k] = st[k];
    set_iv(st);
    sha_compress(st, w);
    w[0] = root7;
    w[1] = __builtin_bswap32(sub.ntime);
    w[2] = __builtin_bswap32(D.nbits);
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
    uint32_t btgt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) btgt[k] = D.btgt[k];
    uint32_t status = le256(hw, tgt) ? BM_SUBMIT_SHARE : 0u;
    if (D.has_block && le256(hw, btgt)) status |= BM_SUBMIT_BLOCK;
    if (sub.ntime < D.ntime_lo || sub.ntime > D.ntime_hi) status |= BM_SUBMIT_NTIME;
    if (!valid) status = BM_SUBMIT_INVALID;

    // hash byte 4k..4k+3 = hw[k] most significant byte first = the little-endian
    // store of digest word 7 - k
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = valid ? st[7 - k] : 0xFFFFFFFFu;
    o[8] = status;
    o[9] = 0;
}

}  // namespace bm
