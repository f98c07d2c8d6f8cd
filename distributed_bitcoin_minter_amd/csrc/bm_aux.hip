// bm_aux.hip -- the one unit of the host runtime with device code: the small
// kernels of bm_aux_kernels.hpp, the host wrapper the searches launch the
// second-pass reduction through, and the entry points outside the search
// path (bm_reduce_gpu, bm_hash_gpu, bm_header_hash_gpu, and bm_job_verify_gpu,
// bm_pool_verify_gpu, bm_jobs_verify_gpu and the device side of bm_share_set_verify,
// bm_share_set_verify_jobs, bm_ledger_verify_jobs and the session table, whose kernels
// have units of their own, bm_job_verify_inst.hip, bm_pool_verify_inst.hip,
// bm_jobs_verify_inst.hip, bm_share_set_inst.hip, bm_ledger_inst.hip and
// bm_sessions_inst.hip).  See
// bm_runtime.hpp for the layout of the host runtime.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bm_aux_kernels.hpp"
#include "bm_job.hpp"
#include "bm_ledger_host.hpp"
#include "bm_runtime.hpp"
#include "bm_sessions_host.hpp"
#include "bm_share_set_host.hpp"

namespace bm {

static_assert(kCtrClockSlot == kClockSlot, "the host reads the clock stamps where the kernels write them");

int launch_reduce_partials(const Partial* part, uint32_t n, Partial* out, hipStream_t s) {
    reduce_partials<<<1, kReduceThreads, 0, s>>>(part, n, out);
    return hip_status(hipGetLastError());
}

namespace {

// bm_reduce_gpu: n partials, one per lane, through block_min (ds_swizzle
// butterflies, readlane, LDS) and then reduce_partials -- the reductions the
// search uses above its per-lane scans.
int reduce_impl(bm_ctx* ctx, const bm_result_t* in, size_t n, bm_result_t* out) {
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    const size_t blocks = (n + kBlock - 1) / kBlock;
    BM_TRY(grow(d, d.d_test, d.test_cap, n + blocks + 1));
    Partial* d_in = d.d_test;
    Partial* d_blk = d.d_test + n;
    Partial* d_out = d_blk + blocks;
    if (n) BM_HIP(hipMemcpyAsync(d_in, in, n * sizeof(Partial), hipMemcpyHostToDevice, d.stream));
    if (blocks) {
        lane_partials_min<<<dim3((uint32_t)blocks), kBlock, 0, d.stream>>>(d_in, (uint32_t)n, d_blk);
        BM_HIP(hipGetLastError());
    }
    BM_TRY(launch_reduce_partials(d_blk, (uint32_t)blocks, d_out, d.stream));
    Partial r;
    BM_HIP(hipMemcpyAsync(&r, d_out, sizeof r, hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    out->hash = r.hash;
    out->nonce = r.nonce;
    return BM_OK;
}

int hash_impl(bm_ctx* ctx, const uint8_t* msg, size_t len, const uint64_t* nonces, size_t n, uint64_t* out) {
    if (n == 0) return BM_OK;
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    HashArgs A;
    std::memset(&A, 0, sizeof A);
    // midstate over the whole 64-byte blocks of "msg "
    const uint64_t pre = (uint64_t)len + 1;
    const uint64_t full = pre / 64;
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    uint8_t blk[64];
    for (uint64_t b = 0; b < full; ++b) {
        for (int i = 0; i < 64; ++i) {
            const uint64_t pos = b * 64 + (uint64_t)i;
            blk[i] = pos < len ? msg[pos] : (uint8_t)' ';
        }
        host::compress_bytes(st, blk);
    }
    std::memcpy(A.mid, st, sizeof st);
    A.tail_len = (uint32_t)(pre - full * 64);
    for (uint32_t i = 0; i < A.tail_len; ++i) {
        const uint64_t pos = full * 64 + i;
        A.tail[i] = pos < len ? msg[pos] : (uint8_t)' ';
    }
    A.total_prefix = pre;
    A.n = n;
    BM_TRY(grow(d, d.d_hash_io, d.hash_cap, n, 2 * sizeof(uint64_t)));
    BM_HIP(hipMemcpyAsync(d.d_hash_io, nonces, n * sizeof(uint64_t), hipMemcpyHostToDevice, d.stream));
    const uint64_t grid = (n + kHashThreads - 1) / kHashThreads;
    hash_kernel<<<dim3((uint32_t)grid), kHashThreads, 0, d.stream>>>(A, d.d_hash_io, d.d_hash_io + n);
    BM_HIP(hipGetLastError());
    BM_HIP(hipMemcpyAsync(out, d.d_hash_io + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    return BM_OK;
}

// bm_header_hash_gpu: the full double hash of arbitrary nonces on the first
// device, most significant byte first.
int header_hash_impl(bm_ctx* ctx, const uint8_t* header, const uint32_t* nonces, size_t n, uint8_t* out) {
    if (n == 0) return BM_OK;
    if (!g_header_hash) return BM_EINTERNAL;
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    HeaderHashArgs A;
    std::memset(&A, 0, sizeof A);
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    host::compress_bytes(st, header);
    std::memcpy(A.mid, st, sizeof st);
    for (int i = 0; i < 3; ++i) A.w[i] = host::load_be32(header + 64 + 4 * i);
    A.n = (uint32_t)n;
    BM_TRY(grow(d, d.d_hdr_io, d.hdr_cap, n, 9 * sizeof(uint32_t)));
    std::vector<uint32_t> words(8 * n);
    uint32_t* d_in = d.d_hdr_io;
    uint32_t* d_out = d.d_hdr_io + n;
    BM_HIP(hipMemcpyAsync(d_in, nonces, n * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    const uint32_t grid = (uint32_t)((n + 63) / 64);
    void* args[] = {&A, &d_in, &d_out};
    BM_HIP(hipLaunchKernel(g_header_hash, dim3(grid), dim3(64), args, 0, d.stream));
    BM_HIP(hipMemcpyAsync(words.data(), d_out, 8 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    // digest word k (big-endian) holds digest bytes 4k..4k+3; the hash is the
    // digest reversed
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 8; ++k) {
            const uint32_t w = words[8 * i + k];
            uint8_t* o = out + 32 * i + 4 * (7 - k);
            o[0] = (uint8_t)w;
            o[1] = (uint8_t)(w >> 8);
            o[2] = (uint8_t)(w >> 16);
            o[3] = (uint8_t)(w >> 24);
        }
    return BM_OK;
}

// job_verify_kernel, registered by bm_job_verify_inst.hip at load time
const void* g_job_verify = nullptr;

// bm_job_verify_gpu on the first device: the job's tail template, its branch and
// the submissions go up in one copy, one launch gives a lane to each submission,
// the verdicts come back in one copy.  The caller's arrays are written last.
int job_verify_impl(bm_ctx* ctx, const bm_job_t* job, const uint8_t* target, const bm_job_submit_t* submits, size_t n,
                    bm_job_verdict_t* verdicts, bm_job_verify_result_t* out) {
    if (!g_job_verify) return BM_EINTERNAL;
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    JobVerifyArgs A;
    std::vector<uint32_t> tail, branch;
    host::verify_prepare(job, target, A, tail, branch);
    A.n = (uint32_t)n;
    // device buffer, in 8-byte units: tail | branch | submits | verdicts
    const size_t tail_u = tail.size() / 2, branch_u = branch.size() / 2;
    const size_t sub_u = n * sizeof(bm_job_submit_t) / 8, in_u = tail_u + branch_u + sub_u;
    const size_t out_u = n * sizeof(bm_job_verdict_t) / 8;
    // and a pinned host copy of the same layout: the staging of the one copy up and the target of the one
    // copy back (kept with the context: a batch is tens of megabytes, and fresh pageable memory per call
    // costs more than the kernel)
    BM_TRY(grow(d, d.h_verify, d.hverify_cap, in_u + out_u, sizeof(uint64_t), true));
    BM_TRY(grow(d, d.d_verify, d.verify_cap, in_u + out_u));
    uint64_t* stage = d.h_verify;
    const bm_job_verdict_t* got = reinterpret_cast<const bm_job_verdict_t*>(d.h_verify + in_u);
    std::memcpy(stage, tail.data(), 8 * tail_u);
    if (branch_u) std::memcpy(stage + tail_u, branch.data(), 8 * branch_u);
    std::memcpy(stage + tail_u + branch_u, submits, 8 * sub_u);
    BM_HIP(hipMemcpyAsync(d.d_verify, stage, 8 * in_u, hipMemcpyHostToDevice, d.stream));
    const uint32_t* d_tail = reinterpret_cast<const uint32_t*>(d.d_verify);
    const uint32_t* d_branch = reinterpret_cast<const uint32_t*>(d.d_verify + tail_u);
    const bm_job_submit_t* d_sub = reinterpret_cast<const bm_job_submit_t*>(d.d_verify + tail_u + branch_u);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(d.d_verify + in_u);
    const uint32_t grid = (uint32_t)((n + 63) / 64);
    void* args[] = {&A, &d_tail, &d_branch, &d_sub, &d_out};
    BM_HIP(hipLaunchKernel(g_job_verify, dim3(grid), dim3(64), args, 0, d.stream));
    BM_HIP(hipMemcpyAsync(d.h_verify + in_u, d_out, 8 * out_u, hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    // the tripwire: the ends of the batch and every claimed block, by the CPU path
    uint8_t bt[32];
    const uint8_t* block_target = host::target_from_bits(job->nbits, bt) ? bt : nullptr;
    for (size_t i = 0; i < n; ++i) {
        if (i != 0 && i != n - 1 && !(got[i].status & BM_SUBMIT_BLOCK)) continue;
        bm_job_verdict_t want;
        host::verify_one(job, target, block_target, submits[i], want);
        if (std::memcmp(&want, &got[i], sizeof want) != 0) return BM_EINTERNAL;
    }
    bm_job_verify_result_t r;
    host::verify_count(got, n, r);
    std::memcpy(verdicts, got, n * sizeof(bm_job_verdict_t));
    *out = r;
    return BM_OK;
}

// pool_verify_kernel, registered by bm_pool_verify_inst.hip at load time
const void* g_pool_verify = nullptr;

// What bm_pool_verify_gpu and bm_share_set_verify share: the stage, the launch of
// pool_verify_kernel, and the tripwire.  The job's tail template, its branch, the
// session table and the submissions go up in one copy, one launch gives a lane to
// each submission.  The buffers are job_verify_impl's (a context runs one call at a
// time).  Device buffer, in 8-byte units:
//   tail | branch | sessions | submits | ctl | verdicts | lanes
// ctl (ctl_u units, zeros, the end of the copy up) and lanes (lane_u units, never
// copied) are the share set's; bm_pool_verify_gpu asks for none of either.  The
// pinned host copy has the same layout up to the verdicts' end.
struct PoolStage {
    size_t in_u = 0, out_u = 0;       // units before the verdicts (ctl included), units of the verdicts
    uint32_t* d_out = nullptr;        // the verdicts on the device
    uint64_t* d_lanes = nullptr;      // lane_u units after them
    const bm_job_verdict_t* got = nullptr;  // the verdicts' place in the pinned copy
    // jobs_verify_launch only: the staged records on the device, and where a ledger's extras start (below)
    const bm_jobs_submit_t* d_sub = nullptr;
    size_t extra_at = 0;
    // with a LedgerStage: accounts[] and weights[] on the device, and where the credit's control words are
    const uint32_t* d_acc = nullptr;
    const uint64_t* d_wgt = nullptr;
    size_t ctl_at = 0;
};

// What a ledger adds to jobs_verify_launch's copy up, between the block table and
// ctl: accounts[] (32-bit, padded to a unit), weights[] and the credit kernel's
// control words, zero.  NULL accounts are staged as the identity, NULL weights as ones.
// A session table (bm_sessions_t) has the three per-session arrays on the device
// already: with d_sessions set they are neither staged nor copied, the kernels get
// these pointers, and the extras are the control words alone.
struct LedgerStage {
    const uint32_t* accounts;
    const uint64_t* weights;
    const uint32_t* d_sessions = nullptr;
    const uint32_t* d_accounts = nullptr;
    const uint64_t* d_weights = nullptr;
    static size_t acc_units(size_t ses_staged) { return (ses_staged + 1) / 2; }
    static size_t units(size_t ses_staged) { return acc_units(ses_staged) + ses_staged + kLedgerCtlUnits; }
};

int pool_verify_launch(DeviceCtx& d, const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                       const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi, size_t ctl_u,
                       size_t lane_u, PoolStage& st) {
    if (!g_pool_verify) return BM_EINTERNAL;
    PoolVerifyArgs A;
    std::vector<uint32_t> tail, branch;
    host::pool_verify_prepare(job, A, tail, branch);
    A.n = (uint32_t)n;
    A.nsessions = (uint32_t)nsessions;
    A.ntime_lo = ntime_lo;
    A.ntime_hi = ntime_hi;
    // An empty table is staged as one zero session: a lane whose index is out of range reads entry 0 and
    // stores INVALID
    const size_t staged = nsessions ? nsessions : 1;
    const size_t tail_u = tail.size() / 2, branch_u = branch.size() / 2;
    const size_t ses_u = staged * sizeof(bm_pool_session_t) / 8, sub_u = n * sizeof(bm_pool_submit_t) / 8;
    const size_t in_u = tail_u + branch_u + ses_u + sub_u + ctl_u;
    const size_t out_u = n * sizeof(bm_job_verdict_t) / 8;
    BM_TRY(grow(d, d.h_verify, d.hverify_cap, in_u + out_u, sizeof(uint64_t), true));
    BM_TRY(grow(d, d.d_verify, d.verify_cap, in_u + out_u + lane_u));
    uint64_t* stage = d.h_verify;
    std::memcpy(stage, tail.data(), 8 * tail_u);
    if (branch_u) std::memcpy(stage + tail_u, branch.data(), 8 * branch_u);
    if (nsessions)
        std::memcpy(stage + tail_u + branch_u, sessions, 8 * ses_u);
    else
        std::memset(stage + tail_u + branch_u, 0, 8 * ses_u);
    std::memcpy(stage + tail_u + branch_u + ses_u, submits, 8 * sub_u);
    if (ctl_u) std::memset(stage + in_u - ctl_u, 0, 8 * ctl_u);
    BM_HIP(hipMemcpyAsync(d.d_verify, stage, 8 * in_u, hipMemcpyHostToDevice, d.stream));
    const uint32_t* d_tail = reinterpret_cast<const uint32_t*>(d.d_verify);
    const uint32_t* d_branch = reinterpret_cast<const uint32_t*>(d.d_verify + tail_u);
    const uint32_t* d_ses = reinterpret_cast<const uint32_t*>(d.d_verify + tail_u + branch_u);
    const bm_pool_submit_t* d_sub = reinterpret_cast<const bm_pool_submit_t*>(d.d_verify + tail_u + branch_u + ses_u);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(d.d_verify + in_u);
    const uint32_t grid = (uint32_t)((n + 63) / 64);
    void* args[] = {&A, &d_tail, &d_branch, &d_ses, &d_sub, &d_out};
    BM_HIP(hipLaunchKernel(g_pool_verify, dim3(grid), dim3(64), args, 0, d.stream));
    st.in_u = in_u;
    st.out_u = out_u;
    st.d_out = d_out;
    st.d_lanes = d.d_verify + in_u + out_u;
    st.got = reinterpret_cast<const bm_job_verdict_t*>(d.h_verify + in_u);
    return BM_OK;
}

// The tripwire: the ends of the batch and every claimed block, by the CPU path.  The
// status bits of `ignore` are not the verifier's and do not count.
int pool_verify_tripwire(const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                         const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                         const bm_job_verdict_t* got, uint32_t ignore) {
    uint8_t bt[32];
    const uint8_t* block_target = host::target_from_bits(job->nbits, bt) ? bt : nullptr;
    for (size_t i = 0; i < n; ++i) {
        if (i != 0 && i != n - 1 && !(got[i].status & BM_SUBMIT_BLOCK)) continue;
        bm_job_verdict_t want, have = got[i];
        have.status &= ~ignore;
        host::pool_verify_one(job, sessions, nsessions, block_target, ntime_lo, ntime_hi, submits[i], want);
        if (std::memcmp(&want, &have, sizeof want) != 0) return BM_EINTERNAL;
    }
    return BM_OK;
}

// bm_pool_verify_gpu on the first device, the shape of job_verify_impl: one copy up,
// one launch, the verdicts back in one copy.  The caller's arrays are written last.
int pool_verify_impl(bm_ctx* ctx, const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                     const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                     bm_job_verdict_t* verdicts, bm_pool_verify_result_t* out) {
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    PoolStage st;
    BM_TRY(pool_verify_launch(d, job, sessions, nsessions, submits, n, ntime_lo, ntime_hi, 0, 0, st));
    BM_HIP(hipMemcpyAsync(d.h_verify + st.in_u, st.d_out, 8 * st.out_u, hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    BM_TRY(pool_verify_tripwire(job, sessions, nsessions, submits, n, ntime_lo, ntime_hi, st.got, 0));
    bm_pool_verify_result_t r;
    host::pool_verify_count(st.got, n, r);
    std::memcpy(verdicts, st.got, n * sizeof(bm_job_verdict_t));
    *out = r;
    return BM_OK;
}

// jobs_verify_kernel, registered by bm_jobs_verify_inst.hip at load time
const void* g_jobs_verify = nullptr;

// What bm_jobs_verify_gpu and bm_share_set_verify_jobs share: the grouping, the stage
// and the launch of jobs_verify_kernel.  The buffers are job_verify_impl's.  Device
// buffer, in 8-byte units:
//   descriptors | words (all tails, all branches) | sessions | staged submits | block table | extras | ctl | verdicts | lanes
// with ctl and lanes as in pool_verify_launch, extras a ledger's (LedgerStage; none without one), and the verdicts and what follows them
// where PoolStage says, so the share set's kernels take them unchanged.  The counting
// sort's scatter is the copy of the submissions into the pinned buffer; plan and
// *staged (the pinned copy of the staged records) stay valid for the tripwire.
int jobs_verify_launch(DeviceCtx& d, const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions,
                       size_t nsessions, const bm_jobs_submit_t* submits, size_t n, size_t ctl_u, size_t lane_u,
                       PoolStage& st, host::JobsPlan& plan, const bm_jobs_submit_t** staged,
                       const LedgerStage* lg = nullptr) {
    if (!g_jobs_verify) return BM_EINTERNAL;
    std::vector<JobsVerifyDesc> desc;
    std::vector<uint32_t> words;
    host::jobs_verify_prepare(jobs, njobs, desc, words);
    host::jobs_plan(submits, n, njobs, plan);
    // An empty job table is staged as one zero descriptor and an empty session table as one zero session, so
    // every array on the device has an entry; no lane reads either
    const size_t ses_staged = nsessions ? nsessions : 1, desc_staged = njobs ? njobs : 1;
    const size_t desc_u = desc_staged * sizeof(JobsVerifyDesc) / 8, words_u = words.size() / 2;
    const bool resident = lg && lg->d_sessions;  // a session table's arrays: nothing per session is staged
    const size_t ses_u = resident ? 0 : ses_staged * sizeof(bm_pool_session_t) / 8, sub_u = n * sizeof(bm_jobs_submit_t) / 8;
    const size_t blk_u = plan.blocks.size() * sizeof(JobsVerifyBlock) / 8;
    const size_t extra_u = !lg ? 0 : resident ? (size_t)kLedgerCtlUnits : LedgerStage::units(ses_staged);
    const size_t in_u = desc_u + words_u + ses_u + sub_u + blk_u + extra_u + ctl_u;
    const size_t out_u = n * sizeof(bm_job_verdict_t) / 8;
    BM_TRY(grow(d, d.h_verify, d.hverify_cap, in_u + out_u, sizeof(uint64_t), true));
    BM_TRY(grow(d, d.d_verify, d.verify_cap, in_u + out_u + lane_u));
    uint64_t* stage = d.h_verify;
    size_t at = 0;
    const size_t desc_at = at;
    if (njobs)
        std::memcpy(stage + at, desc.data(), 8 * desc_u);
    else
        std::memset(stage + at, 0, 8 * desc_u);
    at += desc_u;
    const size_t words_at = at;
    if (words_u) std::memcpy(stage + at, words.data(), 8 * words_u);
    at += words_u;
    const size_t ses_at = at;
    if (nsessions && !resident)
        std::memcpy(stage + at, sessions, 8 * ses_u);
    else
        std::memset(stage + at, 0, 8 * ses_u);
    at += ses_u;
    const size_t sub_at = at;
    bm_jobs_submit_t* h_staged = reinterpret_cast<bm_jobs_submit_t*>(stage + at);
    host::jobs_stage(submits, n, njobs, plan, h_staged);
    at += sub_u;
    const size_t blk_at = at;
    std::memcpy(stage + at, plan.blocks.data(), 8 * blk_u);
    at += blk_u;
    const size_t extra_at = at;
    if (lg) {
        std::memset(stage + at, 0, 8 * extra_u);
        if (!resident) {
            uint32_t* acc = reinterpret_cast<uint32_t*>(stage + at);
            uint64_t* wgt = stage + at + LedgerStage::acc_units(ses_staged);
            for (size_t s = 0; s < nsessions; ++s) acc[s] = lg->accounts ? lg->accounts[s] : (uint32_t)s;
            for (size_t s = 0; s < nsessions; ++s) wgt[s] = lg->weights ? lg->weights[s] : 1ull;
        }
        at += extra_u;
    }
    if (ctl_u) std::memset(stage + at, 0, 8 * ctl_u);
    BM_HIP(hipMemcpyAsync(d.d_verify, stage, 8 * in_u, hipMemcpyHostToDevice, d.stream));
    const JobsVerifyDesc* d_desc = reinterpret_cast<const JobsVerifyDesc*>(d.d_verify + desc_at);
    const uint32_t* d_words = reinterpret_cast<const uint32_t*>(d.d_verify + words_at);
    const uint32_t* d_ses = resident ? lg->d_sessions : reinterpret_cast<const uint32_t*>(d.d_verify + ses_at);
    uint32_t nses = (uint32_t)nsessions;
    const bm_jobs_submit_t* d_sub = reinterpret_cast<const bm_jobs_submit_t*>(d.d_verify + sub_at);
    const JobsVerifyBlock* d_blk = reinterpret_cast<const JobsVerifyBlock*>(d.d_verify + blk_at);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(d.d_verify + in_u);
    void* args[] = {&d_desc, &d_words, &d_ses, &nses, &d_sub, &d_blk, &d_out};
    BM_HIP(hipLaunchKernel(g_jobs_verify, dim3((uint32_t)plan.blocks.size()), dim3(kJobsVerifyThreads), args, 0,
                           d.stream));
    st.in_u = in_u;
    st.out_u = out_u;
    st.d_out = d_out;
    st.d_lanes = d.d_verify + in_u + out_u;
    st.got = reinterpret_cast<const bm_job_verdict_t*>(d.h_verify + in_u);
    st.d_sub = d_sub;
    st.extra_at = extra_at;
    if (resident) {
        st.d_acc = lg->d_accounts;
        st.d_wgt = lg->d_weights;
        st.ctl_at = extra_at;
    } else if (lg) {
        st.d_acc = reinterpret_cast<const uint32_t*>(d.d_verify + extra_at);
        st.d_wgt = d.d_verify + extra_at + LedgerStage::acc_units(ses_staged);
        st.ctl_at = extra_at + LedgerStage::acc_units(ses_staged) + ses_staged;
    }
    *staged = h_staged;
    return BM_OK;
}

// bm_jobs_verify_gpu on the first device, the shape of pool_verify_impl: one copy up,
// one launch, the verdicts back in one copy.  The caller's arrays are written last.
int jobs_verify_impl(bm_ctx* ctx, const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions,
                     size_t nsessions, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                     bm_pool_verify_result_t* out) {
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    PoolStage st;
    host::JobsPlan plan;
    const bm_jobs_submit_t* staged = nullptr;
    BM_TRY(jobs_verify_launch(d, jobs, njobs, sessions, nsessions, submits, n, 0, 0, st, plan, &staged));
    BM_HIP(hipMemcpyAsync(d.h_verify + st.in_u, st.d_out, 8 * st.out_u, hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    BM_TRY(host::jobs_verify_tripwire(jobs, njobs, sessions, nsessions, submits, n, plan, staged, st.got, 0));
    bm_pool_verify_result_t r;
    host::pool_verify_count(st.got, n, r);
    std::memcpy(verdicts, st.got, n * sizeof(bm_job_verdict_t));
    *out = r;
    return BM_OK;
}

// ---- the share set on a device (bm_share_set_host.hpp, bm_share_set.hpp) ----
// The four kernels, registered by bm_share_set_inst.hip at load time
const void* g_share_insert = nullptr;
const void* g_share_resolve = nullptr;
const void* g_share_commit = nullptr;
const void* g_share_rollback = nullptr;

// Winners store EMPTY again: the table is what it was before the call's insert.
int share_set_rollback(DeviceCtx& d, const ShareSetArgs& S, uint32_t* d_slots, const uint32_t* lane_slot,
                       const uint32_t* lane_rank) {
    ShareSetArgs A = S;
    void* args[] = {&A, &d_slots, &lane_slot, &lane_rank};
    BM_HIP(hipLaunchKernel(g_share_rollback, dim3((S.n + 63) / 64), dim3(kShareSetThreads), args, 0, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    return BM_OK;
}

// bm_share_set_verify and bm_share_set_verify_jobs on a device set: a verifier's
// stage and launch (`launch`: bm_pool_verify_gpu's or bm_jobs_verify_gpu's, with one
// control unit and n lane units), then the
// insert and the resolve on the same stream, one copy back (the two control words
// and the verdicts, adjacent on the device), and the commit -- or the rollback, when
// the batch does not fit.  `tripwire` is that verifier's, over the verdicts with
// BM_SUBMIT_DUPLICATE masked off.  The caller's arrays are written last.  From the insert's
// launch to the end of the commit or rollback the table holds this call's candidate
// ids: a failure in between poisons the set until it is cleared.  `after` (the
// ledger's credit; nothing for the plain calls) runs once the commit is enqueued, over
// the stage and the final verdicts; its failure is one of those.
template <class Launch, class Tripwire, class After>
int share_set_verify_impl(bm_share_set_t* set, size_t n, Launch&& launch, Tripwire&& tripwire, After&& after,
                          bm_job_verdict_t* verdicts, bm_share_set_result_t* out) {
    if (!g_share_insert || !g_share_resolve || !g_share_commit || !g_share_rollback) return BM_EINTERNAL;
    if (set->poisoned) return BM_EINTERNAL;
    DeviceCtx& d = set->ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    static_assert(kShareCtlWords * sizeof(uint32_t) == sizeof(uint64_t), "the control words are one unit");
    PoolStage st;
    BM_TRY(launch(d, st));
    ShareSetArgs S;
    S.n = (uint32_t)n;
    S.nslots = set->nslots;
    S.count = (uint32_t)set->count;
    S.capacity = (uint32_t)set->capacity;
    uint32_t* d_verdicts = st.d_out;
    uint32_t* d_ctl = st.d_out - kShareCtlWords;
    uint32_t* lane_slot = reinterpret_cast<uint32_t*>(st.d_lanes);
    uint32_t* lane_rank = lane_slot + n;
    const uint32_t* d_keys = set->d_keys;
    uint32_t* d_slots = set->d_slots;
    const dim3 grid((uint32_t)((n + 63) / 64)), block(kShareSetThreads);
    const uint32_t* ctl = reinterpret_cast<const uint32_t*>(st.got) - kShareCtlWords;
    set->poisoned = true;
    {
        void* args[] = {&S, &d_verdicts, &d_keys, &d_slots, &lane_slot, &d_ctl};
        BM_HIP(hipLaunchKernel(g_share_insert, grid, block, args, 0, d.stream));
    }
    {
        void* args[] = {&S, &d_verdicts, &d_slots, &lane_slot, &lane_rank, &d_ctl};
        BM_HIP(hipLaunchKernel(g_share_resolve, grid, block, args, 0, d.stream));
    }
    BM_HIP(hipMemcpyAsync(d.h_verify + st.in_u - 1, d_ctl, 8 * (1 + st.out_u), hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    const uint32_t fault = ctl[kShareCtlFault];
    const uint64_t winners = ctl[kShareCtlWinners];
    bm_share_set_result_t r;
    host::share_set_count(st.got, n, r);
    uint64_t eligible = 0;
    for (size_t i = 0; i < n; ++i) eligible += share_eligible(st.got[i].status) ? 1 : 0;
    int rc = BM_OK;
    if (fault & kShareFaultId)
        rc = BM_EINTERNAL;
    else if ((fault & kShareFaultFull) || set->count + winners > set->capacity)
        rc = BM_EFULL;
    else if (winners + r.duplicates != eligible)  // every eligible lane is a winner or a duplicate
        rc = BM_EINTERNAL;
    else
        rc = tripwire(st.got);
    if (rc != BM_OK) {
        BM_TRY(share_set_rollback(d, S, d_slots, lane_slot, lane_rank));
        set->poisoned = false;
        return rc;
    }
    {
        uint32_t* keys = set->d_keys;
        void* args[] = {&S, &d_verdicts, &keys, &d_slots, &lane_slot, &lane_rank};
        BM_HIP(hipLaunchKernel(g_share_commit, grid, block, args, 0, d.stream));
    }
    BM_TRY(after(d, st));
    BM_HIP(hipStreamSynchronize(d.stream));
    set->poisoned = false;
    set->count += winners;
    r.recorded = winners;
    r.count = set->count;
    std::memcpy(verdicts, st.got, n * sizeof(bm_job_verdict_t));
    *out = r;
    return BM_OK;
}

int share_set_clear_impl(bm_share_set_t* set) {
    DeviceCtx& d = set->ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    BM_HIP(hipMemsetAsync(set->d_slots, 0xFF, sizeof(uint32_t) * (size_t)set->nslots, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    set->count = 0;
    set->poisoned = false;
    return BM_OK;
}

int share_set_verify_op(bm_share_set_t* set, const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                        const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                        bm_job_verdict_t* verdicts, bm_share_set_result_t* out) {
    DeviceGuard guard;
    return guarded([&] {
        return share_set_verify_impl(
            set, n,
            [&](DeviceCtx& d, PoolStage& st) {
                return pool_verify_launch(d, job, sessions, nsessions, submits, n, ntime_lo, ntime_hi, 1, n, st);
            },
            [&](const bm_job_verdict_t* got) {
                return pool_verify_tripwire(job, sessions, nsessions, submits, n, ntime_lo, ntime_hi, got,
                                            BM_SUBMIT_DUPLICATE);
            },
            [](DeviceCtx&, const PoolStage&) { return (int)BM_OK; }, verdicts, out);
    });
}

int share_set_verify_jobs_op(bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                             const bm_pool_session_t* sessions, size_t nsessions, const bm_jobs_submit_t* submits,
                             size_t n, bm_job_verdict_t* verdicts, bm_share_set_result_t* out) {
    DeviceGuard guard;
    return guarded([&] {
        host::JobsPlan plan;
        const bm_jobs_submit_t* staged = nullptr;
        return share_set_verify_impl(
            set, n,
            [&](DeviceCtx& d, PoolStage& st) {
                return jobs_verify_launch(d, jobs, njobs, sessions, nsessions, submits, n, 1, n, st, plan, &staged);
            },
            [&](const bm_job_verdict_t* got) {
                return host::jobs_verify_tripwire(jobs, njobs, sessions, nsessions, submits, n, plan, staged, got,
                                                  BM_SUBMIT_DUPLICATE);
            },
            [](DeviceCtx&, const PoolStage&) { return (int)BM_OK; }, verdicts, out);
    });
}

int share_set_clear_op(bm_share_set_t* set) {
    DeviceGuard guard;
    return share_set_clear_impl(set);
}

void share_set_destroy_op(bm_share_set_t* set) {
    DeviceGuard guard;
    DeviceCtx& d = set->ctx->devs[0];
    (void)hipSetDevice(d.id);
    (void)hipStreamSynchronize(d.stream);
    if (set->d_keys) (void)hipFree(set->d_keys);
    if (set->d_slots) (void)hipFree(set->d_slots);
    set->d_keys = set->d_slots = nullptr;
}

const ShareSetDeviceOps kShareSetOps = {share_set_verify_op, share_set_verify_jobs_op, share_set_clear_op,
                                        share_set_destroy_op};

// The set's two device arrays, the table empty.  A failed allocation frees what it
// made and leaves the context as it was.
int share_set_create_impl(bm_ctx* ctx, bm_share_set_t* set) {
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, sizeof(uint32_t) * kShareKeyWords * set->capacity);
    if (e == hipSuccess) {
        set->d_keys = static_cast<uint32_t*>(p);
        e = hipMalloc(&p, sizeof(uint32_t) * (size_t)set->nslots);
        if (e == hipSuccess) set->d_slots = static_cast<uint32_t*>(p);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? BM_ENOMEM : BM_EHIP;
    }
    return share_set_clear_impl(set);
}

// ---- the ledger on a device (bm_ledger_host.hpp, bm_ledger.hpp) ----
// The two kernels, registered by bm_ledger_inst.hip at load time
const void* g_ledger_credit = nullptr;
const void* g_ledger_fill = nullptr;

// The empty-row pattern over rows [first, first + count), enqueued.
int ledger_fill(DeviceCtx& d, bm_ledger_t* ledger, size_t first, size_t count) {
    if (!g_ledger_fill) return BM_EINTERNAL;
    if (count == 0) return BM_OK;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(ledger->d_rows) + kLedgerRowWords * first;
    uint64_t nwords = (uint64_t)kLedgerRowWords * count;
    const uint32_t grid = (uint32_t)((nwords + kLedgerFillThreads - 1) / kLedgerFillThreads);
    void* args[] = {&words, &nwords};
    BM_HIP(hipLaunchKernel(g_ledger_fill, dim3(grid), dim3(kLedgerFillThreads), args, 0, d.stream));
    return BM_OK;
}

// The credit of a verified batch, once the call can no longer be refused: the launch
// of ledger_credit_kernel over the stage of jobs_verify_launch (with a LedgerStage)
// and the final verdicts on the device, its seven control words back, and their
// compare with the totals of the verdicts the host holds (`want`).  From the launch
// on the rows may hold a part of this call: a failure poisons the ledger.
int ledger_credit_launch(bm_ledger_t* ledger, DeviceCtx& d, const PoolStage& st, size_t n, size_t nsessions) {
    LedgerArgs A;
    A.n = (uint32_t)n;
    A.nsessions = (uint32_t)nsessions;
    A.rows = (uint32_t)ledger->rows;
    A.rounds = ledger->peel;
    const uint32_t* d_sub = reinterpret_cast<const uint32_t*>(st.d_sub);
    const uint32_t* d_verdicts = st.d_out;
    const uint32_t* d_acc = st.d_acc;
    const uint64_t* d_wgt = st.d_wgt;
    uint64_t* d_ctl = d.d_verify + st.ctl_at;
    uint64_t* d_rows = ledger->d_rows;
    void* args[] = {&A, &d_sub, &d_verdicts, &d_acc, &d_wgt, &d_rows, &d_ctl};
    ledger->poisoned = true;
    BM_HIP(hipLaunchKernel(g_ledger_credit, dim3((uint32_t)((n + kLedgerThreads - 1) / kLedgerThreads)),
                           dim3(kLedgerThreads), args, 0, d.stream));
    return BM_OK;
}

int ledger_credit(bm_ledger_t* ledger, DeviceCtx& d, const PoolStage& st, size_t n, size_t nsessions,
                  const host::LedgerTotals& want) {
    BM_TRY(ledger_credit_launch(ledger, d, st, n, nsessions));
    const size_t ctl_at = st.ctl_at;
    uint64_t* d_ctl = d.d_verify + ctl_at;
    BM_HIP(hipMemcpyAsync(d.h_verify + ctl_at, d_ctl, 8 * kLedgerCtlWords, hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    if (std::memcmp(d.h_verify + ctl_at, want.word, 8 * kLedgerCtlWords) != 0) return BM_EINTERNAL;
    ledger->poisoned = false;
    return BM_OK;
}

// bm_ledger_verify_jobs on a device ledger: share_set_verify_impl with the credit as
// its step after the commit, or without a set jobs_verify_impl's shape with the credit
// after the tripwire.  The caller's arrays are written last.
int ledger_verify_jobs_impl(bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                            const bm_pool_session_t* sessions, size_t nsessions, const uint32_t* accounts,
                            const uint64_t* weights, const bm_jobs_submit_t* submits, size_t n,
                            bm_job_verdict_t* verdicts, bm_ledger_result_t* out) {
    if (!g_ledger_credit || !g_jobs_verify) return BM_EINTERNAL;
    if (ledger->poisoned) return BM_EINTERNAL;
    const LedgerStage lg = {accounts, weights};
    host::JobsPlan plan;
    const bm_jobs_submit_t* staged = nullptr;
    host::LedgerTotals t;
    bm_share_set_result_t r;
    if (set) {
        BM_TRY(share_set_verify_impl(
            set, n,
            [&](DeviceCtx& d, PoolStage& st) {
                return jobs_verify_launch(d, jobs, njobs, sessions, nsessions, submits, n, 1, n, st, plan, &staged, &lg);
            },
            [&](const bm_job_verdict_t* got) {
                return host::jobs_verify_tripwire(jobs, njobs, sessions, nsessions, submits, n, plan, staged, got,
                                                  BM_SUBMIT_DUPLICATE);
            },
            [&](DeviceCtx& d, const PoolStage& st) {
                host::ledger_totals(submits, st.got, n, nsessions, weights, t);
                return ledger_credit(ledger, d, st, n, nsessions, t);
            },
            verdicts, &r));
    } else {
        DeviceCtx& d = ledger->ctx->devs[0];
        BM_HIP(hipSetDevice(d.id));
        PoolStage st;
        BM_TRY(jobs_verify_launch(d, jobs, njobs, sessions, nsessions, submits, n, 0, 0, st, plan, &staged, &lg));
        BM_HIP(hipMemcpyAsync(d.h_verify + st.in_u, st.d_out, 8 * st.out_u, hipMemcpyDeviceToHost, d.stream));
        BM_HIP(hipStreamSynchronize(d.stream));
        BM_TRY(host::jobs_verify_tripwire(jobs, njobs, sessions, nsessions, submits, n, plan, staged, st.got, 0));
        host::ledger_totals(submits, st.got, n, nsessions, weights, t);
        BM_TRY(ledger_credit(ledger, d, st, n, nsessions, t));
        host::share_set_count(st.got, n, r);
        std::memcpy(verdicts, st.got, n * sizeof(bm_job_verdict_t));
    }
    host::ledger_result(r, t, *out);
    return BM_OK;
}

int ledger_verify_jobs_op(bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                          const bm_pool_session_t* sessions, size_t nsessions, const uint32_t* accounts,
                          const uint64_t* weights, const bm_jobs_submit_t* submits, size_t n,
                          bm_job_verdict_t* verdicts, bm_ledger_result_t* out) {
    DeviceGuard guard;
    return guarded([&] {
        return ledger_verify_jobs_impl(ledger, set, jobs, njobs, sessions, nsessions, accounts, weights, submits, n,
                                       verdicts, out);
    });
}

// bm_ledger_read and bm_ledger_drain: one copy down on the stream and, for a drain,
// the fill of exactly those rows behind it.  The caller's array is written last.
int ledger_read_impl(bm_ledger_t* ledger, size_t first, size_t count, bool drain, bm_ledger_row_t* out) {
    if (ledger->poisoned) return BM_EINTERNAL;
    if (count == 0) return BM_OK;
    DeviceCtx& d = ledger->ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    std::vector<bm_ledger_row_t> tmp(count);
    BM_HIP(hipMemcpyAsync(tmp.data(), ledger->d_rows + kLedgerRowWords * first, count * sizeof(bm_ledger_row_t),
                          hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    if (drain) {
        ledger->poisoned = true;
        BM_TRY(ledger_fill(d, ledger, first, count));
        BM_HIP(hipStreamSynchronize(d.stream));
        ledger->poisoned = false;
    }
    std::memcpy(out, tmp.data(), count * sizeof(bm_ledger_row_t));
    return BM_OK;
}

int ledger_read_op(bm_ledger_t* ledger, size_t first, size_t count, bool drain, bm_ledger_row_t* out) {
    DeviceGuard guard;
    return guarded([&] { return ledger_read_impl(ledger, first, count, drain, out); });
}

int ledger_clear_op(bm_ledger_t* ledger) {
    DeviceGuard guard;
    DeviceCtx& d = ledger->ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    BM_TRY(ledger_fill(d, ledger, 0, ledger->rows));
    BM_HIP(hipStreamSynchronize(d.stream));
    ledger->poisoned = false;
    return BM_OK;
}

void ledger_destroy_op(bm_ledger_t* ledger) {
    DeviceGuard guard;
    DeviceCtx& d = ledger->ctx->devs[0];
    (void)hipSetDevice(d.id);
    (void)hipStreamSynchronize(d.stream);
    if (ledger->d_rows) (void)hipFree(ledger->d_rows);
    ledger->d_rows = nullptr;
}

const LedgerDeviceOps kLedgerOps = {ledger_verify_jobs_op, ledger_read_op, ledger_clear_op, ledger_destroy_op};

// The ledger's device array, every row empty.  A failed allocation leaves the context
// as it was.
int ledger_create_impl(bm_ctx* ctx, bm_ledger_t* ledger) {
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, sizeof(bm_ledger_row_t) * ledger->rows);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? BM_ENOMEM : BM_EHIP;
    }
    ledger->d_rows = static_cast<uint64_t*>(p);
    return ledger_clear_op(ledger);
}

// ---- the session table on a device (bm_sessions_host.hpp, bm_sessions.hpp) ----
// The three kernels, registered by bm_sessions_inst.hip at load time
const void* g_sessions_set = nullptr;
const void* g_sessions_tally = nullptr;
const void* g_sessions_retarget = nullptr;

// bm_sessions_set: the resolved records up in one copy, one launch scatters them.  The
// buffers are job_verify_impl's.  From the launch on slots may hold a part of the call:
// a failure poisons the table.
int sessions_set_impl(bm_sessions_t* t, const SessionSetRecord* recs, size_t k, uint64_t now_ms) {
    if (!g_sessions_set) return BM_EINTERNAL;
    DeviceCtx& d = t->ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    const size_t units = k * sizeof(SessionSetRecord) / 8;
    BM_TRY(grow(d, d.h_verify, d.hverify_cap, units, sizeof(uint64_t), true));
    BM_TRY(grow(d, d.d_verify, d.verify_cap, units));
    std::memcpy(d.h_verify, recs, 8 * units);
    BM_HIP(hipMemcpyAsync(d.d_verify, d.h_verify, 8 * units, hipMemcpyHostToDevice, d.stream));
    uint32_t n = (uint32_t)k, capacity = (uint32_t)t->capacity;
    const uint32_t* d_recs = reinterpret_cast<const uint32_t*>(d.d_verify);
    void* args[] = {&n, &capacity, &now_ms, &d_recs, &t->d_sessions, &t->d_accounts, &t->d_weights, &t->d_state};
    t->poisoned = true;
    BM_HIP(hipLaunchKernel(g_sessions_set, dim3((n + kSessionsThreads - 1) / kSessionsThreads), dim3(kSessionsThreads),
                           args, 0, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    t->poisoned = false;
    return BM_OK;
}

int sessions_set_op(bm_sessions_t* t, const SessionSetRecord* recs, size_t k, uint64_t now_ms) {
    DeviceGuard guard;
    return guarded([&] { return sessions_set_impl(t, recs, k, now_ms); });
}

// The states of slots [first, first + count): one copy down on the stream.
int sessions_states_op(bm_sessions_t* t, size_t first, size_t count, bm_session_state_t* out) {
    DeviceGuard guard;
    DeviceCtx& d = t->ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    BM_HIP(hipMemcpyAsync(out, t->d_state + kSessionStateWords * first, count * sizeof(bm_session_state_t),
                          hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    return BM_OK;
}

// What follows a verified batch once the call can no longer be refused: the credit
// kernel with a ledger, the tally kernel, the eight control words back in one copy and
// their compare with the totals of the verdicts the host holds.  From the first launch
// on the rows and the states may hold a part of this call: a failure poisons both.
int sessions_after(bm_sessions_t* t, bm_ledger_t* ledger, DeviceCtx& d, const PoolStage& st, size_t n, size_t nsessions,
                   const host::LedgerTotals& want) {
    if (ledger) BM_TRY(ledger_credit_launch(ledger, d, st, n, nsessions));
    SessionsTallyArgs A;
    A.n = (uint32_t)n;
    A.nsessions = (uint32_t)nsessions;
    const uint32_t* d_sub = reinterpret_cast<const uint32_t*>(st.d_sub);
    const uint32_t* d_verdicts = st.d_out;
    uint64_t* d_state = t->d_state;
    uint64_t* d_ctl = d.d_verify + st.ctl_at;
    uint64_t* d_tally = d_ctl + kTallyCtlWord;
    void* args[] = {&A, &d_sub, &d_verdicts, &d_state, &d_tally};
    t->poisoned = true;
    BM_HIP(hipLaunchKernel(g_sessions_tally, dim3((uint32_t)((n + kSessionsThreads - 1) / kSessionsThreads)),
                           dim3(kSessionsThreads), args, 0, d.stream));
    static_assert(kTallyCtlWord < kLedgerCtlUnits && kTallyCtlWord >= kLedgerCtlWords, "the tally's word is the padding");
    BM_HIP(hipMemcpyAsync(d.h_verify + st.ctl_at, d_ctl, 8 * kLedgerCtlUnits, hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    const uint64_t* got = d.h_verify + st.ctl_at;
    if (ledger) {
        if (std::memcmp(got, want.word, 8 * kLedgerCtlWords) != 0) return BM_EINTERNAL;
        ledger->poisoned = false;
    }
    if (got[kTallyCtlWord] != want.word[kLedgerAccepted]) return BM_EINTERNAL;
    t->poisoned = false;
    return BM_OK;
}

// bm_sessions_verify_jobs on a device table: ledger_verify_jobs_impl's two shapes over
// the table's mirror on the host and the table's arrays on the device, with
// sessions_after where the credit is.  The caller's arrays are written last.
int sessions_verify_jobs_impl(bm_sessions_t* t, bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs,
                              size_t njobs, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                              bm_ledger_result_t* out) {
    if (!g_sessions_tally || !g_jobs_verify || (ledger && !g_ledger_credit)) return BM_EINTERNAL;
    if (ledger && ledger->poisoned) return BM_EINTERNAL;
    const bm_pool_session_t* sessions = t->sessions.data();
    const size_t nsessions = (size_t)t->count;
    const uint64_t* weights = t->weights.data();
    const LedgerStage lg = {t->accounts.data(), weights, t->d_sessions, t->d_accounts, t->d_weights};
    host::JobsPlan plan;
    const bm_jobs_submit_t* staged = nullptr;
    host::LedgerTotals tot;
    bm_share_set_result_t r;
    if (set) {
        BM_TRY(share_set_verify_impl(
            set, n,
            [&](DeviceCtx& d, PoolStage& st) {
                return jobs_verify_launch(d, jobs, njobs, sessions, nsessions, submits, n, 1, n, st, plan, &staged, &lg);
            },
            [&](const bm_job_verdict_t* got) {
                return host::jobs_verify_tripwire(jobs, njobs, sessions, nsessions, submits, n, plan, staged, got,
                                                  BM_SUBMIT_DUPLICATE);
            },
            [&](DeviceCtx& d, const PoolStage& st) {
                host::ledger_totals(submits, st.got, n, nsessions, weights, tot);
                return sessions_after(t, ledger, d, st, n, nsessions, tot);
            },
            verdicts, &r));
    } else {
        DeviceCtx& d = t->ctx->devs[0];
        BM_HIP(hipSetDevice(d.id));
        PoolStage st;
        BM_TRY(jobs_verify_launch(d, jobs, njobs, sessions, nsessions, submits, n, 0, 0, st, plan, &staged, &lg));
        BM_HIP(hipMemcpyAsync(d.h_verify + st.in_u, st.d_out, 8 * st.out_u, hipMemcpyDeviceToHost, d.stream));
        BM_HIP(hipStreamSynchronize(d.stream));
        BM_TRY(host::jobs_verify_tripwire(jobs, njobs, sessions, nsessions, submits, n, plan, staged, st.got, 0));
        host::ledger_totals(submits, st.got, n, nsessions, weights, tot);
        BM_TRY(sessions_after(t, ledger, d, st, n, nsessions, tot));
        host::share_set_count(st.got, n, r);
        std::memcpy(verdicts, st.got, n * sizeof(bm_job_verdict_t));
    }
    host::ledger_result(r, tot, *out);
    return BM_OK;
}

int sessions_verify_jobs_op(bm_sessions_t* t, bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs,
                            size_t njobs, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                            bm_ledger_result_t* out) {
    DeviceGuard guard;
    return guarded([&] { return sessions_verify_jobs_impl(t, ledger, set, jobs, njobs, submits, n, verdicts, out); });
}

// bm_sessions_retarget on a device table.  Device buffer, in 8-byte units: the eight
// control words, then the change list of A.cap entries.  The decide pass, the control
// words back, then exactly the entries the pass wrote; the host sorts them by session and
// checks each against its mirror and against bm_target_from_difficulty_fx; then the apply
// pass and the control words again.  Nothing is written to the table before the apply
// pass: BM_EFULL leaves it as it was.
// The compacted list (a wave's entries ascending, the waves in the order their atomics
// landed) into `out`, ascending by session.  A short list is copied and sorted; a long
// one goes through a table of positions by session, one pass over the slots.  An entry
// whose session is out of range or repeated stays out of order: the caller's check fails.
void sessions_order_changes(const bm_vardiff_change_t* list, size_t k, uint32_t count, bm_vardiff_change_t* out) {
    if (k * 16 < count) {
        std::memcpy(out, list, k * sizeof(bm_vardiff_change_t));
        std::sort(out, out + k, [](const bm_vardiff_change_t& a, const bm_vardiff_change_t& b) { return a.session < b.session; });
        return;
    }
    std::vector<uint32_t> at(count, 0xFFFFFFFFu);
    size_t placed = 0;
    for (size_t i = 0; i < k; ++i)
        if (list[i].session < count && at[list[i].session] == 0xFFFFFFFFu) at[list[i].session] = (uint32_t)i;
    for (uint32_t s = 0; s < count; ++s)
        if (at[s] != 0xFFFFFFFFu) out[placed++] = list[at[s]];
    for (size_t i = 0; placed < k; ++i)  // what found no place of its own: in the list's order, behind the rest
        if (!(list[i].session < count && at[list[i].session] == (uint32_t)i)) out[placed++] = list[i];
}

int sessions_retarget_impl(bm_sessions_t* t, const SessionsRetargetArgs& args_in, bm_vardiff_change_t* changes,
                           bm_vardiff_result_t* out) {
    if (!g_sessions_retarget) return BM_EINTERNAL;
    bm_vardiff_result_t r;
    std::memset(&r, 0, sizeof r);
    SessionsRetargetArgs A = args_in;
    if (A.count == 0) {
        *out = r;
        return BM_OK;
    }
    DeviceCtx& d = t->ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    const size_t entry_u = sizeof(bm_vardiff_change_t) / 8;
    const size_t units = kRetargetCtlWords + (size_t)A.cap * entry_u;
    BM_TRY(grow(d, d.h_verify, d.hverify_cap, units, sizeof(uint64_t), true));
    BM_TRY(grow(d, d.d_verify, d.verify_cap, units));
    uint64_t* d_ctl = d.d_verify;
    uint32_t* d_list = reinterpret_cast<uint32_t*>(d.d_verify + kRetargetCtlWords);
    const dim3 grid((A.count + kSessionsThreads - 1) / kSessionsThreads), block(kSessionsThreads);
    void* args[] = {&A, &t->d_sessions, &t->d_weights, &t->d_state, &d_list, &d_ctl};
    BM_HIP(hipMemsetAsync(d_ctl, 0, 8 * kRetargetCtlWords, d.stream));
    A.apply = 0;
    BM_HIP(hipLaunchKernel(g_sessions_retarget, grid, block, args, 0, d.stream));
    BM_HIP(hipMemcpyAsync(d.h_verify, d_ctl, 8 * kRetargetCtlWords, hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    const uint64_t* ctl = d.h_verify;
    r.open = ctl[kRetargetOpen], r.evaluated = ctl[kRetargetEvaluated], r.changed = ctl[kRetargetChanged];
    r.raised = ctl[kRetargetRaised], r.lowered = ctl[kRetargetLowered];
    if (r.open > A.count || r.evaluated > r.open || r.changed > r.evaluated || r.raised + r.lowered != r.changed) {
        t->poisoned = true;
        return BM_EINTERNAL;
    }
    if (r.changed > A.cap) {  // A.cap is the caller's, or the count where that is smaller
        *out = r;
        return BM_EFULL;
    }
    const size_t k = (size_t)r.changed;
    if (k) {
        BM_HIP(hipMemcpyAsync(d.h_verify + kRetargetCtlWords, d_list, k * sizeof(bm_vardiff_change_t),
                              hipMemcpyDeviceToHost, d.stream));
        BM_HIP(hipStreamSynchronize(d.stream));
        sessions_order_changes(reinterpret_cast<const bm_vardiff_change_t*>(d.h_verify + kRetargetCtlWords), k, A.count,
                               changes);
    }
    for (size_t i = 0; i < k; ++i) {
        const bm_vardiff_change_t& c = changes[i];
        uint8_t want[32];
        bool ok = c.session < A.count && c.reserved == 0 && (i == 0 || changes[i - 1].session < c.session);
        ok = ok && c.old_fx == t->weights[c.session] && c.new_fx != c.old_fx && c.new_fx != 0;
        ok = ok && bm_target_from_difficulty_fx(c.new_fx, want) == BM_OK && std::memcmp(want, c.target, 32) == 0;
        if (!ok) {
            t->poisoned = true;
            return BM_EINTERNAL;
        }
    }
    A.apply = 1;
    t->poisoned = true;
    BM_HIP(hipLaunchKernel(g_sessions_retarget, grid, block, args, 0, d.stream));
    BM_HIP(hipMemcpyAsync(d.h_verify, d_ctl, 8 * kRetargetCtlWords, hipMemcpyDeviceToHost, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    if (ctl[kRetargetApplied] != r.changed || ctl[kRetargetChanged] != r.changed) return BM_EINTERNAL;
    t->poisoned = false;
    *out = r;
    return BM_OK;
}

int sessions_retarget_op(bm_sessions_t* t, const SessionsRetargetArgs& A, bm_vardiff_change_t* changes, size_t,
                         bm_vardiff_result_t* out) {
    DeviceGuard guard;
    return guarded([&] { return sessions_retarget_impl(t, A, changes, out); });
}

// Every slot never set: zeros in all four arrays.
int sessions_clear_op(bm_sessions_t* t) {
    DeviceGuard guard;
    DeviceCtx& d = t->ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    BM_HIP(hipMemsetAsync(t->d_sessions, 0, sizeof(bm_pool_session_t) * t->capacity, d.stream));
    BM_HIP(hipMemsetAsync(t->d_accounts, 0, sizeof(uint32_t) * t->capacity, d.stream));
    BM_HIP(hipMemsetAsync(t->d_weights, 0, sizeof(uint64_t) * t->capacity, d.stream));
    BM_HIP(hipMemsetAsync(t->d_state, 0, sizeof(bm_session_state_t) * t->capacity, d.stream));
    BM_HIP(hipStreamSynchronize(d.stream));
    return BM_OK;
}

void sessions_destroy_op(bm_sessions_t* t) {
    DeviceGuard guard;
    DeviceCtx& d = t->ctx->devs[0];
    (void)hipSetDevice(d.id);
    (void)hipStreamSynchronize(d.stream);
    if (t->d_sessions) (void)hipFree(t->d_sessions);
    if (t->d_accounts) (void)hipFree(t->d_accounts);
    if (t->d_weights) (void)hipFree(t->d_weights);
    if (t->d_state) (void)hipFree(t->d_state);
    t->d_sessions = t->d_accounts = nullptr;
    t->d_weights = t->d_state = nullptr;
}

const SessionsDeviceOps kSessionsOps = {sessions_set_op,      sessions_states_op, sessions_verify_jobs_op,
                                        sessions_retarget_op, sessions_clear_op,  sessions_destroy_op};

// The table's four device arrays, every slot never set.  A failed allocation leaves what
// it made to bm_sessions_destroy and the context as it was.
int sessions_create_impl(bm_ctx* ctx, bm_sessions_t* t) {
    DeviceCtx& d = ctx->devs[0];
    BM_HIP(hipSetDevice(d.id));
    const size_t bytes[4] = {sizeof(bm_pool_session_t), sizeof(uint32_t), sizeof(uint64_t), sizeof(bm_session_state_t)};
    void* p[4] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipMalloc(&p[i], bytes[i] * t->capacity);
    t->d_sessions = static_cast<uint32_t*>(p[0]);
    t->d_accounts = static_cast<uint32_t*>(p[1]);
    t->d_weights = static_cast<uint64_t*>(p[2]);
    t->d_state = static_cast<uint64_t*>(p[3]);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? BM_ENOMEM : BM_EHIP;
    }
    return sessions_clear_op(t);
}

}  // namespace
}  // namespace bm

extern "C" {

void bm_register_pool_verify_kernel(const void* fn) { bm::g_pool_verify = fn; }

int bm_pool_verify_gpu(bm_ctx_t* ctx, const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                       const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                       bm_job_verdict_t* verdicts, bm_pool_verify_result_t* out) {
    if (!ctx) return BM_EINVAL;
    const int rc = bm::host::pool_verify_check(job, sessions, nsessions, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    if (n == 0) {
        std::memset(out, 0, sizeof *out);
        return BM_OK;
    }
    bm::DeviceGuard guard;
    return bm::guarded([&] {
        return bm::pool_verify_impl(ctx, job, sessions, nsessions, submits, n, ntime_lo, ntime_hi, verdicts, out);
    });
}

void bm_register_jobs_verify_kernel(const void* fn) { bm::g_jobs_verify = fn; }

int bm_jobs_verify_gpu(bm_ctx_t* ctx, const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions,
                       size_t nsessions, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                       bm_pool_verify_result_t* out) {
    if (!ctx) return BM_EINVAL;
    const int rc = bm::host::jobs_verify_check(jobs, njobs, sessions, nsessions, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    if (n == 0) {
        std::memset(out, 0, sizeof *out);
        return BM_OK;
    }
    bm::DeviceGuard guard;
    return bm::guarded([&] {
        return bm::jobs_verify_impl(ctx, jobs, njobs, sessions, nsessions, submits, n, verdicts, out);
    });
}

void bm_register_share_set_kernels(const void* insert, const void* resolve, const void* commit, const void* rollback) {
    bm::g_share_insert = insert;
    bm::g_share_resolve = resolve;
    bm::g_share_commit = commit;
    bm::g_share_rollback = rollback;
}

int bm_share_set_create(bm_ctx_t* ctx, size_t capacity, bm_share_set_t** out) {
    if (!ctx || !out || capacity == 0 || capacity > BM_MAX_SHARE_SET) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    bm_share_set_t* set = new (std::nothrow) bm_share_set;
    if (!set) return BM_ENOMEM;
    set->capacity = capacity;
    set->nslots = bm::share_set_slots(capacity);
    set->ctx = ctx;
    set->ops = &bm::kShareSetOps;
    bm::DeviceGuard guard;
    const int rc = bm::share_set_create_impl(ctx, set);
    if (rc != BM_OK) {
        bm_share_set_destroy(set);
        return rc;
    }
    *out = set;
    return BM_OK;
}

void bm_register_ledger_kernels(const void* credit, const void* fill) {
    bm::g_ledger_credit = credit;
    bm::g_ledger_fill = fill;
}

int bm_ledger_create(bm_ctx_t* ctx, size_t rows, bm_ledger_t** out) {
    if (!ctx || !out || rows == 0 || rows > BM_MAX_LEDGER_ROWS) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    bm_ledger_t* ledger = new (std::nothrow) bm_ledger;
    if (!ledger) return BM_ENOMEM;
    ledger->rows = rows;
    ledger->ctx = ctx;
    ledger->ops = &bm::kLedgerOps;
    const int rc = bm::ledger_create_impl(ctx, ledger);
    if (rc != BM_OK) {
        bm_ledger_destroy(ledger);
        return rc;
    }
    *out = ledger;
    return BM_OK;
}

void bm_register_sessions_kernels(const void* set, const void* tally, const void* retarget) {
    bm::g_sessions_set = set;
    bm::g_sessions_tally = tally;
    bm::g_sessions_retarget = retarget;
}

int bm_sessions_create(bm_ctx_t* ctx, size_t capacity, bm_sessions_t** out) {
    if (!ctx || !out || capacity == 0 || capacity > BM_MAX_POOL_SESSIONS) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    return bm::guarded([&] {
        bm_sessions_t* t = new (std::nothrow) bm_sessions;
        if (!t) return (int)BM_ENOMEM;
        t->capacity = capacity;
        t->ctx = ctx;
        t->ops = &bm::kSessionsOps;
        int rc = BM_OK;
        try {  // the mirror
            t->sessions.assign(capacity, bm_pool_session_t());
            t->accounts.assign(capacity, 0);
            t->weights.assign(capacity, 0);
        } catch (...) {
            rc = BM_ENOMEM;
        }
        if (rc == BM_OK) {
            bm::DeviceGuard guard;
            rc = bm::sessions_create_impl(ctx, t);
        }
        if (rc != BM_OK) {
            bm_sessions_destroy(t);
            return rc;
        }
        *out = t;
        return (int)BM_OK;
    });
}

void bm_register_job_verify_kernel(const void* fn) { bm::g_job_verify = fn; }

int bm_job_verify_gpu(bm_ctx_t* ctx, const bm_job_t* job, const uint8_t* target, const bm_job_submit_t* submits,
                      size_t n, bm_job_verdict_t* verdicts, bm_job_verify_result_t* out) {
    if (!ctx) return BM_EINVAL;
    const int rc = bm::host::verify_check(job, target, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    if (n == 0) {
        std::memset(out, 0, sizeof *out);
        return BM_OK;
    }
    bm::DeviceGuard guard;
    return bm::guarded([&] { return bm::job_verify_impl(ctx, job, target, submits, n, verdicts, out); });
}

int bm_reduce_gpu(bm_ctx_t* ctx, const bm_result_t* parts, size_t n, bm_result_t* out) {
    if (!ctx || !out || (n && !parts) || n > BM_MAX_REDUCE) return BM_EINVAL;
    bm::DeviceGuard guard;
    bm_result_t r;
    int rc = bm::reduce_impl(ctx, parts, n, &r);
    if (rc == BM_OK) *out = r;
    return rc;
}

int bm_hash_gpu(bm_ctx_t* ctx, const uint8_t* msg, size_t len, const uint64_t* nonces, size_t n, uint64_t* out) {
    if (!ctx || (n && (!nonces || !out)) || (len && !msg) || len > BM_MAX_MSG_LEN) return BM_EINVAL;
    bm::DeviceGuard guard;
    return bm::hash_impl(ctx, msg, len, nonces, n, out);
}

int bm_header_hash_gpu(bm_ctx_t* ctx, const uint8_t* header, const uint32_t* nonces, size_t n, uint8_t* out) {
    if (!ctx || !header || (n && (!nonces || !out)) || n > BM_MAX_HEADER_HASHES) return BM_EINVAL;
    bm::DeviceGuard guard;
    return bm::guarded([&] { return bm::header_hash_impl(ctx, header, nonces, n, out); });
}

}  // extern "C"
