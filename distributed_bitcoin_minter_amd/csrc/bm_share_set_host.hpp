// bm_share_set_host.hpp -- what a bm_share_set_t is (include/btcminer.h has the
// semantics): shared by bm_share_set.cpp (the entry points and the CPU set: plain
// C++, no HIP, also compiled into tools/share_set_check.cpp's program) and by
// bm_aux.hip (the device set: bm_share_set_create and the three operations a device
// set reaches through `ops`, so that the plain unit links without the HIP runtime).
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "bm_job.hpp"
#include "bm_share_set_args.hpp"

struct bm_ctx;

namespace bm {

using ShareKey = std::array<uint8_t, 32>;  // a header hash, most significant byte first
struct ShareKeyHash {
    size_t operator()(const ShareKey& k) const {  // the least significant end: an accepted share's top is zero
        uint64_t v;
        std::memcpy(&v, k.data() + 24, sizeof v);
        return (size_t)v;
    }
};

// Slots of the device table: the smallest power of two >= max(16, 2 * capacity).
inline uint32_t share_set_slots(size_t capacity) {
    uint32_t s = 16;
    while ((size_t)s < 2 * capacity) s <<= 1;
    return s;
}

// The operations of a device set (bm_aux.hip).
struct ShareSetDeviceOps {
    int (*verify)(bm_share_set_t* set, const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                  const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                  bm_job_verdict_t* verdicts, bm_share_set_result_t* out);
    int (*verify_jobs)(bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions,
                       size_t nsessions, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                       bm_share_set_result_t* out);
    int (*clear)(bm_share_set_t* set);
    void (*destroy)(bm_share_set_t* set);  // the device's memory; the caller deletes the object
};

namespace host {

// What bm_share_set_verify refuses, for either kind of set.
inline int share_set_check(const bm_share_set_t* set, const bm_job_t* job, const bm_pool_session_t* sessions,
                           size_t nsessions, const bm_pool_submit_t* submits, size_t n,
                           const bm_job_verdict_t* verdicts, const bm_share_set_result_t* out) {
    if (!set || !out) return BM_EINVAL;
    static const bm_pool_verify_result_t some = {};  // pool_verify_check only asks that there is one
    return pool_verify_check(job, sessions, nsessions, submits, n, verdicts, &some);
}

// What bm_share_set_verify_jobs refuses, for either kind of set.
inline int share_set_jobs_check(const bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                                const bm_pool_session_t* sessions, size_t nsessions, const bm_jobs_submit_t* submits,
                                size_t n, const bm_job_verdict_t* verdicts, const bm_share_set_result_t* out) {
    if (!set || !out) return BM_EINVAL;
    return jobs_verify_check(jobs, njobs, sessions, nsessions, submits, n, verdicts, out);
}

// *out of a call from its final verdicts, but for recorded and count.
inline void share_set_count(const bm_job_verdict_t* verdicts, size_t n, bm_share_set_result_t& out) {
    bm_pool_verify_result_t r;
    pool_verify_count(verdicts, n, r);
    std::memset(&out, 0, sizeof out);
    out.n = r.n, out.shares = r.shares, out.blocks = r.blocks, out.invalid = r.invalid, out.ntime = r.ntime;
    for (size_t i = 0; i < n; ++i) out.duplicates += (verdicts[i].status & BM_SUBMIT_DUPLICATE) ? 1 : 0;
}

}  // namespace host
}  // namespace bm

struct bm_share_set {
    size_t capacity = 0;
    uint64_t count = 0;
    // a CPU set (ops == nullptr)
    std::unordered_set<bm::ShareKey, bm::ShareKeyHash> keys;
    // a device set, on the first device of ctx
    const bm::ShareSetDeviceOps* ops = nullptr;
    bm_ctx* ctx = nullptr;
    uint32_t* d_keys = nullptr;   // capacity entries of 8 words, indexed by id
    uint32_t* d_slots = nullptr;  // nslots ids
    uint32_t nslots = 0;
    bool poisoned = false;        // a call failed between its insert and its commit or rollback: until the next clear
};

namespace bm {
namespace host {

// The CPU set's step over a batch's plain verdicts, in the caller's order: an
// eligible hash the set holds is flagged BM_SUBMIT_DUPLICATE, any other eligible
// hash is recorded.  What does not fit is found before anything is inserted:
// BM_EFULL with the set and the verdicts untouched.  Throws std::bad_alloc with the
// set as it was.
inline int share_set_apply(bm_share_set& set, bm_job_verdict_t* v, size_t n, uint64_t& recorded) {
    std::vector<ShareKey> fresh;  // this batch's new distinct hashes, in order of first appearance
    {
        std::unordered_set<ShareKey, ShareKeyHash> seen;
        for (size_t i = 0; i < n; ++i) {
            if (!share_eligible(v[i].status)) continue;
            ShareKey k;
            std::memcpy(k.data(), v[i].hash, k.size());
            if (!set.keys.count(k) && seen.insert(k).second) fresh.push_back(k);
        }
    }
    if (set.count + fresh.size() > set.capacity) return BM_EFULL;
    std::unordered_set<ShareKey, ShareKeyHash> pending(fresh.begin(), fresh.end());  // (may throw: nothing has changed yet)
    try {
        for (const ShareKey& k : fresh) set.keys.insert(k);
    } catch (...) {  // out of memory half way: the set goes back to what it was
        for (const ShareKey& k : fresh) set.keys.erase(k);
        throw;
    }
    // nothing below allocates: the batch's first occurrence of a fresh hash is the unflagged one
    for (size_t i = 0; i < n; ++i) {
        if (!share_eligible(v[i].status)) continue;
        ShareKey k;
        std::memcpy(k.data(), v[i].hash, k.size());
        if (!pending.erase(k)) v[i].status |= BM_SUBMIT_DUPLICATE;
    }
    recorded = fresh.size();
    set.count += recorded;
    return BM_OK;
}

}  // namespace host
}  // namespace bm
