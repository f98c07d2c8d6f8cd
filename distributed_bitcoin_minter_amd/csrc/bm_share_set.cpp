// bm_share_set.cpp -- the entry points of the share set that need no GPU
// (include/btcminer.h): bm_share_set_create_cpu, bm_share_set_destroy,
// bm_share_set_clear, bm_share_set_count, bm_share_set_verify and
// bm_share_set_verify_jobs, which are the specification on a CPU set and hand a
// device set to bm_aux.hip's operations (bm_share_set_host.hpp).  Plain C++: no HIP
// in here.
#include <new>
#include <vector>

#include "bm_share_set_host.hpp"

#define BM_SHARE_TRY(call)            \
    do {                              \
        const int rc_ = (call);       \
        if (rc_ != BM_OK) return rc_; \
    } while (0)

namespace bm {
namespace {

// The specification: one submission at a time, in the caller's order, over a hash
// set of 32-byte arrays (host::share_set_apply).  one(i, v): the plain verdict of
// submission i, bm_pool_verify_cpu's or bm_jobs_verify_cpu's.
template <class One>
int verify_cpu(bm_share_set_t* set, size_t n, One&& one, bm_job_verdict_t* verdicts, bm_share_set_result_t* out) {
    std::vector<bm_job_verdict_t> v(n);
    for (size_t i = 0; i < n; ++i) one(i, v[i]);
    uint64_t recorded = 0;
    BM_SHARE_TRY(host::share_set_apply(*set, v.data(), n, recorded));
    bm_share_set_result_t r;
    host::share_set_count(v.data(), n, r);
    r.recorded = recorded;
    r.count = set->count;
    std::memcpy(verdicts, v.data(), n * sizeof(bm_job_verdict_t));
    *out = r;
    return BM_OK;
}

template <class F>
int guarded(F&& f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return BM_ENOMEM;
    } catch (...) {
        return BM_EINTERNAL;
    }
}

}  // namespace
}  // namespace bm

extern "C" {

int bm_share_set_create_cpu(size_t capacity, bm_share_set_t** out) {
    if (!out || capacity == 0 || capacity > BM_MAX_SHARE_SET) return BM_EINVAL;
    bm_share_set_t* set = new (std::nothrow) bm_share_set;
    if (!set) return BM_ENOMEM;
    set->capacity = capacity;
    *out = set;
    return BM_OK;
}

void bm_share_set_destroy(bm_share_set_t* set) {
    if (!set) return;
    if (set->ops) set->ops->destroy(set);
    delete set;
}

int bm_share_set_clear(bm_share_set_t* set) {
    if (!set) return BM_EINVAL;
    if (set->ops) return set->ops->clear(set);
    set->keys.clear();
    set->count = 0;
    return BM_OK;
}

int bm_share_set_count(const bm_share_set_t* set, uint64_t* count, uint64_t* capacity) {
    if (!set) return BM_EINVAL;
    if (count) *count = set->count;
    if (capacity) *capacity = set->capacity;
    return BM_OK;
}

int bm_share_set_verify(bm_share_set_t* set, const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                        const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                        bm_job_verdict_t* verdicts, bm_share_set_result_t* out) {
    const int rc = bm::host::share_set_check(set, job, sessions, nsessions, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    if (n == 0) {  // legal, and changes nothing
        std::memset(out, 0, sizeof *out);
        out->count = set->count;
        return BM_OK;
    }
    if (set->ops) return set->ops->verify(set, job, sessions, nsessions, submits, n, ntime_lo, ntime_hi, verdicts, out);
    return bm::guarded([&] {
        uint8_t bt[32];
        const uint8_t* block_target = bm::host::target_from_bits(job->nbits, bt) ? bt : nullptr;
        return bm::verify_cpu(
            set, n,
            [&](size_t i, bm_job_verdict_t& v) {
                bm::host::pool_verify_one(job, sessions, nsessions, block_target, ntime_lo, ntime_hi, submits[i], v);
            },
            verdicts, out);
    });
}

int bm_share_set_verify_jobs(bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                             const bm_pool_session_t* sessions, size_t nsessions, const bm_jobs_submit_t* submits,
                             size_t n, bm_job_verdict_t* verdicts, bm_share_set_result_t* out) {
    const int rc = bm::host::share_set_jobs_check(set, jobs, njobs, sessions, nsessions, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    if (n == 0) {  // legal, and changes nothing
        std::memset(out, 0, sizeof *out);
        out->count = set->count;
        return BM_OK;
    }
    if (set->ops) return set->ops->verify_jobs(set, jobs, njobs, sessions, nsessions, submits, n, verdicts, out);
    return bm::guarded([&] {
        return bm::verify_cpu(
            set, n,
            [&](size_t i, bm_job_verdict_t& v) {
                bm::host::jobs_verify_one(jobs, njobs, sessions, nsessions, submits[i], v);
            },
            verdicts, out);
    });
}

}  // extern "C"
