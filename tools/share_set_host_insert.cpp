// share_set_host_insert.cpp -- measurement only (tools/bench_share_set.py builds it
// into a shared object of its own): the library's CPU set step
// (csrc/bm_share_set_host.hpp, host::share_set_apply -- what bm_share_set_verify runs
// on a CPU set after hashing) over verdicts that bm_pool_verify_gpu returned, on the
// calling thread.  This is what a caller without a device set does after every call.
#include <new>

#include "bm_share_set_host.hpp"

extern "C" int bench_share_set_apply(bm_share_set_t* set, bm_job_verdict_t* verdicts, size_t n, uint64_t* recorded) {
    try {
        uint64_t r = 0;
        const int rc = bm::host::share_set_apply(*set, verdicts, n, r);
        if (rc == BM_OK) *recorded = r;
        return rc;
    } catch (const std::bad_alloc&) {
        return BM_ENOMEM;
    }
}
