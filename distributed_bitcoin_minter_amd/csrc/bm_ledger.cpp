// bm_ledger.cpp -- the entry points of the ledger that need no GPU
// (include/btcminer.h): bm_ledger_create_cpu, bm_ledger_destroy, bm_ledger_clear,
// bm_ledger_rows, bm_ledger_read, bm_ledger_drain, bm_ledger_set_peel and
// bm_ledger_verify_jobs, which are the specification on a CPU ledger and hand a
// device ledger to bm_aux.hip's operations (bm_ledger_host.hpp).  Plain C++: no HIP
// in here.
#include <new>
#include <vector>

#include "bm_ledger_host.hpp"

namespace bm {
namespace {

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

// The specification: the verdicts of bm_share_set_verify_jobs on a CPU set, or of
// bm_jobs_verify_cpu without one, then one submission at a time into its row.
// Everything that can fail comes before the first row changes.
int verify_cpu(bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
               const bm_pool_session_t* sessions, size_t nsessions, const uint32_t* accounts, const uint64_t* weights,
               const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts, bm_ledger_result_t* out) {
    std::vector<bm_job_verdict_t> v(n);
    bm_share_set_result_t r;
    std::memset(&r, 0, sizeof r);
    if (set) {
        const int rc = bm_share_set_verify_jobs(set, jobs, njobs, sessions, nsessions, submits, n, v.data(), &r);
        if (rc != BM_OK) return rc;
    } else {
        bm_pool_verify_result_t p;
        const int rc = bm_jobs_verify_cpu(jobs, njobs, sessions, nsessions, submits, n, v.data(), &p);
        if (rc != BM_OK) return rc;
        r.n = p.n, r.shares = p.shares, r.blocks = p.blocks, r.invalid = p.invalid, r.ntime = p.ntime;
    }
    host::LedgerTotals t;
    host::ledger_totals(submits, v.data(), n, nsessions, weights, t);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t s = submits[i].session;
        if (s >= nsessions) continue;
        host::ledger_credit_row(ledger->table[accounts ? accounts[s] : s], v[i], weights ? weights[s] : 1ull);
    }
    std::memcpy(verdicts, v.data(), n * sizeof(bm_job_verdict_t));
    host::ledger_result(r, t, *out);
    return BM_OK;
}

int read_rows(bm_ledger_t* ledger, size_t first, size_t count, bool drain, bm_ledger_row_t* out) {
    if (!ledger || first > ledger->rows || count > ledger->rows - first || (count && !out)) return BM_EINVAL;
    if (ledger->ops) return ledger->ops->read(ledger, first, count, drain, out);
    for (size_t i = 0; i < count; ++i) {
        out[i] = ledger->table[first + i];
        if (drain) ledger->table[first + i] = host::ledger_empty_row();
    }
    return BM_OK;
}

}  // namespace
}  // namespace bm

extern "C" {

int bm_ledger_create_cpu(size_t rows, bm_ledger_t** out) {
    if (!out || rows == 0 || rows > BM_MAX_LEDGER_ROWS) return BM_EINVAL;
    return bm::guarded([&] {
        bm_ledger_t* ledger = new (std::nothrow) bm_ledger;
        if (!ledger) return BM_ENOMEM;
        ledger->rows = rows;
        try {
            ledger->table.assign(rows, bm::host::ledger_empty_row());
        } catch (...) {
            delete ledger;
            throw;
        }
        *out = ledger;
        return BM_OK;
    });
}

void bm_ledger_destroy(bm_ledger_t* ledger) {
    if (!ledger) return;
    if (ledger->ops) ledger->ops->destroy(ledger);
    delete ledger;
}

int bm_ledger_clear(bm_ledger_t* ledger) {
    if (!ledger) return BM_EINVAL;
    if (ledger->ops) return ledger->ops->clear(ledger);
    for (bm_ledger_row_t& r : ledger->table) r = bm::host::ledger_empty_row();
    return BM_OK;
}

int bm_ledger_rows(const bm_ledger_t* ledger, uint64_t* rows) {
    if (!ledger || !rows) return BM_EINVAL;
    *rows = ledger->rows;
    return BM_OK;
}

int bm_ledger_read(bm_ledger_t* ledger, size_t first, size_t count, bm_ledger_row_t* out) {
    return bm::read_rows(ledger, first, count, false, out);
}

int bm_ledger_drain(bm_ledger_t* ledger, size_t first, size_t count, bm_ledger_row_t* out) {
    return bm::read_rows(ledger, first, count, true, out);
}

int bm_ledger_set_peel(bm_ledger_t* ledger, uint32_t rounds) {
    if (!ledger || rounds > bm::kLedgerMaxPeel) return BM_EINVAL;
    ledger->peel = rounds;
    return BM_OK;
}

int bm_ledger_verify_jobs(bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                          const bm_pool_session_t* sessions, size_t nsessions, const uint32_t* accounts,
                          const uint64_t* weights, const bm_jobs_submit_t* submits, size_t n,
                          bm_job_verdict_t* verdicts, bm_ledger_result_t* out) {
    const int rc = bm::host::ledger_check(ledger, set, jobs, njobs, sessions, nsessions, accounts, submits, n, verdicts,
                                          out);
    if (rc != BM_OK) return rc;
    if (n == 0) {  // legal, and changes nothing
        std::memset(out, 0, sizeof *out);
        out->count = set ? set->count : 0;
        return BM_OK;
    }
    if (ledger->ops)
        return ledger->ops->verify_jobs(ledger, set, jobs, njobs, sessions, nsessions, accounts, weights, submits, n,
                                        verdicts, out);
    return bm::guarded([&] {
        return bm::verify_cpu(ledger, set, jobs, njobs, sessions, nsessions, accounts, weights, submits, n, verdicts,
                              out);
    });
}

}  // extern "C"
