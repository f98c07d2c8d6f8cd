// bm_ledger_host.hpp -- what a bm_ledger_t is (include/btcminer.h has the
// semantics): shared by bm_ledger.cpp (the entry points and the CPU ledger: plain
// C++, no HIP, also compiled into tools/ledger_check.cpp's program) and by
// bm_aux.hip (the device ledger: bm_ledger_create and the operations a device ledger
// reaches through `ops`, so that the plain unit links without the HIP runtime).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "bm_ledger_args.hpp"
#include "bm_share_set_host.hpp"

namespace bm {

// The operations of a device ledger (bm_aux.hip).  The arguments are checked.
struct LedgerDeviceOps {
    int (*verify_jobs)(bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                       const bm_pool_session_t* sessions, size_t nsessions, const uint32_t* accounts,
                       const uint64_t* weights, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                       bm_ledger_result_t* out);
    int (*read)(bm_ledger_t* ledger, size_t first, size_t count, bool drain, bm_ledger_row_t* out);
    int (*clear)(bm_ledger_t* ledger);
    void (*destroy)(bm_ledger_t* ledger);  // the device's memory; the caller deletes the object
};

}  // namespace bm

struct bm_ledger {
    size_t rows = 0;
    uint32_t peel = bm::kLedgerDefaultPeel;
    // a CPU ledger (ops == nullptr)
    std::vector<bm_ledger_row_t> table;
    // a device ledger, on the first device of ctx
    const bm::LedgerDeviceOps* ops = nullptr;
    bm_ctx* ctx = nullptr;
    uint64_t* d_rows = nullptr;  // rows entries of eight words
    bool poisoned = false;       // a call failed after its credit kernel's launch: until the next clear
};

namespace bm {
namespace host {

inline bm_ledger_row_t ledger_empty_row() {
    bm_ledger_row_t r;
    std::memset(&r, 0, sizeof r);
    r.best = kLedgerNoBest;
    return r;
}

// What bm_ledger_verify_jobs refuses, for either kind of ledger.
inline int ledger_check(const bm_ledger_t* ledger, const bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                        const bm_pool_session_t* sessions, size_t nsessions, const uint32_t* accounts,
                        const bm_jobs_submit_t* submits, size_t n, const bm_job_verdict_t* verdicts,
                        const bm_ledger_result_t* out) {
    if (!ledger || !out) return BM_EINVAL;
    const int rc = jobs_verify_check(jobs, njobs, sessions, nsessions, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    if (set) {  // both on the CPU, or both on one context
        if ((set->ops != nullptr) != (ledger->ops != nullptr)) return BM_EINVAL;
        if (ledger->ops && set->ctx != ledger->ctx) return BM_EINVAL;
    }
    if (accounts) {
        for (size_t s = 0; s < nsessions; ++s)
            if (accounts[s] >= ledger->rows) return BM_EINVAL;
    } else if (nsessions > ledger->rows) {
        return BM_EINVAL;
    }
    return BM_OK;
}

// A submission's hash[0..7] as a big-endian integer.
inline uint64_t ledger_hash_top(const bm_job_verdict_t& v) {
    uint64_t t = 0;
    for (int k = 0; k < 8; ++k) t = (t << 8) | v.hash[k];
    return t;
}

// One submission's credit to the row of its account.
inline void ledger_credit_row(bm_ledger_row_t& row, const bm_job_verdict_t& v, uint64_t weight) {
    uint64_t* w = reinterpret_cast<uint64_t*>(&row);
    const int cls = ledger_class(v.status);
    w[cls] += 1;
    if (cls != kLedgerAccepted) return;
    if (v.status & BM_SUBMIT_BLOCK) row.blocks += 1;
    row.work += weight;
    const uint64_t top = ledger_hash_top(v);
    if (top < row.best) row.best = top;
}

// A call's totals over all rows from its final verdicts: the seven control words the
// credit kernel sums, and `unattributed`.
struct LedgerTotals {
    uint64_t word[kLedgerCtlWords] = {};
    uint64_t unattributed = 0;
};

inline void ledger_totals(const bm_jobs_submit_t* submits, const bm_job_verdict_t* v, size_t n, size_t nsessions,
                          const uint64_t* weights, LedgerTotals& t) {
    t = LedgerTotals();
    for (size_t i = 0; i < n; ++i) {
        const uint32_t s = submits[i].session;
        if (s >= nsessions) {
            ++t.unattributed;
            continue;
        }
        const int cls = ledger_class(v[i].status);
        ++t.word[cls];
        if (cls != kLedgerAccepted) continue;
        if (v[i].status & BM_SUBMIT_BLOCK) ++t.word[kLedgerBlocks];
        t.word[kLedgerWork] += weights ? weights[s] : 1ull;
    }
}

// *out from a share-set result (or a plain one widened to it) and the totals.
inline void ledger_result(const bm_share_set_result_t& r, const LedgerTotals& t, bm_ledger_result_t& out) {
    std::memset(&out, 0, sizeof out);
    out.n = r.n, out.shares = r.shares, out.blocks = r.blocks, out.invalid = r.invalid, out.ntime = r.ntime;
    out.duplicates = r.duplicates, out.recorded = r.recorded, out.count = r.count;
    out.credited = t.word[kLedgerAccepted];
    out.unattributed = t.unattributed;
    out.work = t.word[kLedgerWork];
}

}  // namespace host
}  // namespace bm
