// bm_sessions_host.hpp -- what a bm_sessions_t is (include/btcminer.h has the
// semantics): shared by bm_sessions.cpp (the entry points and the CPU table: plain
// C++, no HIP, also compiled into tools/sessions_check.cpp's program) and by
// bm_aux.hip (the device table: bm_sessions_create and the operations a device table
// reaches through `ops`, so that the plain unit links without the HIP runtime).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "bm_ledger_host.hpp"
#include "bm_sessions_args.hpp"

namespace bm {

// One slot of a bm_sessions_set call after the host's part: the index is below the
// capacity and appears once, the target is T(weight) (zero for a closed slot).
struct SessionSetRecord {
    uint32_t slot;
    uint32_t account;
    uint64_t weight;
    bm_pool_session_t session;
};
static_assert(sizeof(SessionSetRecord) == 4 * kSessionSetWords, "the staged record of bm_sessions_set");

// The operations of a device table (bm_aux.hip).  The arguments are checked.
struct SessionsDeviceOps {
    // the scatter of k records and their fresh states; the caller updates the mirror and the count
    int (*set)(bm_sessions_t* table, const SessionSetRecord* recs, size_t k, uint64_t now_ms);
    int (*states)(bm_sessions_t* table, size_t first, size_t count, bm_session_state_t* out);
    int (*verify_jobs)(bm_sessions_t* table, bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs,
                       size_t njobs, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                       bm_ledger_result_t* out);
    // the two passes; on BM_OK `changes` is sorted and checked, and the caller applies it to the mirror
    int (*retarget)(bm_sessions_t* table, const SessionsRetargetArgs& A, bm_vardiff_change_t* changes, size_t cap,
                    bm_vardiff_result_t* out);
    int (*clear)(bm_sessions_t* table);
    void (*destroy)(bm_sessions_t* table);  // the device's memory; the caller deletes the object
};

}  // namespace bm

struct bm_sessions {
    size_t capacity = 0;
    uint64_t count = 0;
    // the three arrays the pool calls take, `capacity` entries each: the CPU table, or a device table's mirror
    std::vector<bm_pool_session_t> sessions;
    std::vector<uint32_t> accounts;
    std::vector<uint64_t> weights;
    uint32_t account_bound = 0;  // no account set since the last clear is above it
    // a CPU table (ops == nullptr)
    std::vector<bm_session_state_t> state;
    // a device table, on the first device of ctx
    const bm::SessionsDeviceOps* ops = nullptr;
    bm_ctx* ctx = nullptr;
    uint32_t* d_sessions = nullptr;  // capacity entries of ten words
    uint32_t* d_accounts = nullptr;
    uint64_t* d_weights = nullptr;
    uint64_t* d_state = nullptr;     // capacity entries of four words
    bool poisoned = false;           // a call failed after a kernel that writes the table was launched: until the next clear
};

namespace bm {
namespace host {

// Every account of a slot below count is a row of the ledger.
inline bool sessions_accounts_fit(const bm_sessions& t, size_t rows) {
    if ((size_t)t.account_bound < rows) return true;
    for (size_t s = 0; s < t.count; ++s)
        if (t.accounts[s] >= rows) return false;
    return true;
}

// What bm_sessions_verify_jobs refuses, for either kind of table.
inline int sessions_verify_check(const bm_sessions* t, const bm_ledger_t* ledger, const bm_share_set_t* set,
                                 const bm_pool_job_t* jobs, size_t njobs, const bm_jobs_submit_t* submits, size_t n,
                                 const bm_job_verdict_t* verdicts, const bm_ledger_result_t* out) {
    if (!t || !out) return BM_EINVAL;
    const int rc = jobs_verify_check(jobs, njobs, t->sessions.data(), (size_t)t->count, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    const bool device = t->ops != nullptr;
    if (ledger && ((ledger->ops != nullptr) != device || (device && ledger->ctx != t->ctx))) return BM_EINVAL;
    if (set && ((set->ops != nullptr) != device || (device && set->ctx != t->ctx))) return BM_EINVAL;
    if (ledger && !sessions_accounts_fit(*t, ledger->rows)) return BM_EINVAL;
    return BM_OK;
}

inline int vardiff_policy_check(const bm_vardiff_policy_t* p) {
    if (!p) return BM_EINVAL;
    if (p->target_ms < 1 || p->target_ms > 0xFFFFFFFFull) return BM_EINVAL;
    if (p->min_difficulty_fx < 1 || p->min_difficulty_fx > p->max_difficulty_fx) return BM_EINVAL;
    if (p->max_up < 1 || p->max_down < 1 || p->band_permille > 1000) return BM_EINVAL;
    return BM_OK;
}

inline SessionsRetargetArgs vardiff_args(const bm_vardiff_policy_t& p, uint64_t now_ms, uint64_t count, size_t cap) {
    SessionsRetargetArgs A;
    std::memset(&A, 0, sizeof A);
    A.now_ms = now_ms;
    A.target_ms = p.target_ms, A.window_ms = p.window_ms;
    A.min_fx = p.min_difficulty_fx, A.max_fx = p.max_difficulty_fx;
    A.burst = p.burst, A.band_permille = p.band_permille, A.max_up = p.max_up, A.max_down = p.max_down;
    A.count = (uint32_t)count;
    A.cap = (uint32_t)(cap < count ? cap : count);
    return A;
}

// A checked change list applied to the three arrays.
inline void sessions_apply_changes(bm_sessions& t, const bm_vardiff_change_t* changes, size_t k) {
    for (size_t i = 0; i < k; ++i) {
        const bm_vardiff_change_t& c = changes[i];
        t.weights[c.session] = c.new_fx;
        std::memcpy(t.sessions[c.session].target, c.target, 32);
    }
}

}  // namespace host
}  // namespace bm
