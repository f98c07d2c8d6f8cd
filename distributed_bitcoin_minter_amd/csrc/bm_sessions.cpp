// bm_sessions.cpp -- the entry points of the session table that need no GPU
// (include/btcminer.h): bm_sessions_create_cpu, bm_sessions_destroy, bm_sessions_clear,
// bm_sessions_count, bm_sessions_set, bm_sessions_get, bm_sessions_verify_jobs and
// bm_sessions_retarget, which are the specification on a CPU table and hand a device
// table to bm_aux.hip's operations (bm_sessions_host.hpp).  The CPU table's vardiff
// rule is written with a 128-bit type, apart from the multiword code the kernel and the
// device table's checks use (bm_sessions_args.hpp).  Plain C++: no HIP in here.
#include <algorithm>
#include <new>
#include <vector>

#include "bm_sessions_host.hpp"

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

using u128 = unsigned __int128;

// Rules 1 to 6 on the CPU table: is the open slot evaluated, and its new difficulty
// (`old` where it is unchanged).
bool evaluate_cpu(const bm_vardiff_policy_t& p, uint64_t now_ms, const bm_session_state_t& s, uint64_t& nw) {
    const uint64_t old = s.difficulty_fx;
    const uint64_t elapsed = now_ms >= s.since_ms ? now_ms - s.since_ms : 0;
    nw = old;
    if (!(elapsed >= p.window_ms || (p.burst != 0 && s.accepted >= p.burst))) return false;
    const u128 D = std::max<uint64_t>(elapsed, 1);
    const u128 N = (u128)std::min<uint64_t>(s.accepted, 0xFFFFFFFFull) * p.target_ms;
    // old * N is below 2^128; an ideal of 2^64 or more is cut by the upper clamp, which is below 2^64
    const u128 ideal = (u128)old * N / D;
    const u128 lo = std::max<uint64_t>(1, old / p.max_down);
    const u128 hi = std::min<u128>((u128)old * p.max_up, ~0ull);
    u128 v = std::min(std::max(ideal, lo), hi);
    v = std::min<u128>(std::max<u128>(v, p.min_difficulty_fx), p.max_difficulty_fx);
    const uint64_t cand = (uint64_t)v;
    const u128 diff = cand > old ? cand - old : old - cand;
    if (diff * 1000 > (u128)old * p.band_permille) nw = cand;
    return true;
}

// The decide pass on the CPU table: the counts and the change list, ascending; nothing changes.
void decide_cpu(const bm_sessions_t& t, const bm_vardiff_policy_t& p, uint64_t now_ms,
                std::vector<bm_vardiff_change_t>& list, std::vector<uint32_t>& evaluated, bm_vardiff_result_t& r) {
    std::memset(&r, 0, sizeof r);
    for (size_t s = 0; s < t.count; ++s) {
        const bm_session_state_t& st = t.state[s];
        if (st.difficulty_fx == 0) continue;
        ++r.open;
        uint64_t nw;
        if (!evaluate_cpu(p, now_ms, st, nw)) continue;
        ++r.evaluated;
        evaluated.push_back((uint32_t)s);
        if (nw == st.difficulty_fx) continue;
        ++r.changed;
        ++(nw > st.difficulty_fx ? r.raised : r.lowered);
        bm_vardiff_change_t c;
        std::memset(&c, 0, sizeof c);
        c.session = (uint32_t)s;
        c.old_fx = st.difficulty_fx, c.new_fx = nw;
        bm_target_from_difficulty_fx(nw, c.target);
        list.push_back(c);
    }
}

// The specification of bm_sessions_verify_jobs: bm_ledger_verify_jobs's CPU path over
// the table's arrays (the rows only with a ledger), then the tally.  Everything that
// can fail comes before the first change.
int verify_cpu(bm_sessions_t* t, bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
               const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts, bm_ledger_result_t* out) {
    const bm_pool_session_t* sessions = t->sessions.data();
    const size_t nsessions = (size_t)t->count;
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
    host::LedgerTotals tot;
    host::ledger_totals(submits, v.data(), n, nsessions, t->weights.data(), tot);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t s = submits[i].session;
        if (s >= nsessions) continue;
        if (ledger) host::ledger_credit_row(ledger->table[t->accounts[s]], v[i], t->weights[s]);
        if (ledger_class(v[i].status) == kLedgerAccepted) t->state[s].accepted += 1;
    }
    std::memcpy(verdicts, v.data(), n * sizeof(bm_job_verdict_t));
    host::ledger_result(r, tot, *out);
    return BM_OK;
}

// bm_sessions_set's host part: the checks, later entries win, the targets.
int set_records(const bm_sessions_t* t, const uint32_t* index, size_t k, const bm_session_init_t* init,
                std::vector<SessionSetRecord>& recs) {
    if (k > t->capacity && !index) return BM_EINVAL;
    for (size_t j = 0; index && j < k; ++j)
        if (index[j] >= t->capacity) return BM_EINVAL;
    std::vector<uint32_t> order(k);
    for (size_t j = 0; j < k; ++j) order[j] = (uint32_t)j;
    if (index) {  // by slot, entries of one slot in the caller's order: the last of a run is the one that counts
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return index[a] < index[b]; });
    }
    recs.reserve(k);
    for (size_t i = 0; i < k; ++i) {
        const uint32_t j = order[i];
        const uint32_t slot = index ? index[j] : j;
        if (i + 1 < k && index && index[order[i + 1]] == slot) continue;
        SessionSetRecord rec;
        std::memset(&rec, 0, sizeof rec);
        rec.slot = slot;
        rec.account = init[j].account;
        rec.weight = init[j].difficulty_fx;
        std::memcpy(rec.session.extranonce1, init[j].extranonce1, 8);
        if (rec.weight) bm_target_from_difficulty_fx(rec.weight, rec.session.target);
        recs.push_back(rec);
    }
    return BM_OK;
}

}  // namespace
}  // namespace bm

extern "C" {

int bm_sessions_create_cpu(size_t capacity, bm_sessions_t** out) {
    if (!out || capacity == 0 || capacity > BM_MAX_POOL_SESSIONS) return BM_EINVAL;
    return bm::guarded([&] {
        bm_sessions_t* t = new (std::nothrow) bm_sessions;
        if (!t) return BM_ENOMEM;
        t->capacity = capacity;
        try {
            t->sessions.assign(capacity, bm_pool_session_t());
            t->accounts.assign(capacity, 0);
            t->weights.assign(capacity, 0);
            t->state.assign(capacity, bm_session_state_t());
        } catch (...) {
            delete t;
            throw;
        }
        *out = t;
        return BM_OK;
    });
}

void bm_sessions_destroy(bm_sessions_t* table) {
    if (!table) return;
    if (table->ops) table->ops->destroy(table);
    delete table;
}

int bm_sessions_clear(bm_sessions_t* table) {
    if (!table) return BM_EINVAL;
    if (table->ops) {
        const int rc = table->ops->clear(table);
        if (rc != BM_OK) return rc;
    }
    std::fill(table->sessions.begin(), table->sessions.end(), bm_pool_session_t());
    std::fill(table->accounts.begin(), table->accounts.end(), 0u);
    std::fill(table->weights.begin(), table->weights.end(), 0ull);
    std::fill(table->state.begin(), table->state.end(), bm_session_state_t());
    table->count = 0;
    table->account_bound = 0;
    table->poisoned = false;
    return BM_OK;
}

int bm_sessions_count(const bm_sessions_t* table, uint64_t* count, uint64_t* capacity) {
    if (!table || (!count && !capacity)) return BM_EINVAL;
    if (count) *count = table->count;
    if (capacity) *capacity = table->capacity;
    return BM_OK;
}

int bm_sessions_set(bm_sessions_t* table, const uint32_t* index, size_t k, const bm_session_init_t* init,
                    uint64_t now_ms) {
    if (!table || (k && !init)) return BM_EINVAL;
    if (table->poisoned) return BM_EINTERNAL;
    return bm::guarded([&] {
        std::vector<bm::SessionSetRecord> recs;
        const int rc = bm::set_records(table, index, k, init, recs);
        if (rc != BM_OK) return rc;
        if (recs.empty()) return (int)BM_OK;
        if (table->ops) {
            const int rd = table->ops->set(table, recs.data(), recs.size(), now_ms);
            if (rd != BM_OK) return rd;
        }
        for (const bm::SessionSetRecord& r : recs) {  // nothing below fails
            table->sessions[r.slot] = r.session;
            table->accounts[r.slot] = r.account;
            table->weights[r.slot] = r.weight;
            if (!table->ops) table->state[r.slot] = bm_session_state_t{r.weight, now_ms, 0, 0};
            if (r.account > table->account_bound) table->account_bound = r.account;
            if ((uint64_t)r.slot + 1 > table->count) table->count = (uint64_t)r.slot + 1;
        }
        return (int)BM_OK;
    });
}

int bm_sessions_get(bm_sessions_t* table, size_t first, size_t count, bm_pool_session_t* sessions, uint32_t* accounts,
                    uint64_t* weights, bm_session_state_t* state) {
    if (!table || first > table->capacity || count > table->capacity - first) return BM_EINVAL;
    if (table->poisoned) return BM_EINTERNAL;
    if (count == 0) return BM_OK;
    return bm::guarded([&] {
        if (state && table->ops) {  // the caller's arrays are written last
            std::vector<bm_session_state_t> tmp(count);
            const int rc = table->ops->states(table, first, count, tmp.data());
            if (rc != BM_OK) return rc;
            std::memcpy(state, tmp.data(), count * sizeof(bm_session_state_t));
        } else if (state) {
            std::memcpy(state, table->state.data() + first, count * sizeof(bm_session_state_t));
        }
        if (sessions) std::memcpy(sessions, table->sessions.data() + first, count * sizeof(bm_pool_session_t));
        if (accounts) std::memcpy(accounts, table->accounts.data() + first, count * sizeof(uint32_t));
        if (weights) std::memcpy(weights, table->weights.data() + first, count * sizeof(uint64_t));
        return (int)BM_OK;
    });
}

int bm_sessions_verify_jobs(bm_sessions_t* table, bm_ledger_t* ledger, bm_share_set_t* set, const bm_pool_job_t* jobs,
                            size_t njobs, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                            bm_ledger_result_t* out) {
    const int rc = bm::host::sessions_verify_check(table, ledger, set, jobs, njobs, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    if (table->poisoned) return BM_EINTERNAL;
    if (n == 0) {  // legal, and changes nothing
        std::memset(out, 0, sizeof *out);
        out->count = set ? set->count : 0;
        return BM_OK;
    }
    if (table->ops) return table->ops->verify_jobs(table, ledger, set, jobs, njobs, submits, n, verdicts, out);
    return bm::guarded([&] { return bm::verify_cpu(table, ledger, set, jobs, njobs, submits, n, verdicts, out); });
}

int bm_sessions_retarget(bm_sessions_t* table, uint64_t now_ms, const bm_vardiff_policy_t* policy,
                         bm_vardiff_change_t* changes, size_t cap, bm_vardiff_result_t* out) {
    if (!table || !out || (cap && !changes)) return BM_EINVAL;
    const int rc = bm::host::vardiff_policy_check(policy);
    if (rc != BM_OK) return rc;
    if (table->poisoned) return BM_EINTERNAL;
    return bm::guarded([&] {
        bm_vardiff_result_t r;
        std::vector<bm_vardiff_change_t> list;
        if (table->ops) {
            const bm::SessionsRetargetArgs A = bm::host::vardiff_args(*policy, now_ms, table->count, cap);
            list.resize(A.cap);
            const int rd = table->ops->retarget(table, A, list.data(), A.cap, &r);
            if (rd == BM_EFULL) *out = r;
            if (rd != BM_OK) return rd;
            list.resize((size_t)r.changed);
        } else {
            std::vector<uint32_t> evaluated;
            bm::decide_cpu(*table, *policy, now_ms, list, evaluated, r);
            if (r.changed > cap) {
                *out = r;
                return (int)BM_EFULL;
            }
            for (const uint32_t s : evaluated) table->state[s].since_ms = now_ms, table->state[s].accepted = 0;
            for (const bm_vardiff_change_t& c : list) {
                table->state[c.session].difficulty_fx = c.new_fx;
                table->state[c.session].retargets += 1;
            }
        }
        bm::host::sessions_apply_changes(*table, list.data(), list.size());
        if (!list.empty()) std::memcpy(changes, list.data(), list.size() * sizeof(bm_vardiff_change_t));
        *out = r;
        return (int)BM_OK;
    });
}

}  // extern "C"
