// bm_sessions.hpp -- the kernels of a device session table (include/btcminer.h has the
// semantics; bm_aux.hip the host part).  The table is four arrays of `capacity` slots:
// sessions (ten words: extranonce1, target), accounts, weights -- the layouts
// jobs_verify_kernel and ledger_credit_kernel read -- and states (four 64-bit words).
//
// sessions_set_kernel scatters the staged records of bm_sessions_set, one lane per
// record.  The host has resolved repeated indices: no two lanes write one slot.
//
// sessions_tally_kernel runs where ledger_credit_kernel runs, on the same stream, one
// lane per staged record: a lane whose session is below the table's count and whose
// final verdict is of class accepted adds one to its slot's `accepted`, a no-return
// 64-bit atomicAdd per lane (vardiff keeps a session at a few shares per window, so the
// scatter rarely contends), and the wave adds its popcount to the call's control word,
// which the host compares with the verdicts it holds.
//
// sessions_retarget_kernel takes one lane per slot below count and runs the rule of
// bm_sessions_retarget in 64-bit words (bm_sessions_args.hpp).  The decide pass (A.apply
// = 0) only reads the table: a wave counts its open, evaluated, changed, raised and
// lowered lanes with ballots, lane 0 adds the non-zero counts to the control words, and
// the add to `changed` returns the wave's base in the change list, where each changed
// lane writes its entry at base + its rank among the wave's changed lanes, if that is
// below A.cap.  The list is unordered between waves: the host sorts it.  The apply pass
// (A.apply = 1), launched once the host has accepted the list, recomputes the same
// decisions from the same inputs and rewrites the slots.  Only changed lanes run the
// 256-bit by 64-bit division.
//
// Nothing spins, retries or waits on another lane; every loop has a fixed trip count.
// No lane returns before the wave's ballots.  All stores are atomics or ordinary vector
// stores.  No LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bm_ledger_args.hpp"
#include "bm_sessions_args.hpp"

namespace bm {

constexpr int kTallyVerdictWords = 10;  // bm_job_verdict_t: eight words of hash, status, reserved
constexpr int kTallySubmitWords = 8;    // a staged bm_jobs_submit_t: session in word 5, original index in word 6

// T(d) as the eight words of a target in memory: most significant byte first.
__device__ inline void sessions_target_words(uint64_t d, uint32_t w[8]) {
    uint64_t q[4];
    target_words_fx(d, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[2 * i] = __builtin_bswap32((uint32_t)(q[i] >> 32));
        w[2 * i + 1] = __builtin_bswap32((uint32_t)q[i]);
    }
}

__global__ __launch_bounds__(kSessionsThreads) void sessions_set_kernel(const uint32_t n, const uint32_t capacity,
                                                                        const uint64_t now_ms,
                                                                        const uint32_t* __restrict__ recs,
                                                                        uint32_t* __restrict__ sessions,
                                                                        uint32_t* __restrict__ accounts,
                                                                        uint64_t* __restrict__ weights,
                                                                        uint64_t* __restrict__ state) {
    const uint32_t k = blockIdx.x * kSessionsThreads + threadIdx.x;
    if (k >= n) return;
    const uint32_t* rec = recs + (size_t)kSessionSetWords * k;
    const uint32_t slot = rec[0];
    if (slot >= capacity) return;  // the host has checked every index; never out of the table
    const uint64_t weight = ((uint64_t)rec[3] << 32) | rec[2];
    uint32_t* ses = sessions + (size_t)kSessionSlotWords * slot;
#pragma unroll
    for (int i = 0; i < kSessionSlotWords; ++i) ses[i] = rec[4 + i];
    accounts[slot] = rec[1];
    weights[slot] = weight;
    uint64_t* st = state + (size_t)kSessionStateWords * slot;
    st[kStateDifficulty] = weight;
    st[kStateSince] = now_ms;
    st[kStateAccepted] = 0;
    st[kStateRetargets] = 0;
}

__global__ __launch_bounds__(kSessionsThreads) void sessions_tally_kernel(const SessionsTallyArgs A,
                                                                          const uint32_t* __restrict__ submits,
                                                                          const uint32_t* __restrict__ verdicts,
                                                                          unsigned long long* __restrict__ state,
                                                                          unsigned long long* __restrict__ ctl) {
    const uint32_t k = blockIdx.x * kSessionsThreads + threadIdx.x;
    uint32_t session = 0xFFFFFFFFu, index = 0xFFFFFFFFu;
    if (k < A.n) {
        const uint32_t* rec = submits + (size_t)kTallySubmitWords * k;
        session = rec[5];
        index = rec[6];
    }
    bool accepted = false;
    if (session < A.nsessions && index < A.n)
        accepted = ledger_class(verdicts[(size_t)kTallyVerdictWords * index + 8]) == kLedgerAccepted;
    if (accepted) atomicAdd(&state[(size_t)kSessionStateWords * session + kStateAccepted], 1ull);
    const unsigned long long total = (unsigned long long)__popcll(__ballot(accepted));
    if (threadIdx.x == 0 && total != 0) atomicAdd(ctl, total);
}

__global__ __launch_bounds__(kSessionsThreads) void sessions_retarget_kernel(const SessionsRetargetArgs A,
                                                                             uint32_t* __restrict__ sessions,
                                                                             uint64_t* __restrict__ weights,
                                                                             uint64_t* __restrict__ state,
                                                                             uint32_t* __restrict__ list,
                                                                             unsigned long long* __restrict__ ctl) {
    const uint32_t lane = threadIdx.x;
    const uint32_t s = blockIdx.x * kSessionsThreads + lane;
    uint64_t old = 0, since = 0, accepted = 0;
    uint64_t* st = state + (size_t)kSessionStateWords * (s < A.count ? s : 0);
    if (s < A.count) {
        old = st[kStateDifficulty];
        since = st[kStateSince];
        accepted = st[kStateAccepted];
    }
    const bool open = old != 0;
    const bool evaluated = open && vardiff_evaluated(A, since, accepted);
    uint64_t nw = old;
    if (evaluated) nw = vardiff_new(A, old, since, accepted);
    const bool changed = nw != old;
    const unsigned long long m_changed = __ballot(changed);

    if (!A.apply) {
        const unsigned long long c_open = (unsigned long long)__popcll(__ballot(open));
        const unsigned long long c_eval = (unsigned long long)__popcll(__ballot(evaluated));
        const unsigned long long c_up = (unsigned long long)__popcll(__ballot(changed && nw > old));
        const unsigned long long c_down = (unsigned long long)__popcll(__ballot(changed && nw < old));
        const unsigned long long c_changed = (unsigned long long)__popcll(m_changed);
        unsigned long long base = 0;
        if (lane == 0) {
            if (c_open) atomicAdd(&ctl[kRetargetOpen], c_open);
            if (c_eval) atomicAdd(&ctl[kRetargetEvaluated], c_eval);
            if (c_up) atomicAdd(&ctl[kRetargetRaised], c_up);
            if (c_down) atomicAdd(&ctl[kRetargetLowered], c_down);
            if (c_changed) base = atomicAdd(&ctl[kRetargetChanged], c_changed);
        }
        base = (unsigned long long)__shfl((long long)base, 0);
        if (changed) {
            const unsigned long long at = base + (unsigned long long)__popcll(m_changed & ((1ull << lane) - 1ull));
            if (at < (unsigned long long)A.cap) {
                uint32_t t[8];
                sessions_target_words(nw, t);
                uint32_t* e = list + (size_t)kSessionChangeWords * at;
                e[0] = s;
                e[1] = 0;
                e[2] = (uint32_t)old, e[3] = (uint32_t)(old >> 32);
                e[4] = (uint32_t)nw, e[5] = (uint32_t)(nw >> 32);
#pragma unroll
                for (int i = 0; i < 8; ++i) e[6 + i] = t[i];
            }
        }
        return;
    }

    if (evaluated) {
        st[kStateSince] = A.now_ms;
        st[kStateAccepted] = 0;
    }
    if (changed) {
        uint32_t t[8];
        sessions_target_words(nw, t);
        st[kStateDifficulty] = nw;
        st[kStateRetargets] += 1;
        weights[s] = nw;
        uint32_t* ses = sessions + (size_t)kSessionSlotWords * s;
#pragma unroll
        for (int i = 0; i < 8; ++i) ses[2 + i] = t[i];
    }
    const unsigned long long c_changed = (unsigned long long)__popcll(m_changed);
    if (lane == 0 && c_changed) atomicAdd(&ctl[kRetargetApplied], c_changed);
}

}  // namespace bm
