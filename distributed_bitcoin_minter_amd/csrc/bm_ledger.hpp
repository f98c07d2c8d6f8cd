// bm_ledger.hpp -- the kernels of a device ledger: the per-account counters behind
// share accounting (include/btcminer.h has the semantics; bm_aux.hip the host part).
//
// ledger_credit_kernel runs after jobs_verify_kernel -- and, with a share set, after
// share_commit_kernel -- on the same stream, one lane per staged record, over what
// the call already has on the device: the staged record (its session, and its
// original index where the caller's record has `job`), the final verdict at that
// index (status, and the first two hash words), and the call's accounts[] and
// weights[] by session.  A lane whose session is known contributes to row
// accounts[session]: one to its class word (ledger_class), one to `blocks` when it
// is accepted with BM_SUBMIT_BLOCK, its weight to `work` and its hash's top 64 bits
// to the minimum `best` when it is accepted.  Every update is a 64-bit integer add or
// min, so the rows depend on the multiset of submissions only.
//
// A pool has many sessions per account, so the scatter contends.  Before any global
// atomic the wave combines, for up to A.rounds rounds (wave-uniform):
//   the row of the first pending lane is the round's; a ballot finds the lanes on it;
//   their class counts are popcounts of ballots, their work a wave sum, their best a
//   wave min; lanes 0..6 add the row's non-zero sums to its words 0..6 -- one
//   wave-instruction over 56 contiguous bytes -- and lane 7 issues the min; the lanes
//   retire.
// Lanes still pending after the last round issue their own atomics.  rounds = 0 is
// the plain per-lane form.
//
// The wave also adds its totals over all rows (six classes and work) to the call's
// control words, one atomic per wave per non-zero word: the host compares them with
// the totals of the verdicts it copied back.
//
// No atomic's return value is used.  Nothing spins, retries or waits on another
// lane; the loop is bounded by A.rounds <= 64 and ends early when no lane is pending.
// No lane returns early: the whole wave reaches every ballot.  All stores are
// atomics or ordinary vector stores.  No LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bm_ledger_args.hpp"

namespace bm {

constexpr int kLedgerVerdictWords = 10;  // bm_job_verdict_t: eight words of hash, status, reserved
constexpr int kLedgerSubmitWords = 8;    // a staged bm_jobs_submit_t: session in word 5, original index in word 6

__device__ inline uint64_t ledger_wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m);
    return v;
}

__device__ inline uint64_t ledger_wave_min(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, m);
        v = o < v ? o : v;
    }
    return v;
}

// The seven sums of the lanes of `on` (a wave-uniform set), selected by lane: lane
// k < 7 gets word k's.  cls, blk, work: the lane's class, block bit and credited work.
__device__ inline uint64_t ledger_sums(bool on, int cls, bool blk, uint64_t work, uint32_t lane) {
    const uint64_t wsum = ledger_wave_sum(on ? work : 0ull);
    uint64_t mine = wsum;  // lane 6's; the others' are replaced below
    const uint64_t c_acc = (uint64_t)__popcll(__ballot(on && cls == kLedgerAccepted));
    const uint64_t c_blk = (uint64_t)__popcll(__ballot(on && blk));
    const uint64_t c_abv = (uint64_t)__popcll(__ballot(on && cls == kLedgerAbove));
    const uint64_t c_nt = (uint64_t)__popcll(__ballot(on && cls == kLedgerNtime));
    const uint64_t c_dup = (uint64_t)__popcll(__ballot(on && cls == kLedgerDuplicates));
    const uint64_t c_inv = (uint64_t)__popcll(__ballot(on && cls == kLedgerInvalid));
    mine = lane == kLedgerAccepted ? c_acc : mine;
    mine = lane == kLedgerBlocks ? c_blk : mine;
    mine = lane == kLedgerAbove ? c_abv : mine;
    mine = lane == kLedgerNtime ? c_nt : mine;
    mine = lane == kLedgerDuplicates ? c_dup : mine;
    mine = lane == kLedgerInvalid ? c_inv : mine;
    return mine;
}

__global__ __launch_bounds__(kLedgerThreads) void ledger_credit_kernel(const LedgerArgs A,
                                                                       const uint32_t* __restrict__ submits,
                                                                       const uint32_t* __restrict__ verdicts,
                                                                       const uint32_t* __restrict__ accounts,
                                                                       const uint64_t* __restrict__ weights,
                                                                       unsigned long long* __restrict__ rows,
                                                                       unsigned long long* __restrict__ ctl) {
    const uint32_t lane = threadIdx.x;
    const uint32_t k = blockIdx.x * kLedgerThreads + lane;
    uint32_t session = 0xFFFFFFFFu, index = 0xFFFFFFFFu;
    if (k < A.n) {
        const uint32_t* rec = submits + (size_t)kLedgerSubmitWords * k;
        session = rec[5];
        index = rec[6];
    }
    bool known = session < A.nsessions && index < A.n;
    uint32_t row = 0;
    uint64_t weight = 0;
    if (known) {
        row = accounts[session];
        weight = weights[session];
    }
    known = known && row < A.rows;  // the host has checked every account; never out of the table
    int cls = -1;
    bool blk = false;
    uint64_t work = 0, best = kLedgerNoBest;
    if (known) {
        const uint32_t* v = verdicts + (size_t)kLedgerVerdictWords * index;
        const uint32_t status = v[8];
        cls = ledger_class(status);
        if (cls == kLedgerAccepted) {
            blk = (status & BM_SUBMIT_BLOCK) != 0;
            work = weight;
            // hash bytes 0..7, most significant first: the verdict holds them as little-endian words
            best = ((uint64_t)__builtin_bswap32(v[0]) << 32) | __builtin_bswap32(v[1]);
        }
    }

    // this call's totals, one atomic per wave per non-zero word
    {
        const uint64_t total = ledger_sums(known, cls, blk, work, lane);
        if (lane < (uint32_t)kLedgerCtlWords && total != 0) atomicAdd(&ctl[lane], (unsigned long long)total);
    }

    bool pending = known;
    for (uint32_t r = 0; r < A.rounds; ++r) {  // A.rounds <= 64
        const unsigned long long todo = __ballot(pending);
        if (todo == 0) break;  // wave-uniform
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t lrow = (uint32_t)__shfl((int)row, (int)leader);
        const bool on = pending && row == lrow;
        const uint64_t sum = ledger_sums(on, cls, blk, work, lane);
        const uint64_t low = ledger_wave_min(on ? best : kLedgerNoBest);
        unsigned long long* dst = rows + (size_t)kLedgerRowWords * lrow;
        if (lane < (uint32_t)kLedgerBest) {
            if (sum != 0) atomicAdd(&dst[lane], (unsigned long long)sum);
        } else if (lane == (uint32_t)kLedgerBest) {
            if (low != kLedgerNoBest) atomicMin(&dst[kLedgerBest], (unsigned long long)low);
        }
        pending = pending && !on;
    }
    if (pending) {
        unsigned long long* dst = rows + (size_t)kLedgerRowWords * row;
        atomicAdd(&dst[cls], 1ull);
        if (blk) atomicAdd(&dst[kLedgerBlocks], 1ull);
        if (work != 0) atomicAdd(&dst[kLedgerWork], (unsigned long long)work);
        if (best != kLedgerNoBest) atomicMin(&dst[kLedgerBest], (unsigned long long)best);
    }
}

// The empty-row pattern over whole rows: seven zeros and best = UINT64_MAX.
__global__ __launch_bounds__(kLedgerFillThreads) void ledger_fill_kernel(unsigned long long* __restrict__ words,
                                                                         const uint64_t nwords) {
    const uint64_t i = (uint64_t)blockIdx.x * kLedgerFillThreads + threadIdx.x;
    if (i < nwords) words[i] = (i % kLedgerRowWords) == (uint64_t)kLedgerBest ? kLedgerNoBest : 0ull;
}

}  // namespace bm
