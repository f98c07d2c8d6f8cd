// bm_sessions_args.hpp -- what the session table's kernels (bm_sessions.hpp), their
// launcher (bm_aux.hip) and the CPU table (bm_sessions.cpp) agree on: the words of a
// slot's four records, the control words of a call, the kernels' argument blocks and
// the vardiff rule's arithmetic in multiword integers (no 128-bit type: device code
// has no 128-bit division).  Plain C++: no HIP in here.
#pragma once
#include <cstdint>

#include "bm_sha256.hpp"  // BM_HD
#include "btcminer.h"

namespace bm {

constexpr int kSessionsThreads = 64;      // one wave: the kernels' ballots cover the workgroup
constexpr int kSessionSlotWords = 10;         // bm_pool_session_t: two words of extranonce1, eight of target
constexpr int kSessionStateWords = 4;     // bm_session_state_t, 64-bit: difficulty_fx, since_ms, accepted, retargets
constexpr int kStateDifficulty = 0, kStateSince = 1, kStateAccepted = 2, kStateRetargets = 3;
constexpr int kSessionSetWords = 14;      // a staged record of bm_sessions_set, 32-bit: slot, account, weight, session
constexpr int kSessionChangeWords = 14;   // bm_vardiff_change_t, 32-bit: session, 0, old, new, eight of target
static_assert(sizeof(bm_pool_session_t) == 4 * kSessionSlotWords, "session layout");
static_assert(sizeof(bm_session_state_t) == 8 * kSessionStateWords, "state layout");
static_assert(sizeof(bm_vardiff_change_t) == 4 * kSessionChangeWords, "change layout");
static_assert(sizeof(bm_session_init_t) == 24, "init layout");

// The control words of bm_sessions_retarget (64-bit, zeroed before the decide pass):
// the five counts of bm_vardiff_result_t -- `changed` is the change list's cursor too --
// and the slots the apply pass rewrote.
constexpr int kRetargetOpen = 0, kRetargetEvaluated = 1, kRetargetChanged = 2, kRetargetRaised = 3,
              kRetargetLowered = 4, kRetargetApplied = 5;
constexpr int kRetargetCtlWords = 8;
// The tally's control word: the unit of padding behind the credit kernel's seven.
constexpr int kTallyCtlWord = 7;

// Kernel argument of sessions_tally_kernel, by value (SGPRs).
struct SessionsTallyArgs {
    uint32_t n;          // staged records
    uint32_t nsessions;  // slots below the table's count
};

// Kernel argument of sessions_retarget_kernel, by value (SGPRs).
struct SessionsRetargetArgs {
    uint64_t now_ms;
    uint64_t target_ms, window_ms, min_fx, max_fx;
    uint32_t burst, band_permille, max_up, max_down;
    uint32_t count;  // slots below the table's count
    uint32_t cap;    // entries the change list holds
    uint32_t apply;  // 0: decide (counts and the list; the table is only read), 1: apply (the table is rewritten)
    uint32_t pad;
};

// ---- exact unsigned arithmetic in 64-bit words ----

struct U128 {
    uint64_t hi, lo;
};

BM_HD inline U128 mul_64x64(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;  // below 3 * 2^32
    U128 r;
    r.lo = (mid << 32) | (uint32_t)p00;
    r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    return r;
}

BM_HD inline bool le_128(const U128& a, const U128& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo <= b.lo); }

// (hi * 2^64 + lo) / d and the remainder, for hi < d: the quotient fits 64 bits.  Restoring
// division, one bit per step, 64 steps.
BM_HD inline uint64_t div_128by64(uint64_t hi, uint64_t lo, uint64_t d, uint64_t* rem) {
    uint64_t r = hi, q = 0;
    for (int i = 63; i >= 0; --i) {
        const uint64_t carry = r >> 63;
        r = (r << 1) | ((lo >> i) & 1u);
        if (carry || r >= d) {  // with the carry the true remainder is r + 2^64 >= d, and r - d wraps to it
            r -= d;
            q |= 1ull << i;
        }
    }
    *rem = r;
    return q;
}

// floor(0xffff * 2^240 / d), d >= 1, as four 64-bit words, most significant first.
BM_HD inline void target_words_fx(uint64_t d, uint64_t q[4]) {
    uint64_t rem = 0;
    q[0] = div_128by64(rem, 0xffffull << 48, d, &rem);
    q[1] = div_128by64(rem, 0, d, &rem);
    q[2] = div_128by64(rem, 0, d, &rem);
    q[3] = div_128by64(rem, 0, d, &rem);
}

// Rule 2 of bm_sessions_retarget for an open slot: is it evaluated?
BM_HD inline bool vardiff_evaluated(const SessionsRetargetArgs& A, uint64_t since_ms, uint64_t accepted) {
    const uint64_t elapsed = A.now_ms >= since_ms ? A.now_ms - since_ms : 0;
    return elapsed >= A.window_ms || (A.burst != 0 && accepted >= A.burst);
}

// Rules 3 to 6 for an evaluated slot of difficulty `old` >= 1: the new difficulty, `old`
// itself where the slot is unchanged.
BM_HD inline uint64_t vardiff_new(const SessionsRetargetArgs& A, uint64_t old, uint64_t since_ms, uint64_t accepted) {
    const uint64_t elapsed = A.now_ms >= since_ms ? A.now_ms - since_ms : 0;
    const uint64_t D = elapsed ? elapsed : 1;
    const uint64_t N = (accepted < 0xFFFFFFFFull ? accepted : 0xFFFFFFFFull) * A.target_ms;  // below 2^64
    const U128 P = mul_64x64(old, N);
    uint64_t rem;
    // an ideal of 2^64 or more is cut by the upper clamp below, which is below 2^64: saturate it
    const uint64_t ideal = P.hi >= D ? ~0ull : div_128by64(P.hi, P.lo, D, &rem);
    uint64_t lo = old / A.max_down;
    lo = lo ? lo : 1;
    const U128 up = mul_64x64(old, A.max_up);
    const uint64_t hi = up.hi ? ~0ull : up.lo;
    uint64_t nw = ideal > lo ? ideal : lo;
    nw = nw < hi ? nw : hi;
    nw = nw > A.min_fx ? nw : A.min_fx;
    nw = nw < A.max_fx ? nw : A.max_fx;
    const uint64_t diff = nw > old ? nw - old : old - nw;
    return le_128(mul_64x64(diff, 1000), mul_64x64(old, A.band_permille)) ? old : nw;
}

}  // namespace bm
