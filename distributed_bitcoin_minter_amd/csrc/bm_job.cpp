// bm_job.cpp -- the pure-CPU entries of the Stratum job layer (include/btcminer.h):
// bm_job_prevhash_from_stratum, bm_job_header, bm_job_verify_cpu,
// bm_pool_verify_cpu, bm_jobs_verify_cpu, bm_target_from_difficulty, bm_target_from_difficulty_fx.  They need no context and no GPU;
// bm_search_job_shares_gpu (bm_search.cpp) builds its headers and
// bm_job_verify_gpu and bm_pool_verify_gpu (bm_aux.hip) check their device with the same code
// (bm_job.hpp).  Plain C++: no HIP in here.
#include "bm_job.hpp"

#include <cmath>

extern "C" {

int bm_job_prevhash_from_stratum(const uint8_t in[32], uint8_t out[32]) {
    if (!in || !out) return BM_EINVAL;
    uint8_t t[32];  // in and out may be the same array
    for (int w = 0; w < 8; ++w)
        for (int b = 0; b < 4; ++b) t[4 * w + b] = in[4 * w + 3 - b];
    std::memcpy(out, t, sizeof t);
    return BM_OK;
}

int bm_job_header(const bm_job_t* job, uint64_t extranonce2, uint32_t ntime, uint32_t version, uint8_t header[80]) {
    if (!header) return BM_EINVAL;
    const int rc = bm::host::job_check(job);
    if (rc != BM_OK) return rc;
    if (!bm::host::extranonce2_fits(extranonce2, job->extranonce2_size)) return BM_EINVAL;
    uint8_t h[bm::kHeaderBytes];
    bm::host::job_header(job, extranonce2, ntime, version, h);
    std::memcpy(header, h, sizeof h);
    return BM_OK;
}

// The specification of bm_job_verify_gpu, and the verifier of a caller without a
// GPU: one bm_job_header and one double hash per submission.
int bm_job_verify_cpu(const bm_job_t* job, const uint8_t target[32], const bm_job_submit_t* submits, size_t n,
                      bm_job_verdict_t* verdicts, bm_job_verify_result_t* out) {
    const int rc = bm::host::verify_check(job, target, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    uint8_t bt[32];
    const uint8_t* block_target = bm::host::target_from_bits(job->nbits, bt) ? bt : nullptr;
    for (size_t i = 0; i < n; ++i) bm::host::verify_one(job, target, block_target, submits[i], verdicts[i]);
    bm::host::verify_count(verdicts, n, *out);
    return BM_OK;
}

// The specification of bm_pool_verify_gpu: bm_job_verify_cpu with extranonce1 and
// the share target taken from the submission's session, and the ntime window.
int bm_pool_verify_cpu(const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                       const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                       bm_job_verdict_t* verdicts, bm_pool_verify_result_t* out) {
    const int rc = bm::host::pool_verify_check(job, sessions, nsessions, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    uint8_t bt[32];
    const uint8_t* block_target = bm::host::target_from_bits(job->nbits, bt) ? bt : nullptr;
    for (size_t i = 0; i < n; ++i)
        bm::host::pool_verify_one(job, sessions, nsessions, block_target, ntime_lo, ntime_hi, submits[i], verdicts[i]);
    bm::host::pool_verify_count(verdicts, n, *out);
    return BM_OK;
}

// The specification of bm_jobs_verify_gpu: bm_pool_verify_cpu per submission, with
// the submission's job and that job's window; a job index past the table is INVALID.
int bm_jobs_verify_cpu(const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions, size_t nsessions,
                       const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                       bm_pool_verify_result_t* out) {
    const int rc = bm::host::jobs_verify_check(jobs, njobs, sessions, nsessions, submits, n, verdicts, out);
    if (rc != BM_OK) return rc;
    for (size_t i = 0; i < n; ++i) bm::host::jobs_verify_one(jobs, njobs, sessions, nsessions, submits[i], verdicts[i]);
    bm::host::pool_verify_count(verdicts, n, *out);
    return BM_OK;
}

// target = floor(diff1 / difficulty), diff1 = 0xffff * 2^208, for the double's
// exact value m * 2^e (m a 53-bit integer): floor(0xffff * 2^(208 - e) / m), one
// long division of a multi-word integer by m.
int bm_target_from_difficulty(double difficulty, uint8_t target[32]) {
    if (!target || !std::isfinite(difficulty) || !(difficulty > 0.0)) return BM_EINVAL;
    int e = 0;
    const double frac = std::frexp(difficulty, &e);          // difficulty = frac * 2^e, frac in [0.5, 1)
    const uint64_t m = (uint64_t)std::ldexp(frac, 53);       // exact: 2^52 <= m < 2^53 (denormals too)
    e -= 53;                                                 // difficulty = m * 2^e
    const int shift = 208 - e;                               // the numerator is 0xffff << shift
    std::memset(target, 0, 32);
    if (shift < 0) return BM_OK;                             // 0xffff >> -shift is below m: the quotient is 0
    // shift > 320: the quotient is above 2^(15 + 321 - 53) > 2^256
    constexpr int kLimbs = 11;                               // 352 bits hold 0xffff << 320
    uint32_t num[kLimbs] = {};                               // least significant limb first
    bool saturate = shift > 320;
    if (!saturate) {
        const int limb = shift / 32, bit = shift % 32;
        const uint64_t v = (uint64_t)0xffffu << bit;
        num[limb] = (uint32_t)v;
        if (limb + 1 < kLimbs) num[limb + 1] = (uint32_t)(v >> 32);
        unsigned __int128 rem = 0;
        uint32_t q[kLimbs];
        for (int i = kLimbs - 1; i >= 0; --i) {
            rem = (rem << 32) | num[i];                      // rem < m < 2^53 before: below 2^85 here
            q[i] = (uint32_t)(rem / m);
            rem %= m;
        }
        for (int i = 8; i < kLimbs; ++i) saturate = saturate || q[i] != 0;
        if (!saturate)
            for (int i = 0; i < 8; ++i) {
                target[31 - 4 * i] = (uint8_t)q[i];
                target[30 - 4 * i] = (uint8_t)(q[i] >> 8);
                target[29 - 4 * i] = (uint8_t)(q[i] >> 16);
                target[28 - 4 * i] = (uint8_t)(q[i] >> 24);
            }
    }
    if (saturate) std::memset(target, 0xFF, 32);
    return BM_OK;
}

// target = floor(0xffff * 2^240 / difficulty_fx), the difficulty in units of 2^-32:
// one long division of the four 64-bit words of the numerator by the 64-bit divisor.
// The quotient is below 2^256 for every divisor >= 1: nothing saturates.
int bm_target_from_difficulty_fx(uint64_t difficulty_fx, uint8_t target[32]) {
    if (!target || difficulty_fx == 0) return BM_EINVAL;
    const uint64_t num[4] = {0xffffull << 48, 0, 0, 0};      // most significant word first
    unsigned __int128 rem = 0;
    for (int i = 0; i < 4; ++i) {
        rem = (rem << 64) | num[i];                           // rem < difficulty_fx before: below 2^128 here
        const uint64_t q = (uint64_t)(rem / difficulty_fx);
        rem -= (unsigned __int128)q * difficulty_fx;          // one 128-bit division per word, not two
        for (int b = 0; b < 8; ++b) target[8 * i + b] = (uint8_t)(q >> (56 - 8 * b));
    }
    return BM_OK;
}

}  // extern "C"
