// jobs_verify_check.cpp -- stand-alone CPU check of the host code of verification
// over several jobs (csrc/bm_job.hpp, csrc/bm_job.cpp) under sanitizers,
// tools/pool_verify_check.cpp's recipe: bm_jobs_verify_cpu on exactly-sized heap
// buffers for the jobs, `sessions`, `submits` and `verdicts`, against
// bm_pool_verify_cpu per submission; the host grouping (host::jobs_plan's counting
// sort and block table, host::jobs_stage's scatter into an exactly-sized stage);
// the descriptors and offsets of host::jobs_verify_prepare against
// host::pool_verify_prepare per job; the tripwire's entries; and the refusals, with
// canaries.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/jobs_verify_check.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_job.cpp -o jobs_verify_check && ./jobs_verify_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bm_job.hpp"

namespace {

int fails = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++fails;
    }
}

uint32_t rng_state = 0x9E3779B9u;
uint8_t rnd8() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 16);
}
uint32_t rnd32() { return ((uint32_t)rnd8() << 24) | ((uint32_t)rnd8() << 16) | ((uint32_t)rnd8() << 8) | rnd8(); }
uint64_t rnd64() { return ((uint64_t)rnd32() << 32) | rnd32(); }

// A heap copy of exactly n bytes (nullptr for none): the sanitizer sees any access past it.
std::unique_ptr<uint8_t[]> random_exact(size_t n) {
    std::unique_ptr<uint8_t[]> p(n ? new uint8_t[n] : nullptr);
    for (size_t i = 0; i < n; ++i) p[i] = rnd8();
    return p;
}

// Jobs that own exactly-sized copies of their parts; their own extranonce1 pointers are NULL.
struct OwnedJobs {
    std::vector<std::unique_ptr<uint8_t[]>> parts;
    std::unique_ptr<bm_pool_job_t[]> jobs;  // exactly njobs entries
    size_t njobs = 0;
};

// Job j: the field (size1 + size2 bytes) at byte pos of a coinbase of total bytes.
struct Shape {
    size_t pos, size1, size2, total, depth;
    uint32_t nbits, lo, hi;
};

OwnedJobs make_jobs(const std::vector<Shape>& shapes) {
    OwnedJobs o;
    o.njobs = shapes.size();
    o.jobs.reset(o.njobs ? new bm_pool_job_t[o.njobs] : nullptr);
    for (size_t j = 0; j < o.njobs; ++j) {
        const Shape& s = shapes[j];
        bm_pool_job_t& pj = o.jobs[j];
        std::memset(&pj, 0, sizeof pj);
        const size_t c2 = s.total - s.pos - s.size1 - s.size2;
        o.parts.push_back(random_exact(s.pos));
        pj.job.coinb1 = o.parts.back().get();
        pj.job.coinb1_len = s.pos;
        pj.job.extranonce1 = nullptr;
        pj.job.extranonce1_len = s.size1;
        pj.job.extranonce2_size = (uint32_t)s.size2;
        o.parts.push_back(random_exact(c2));
        pj.job.coinb2 = o.parts.back().get();
        pj.job.coinb2_len = c2;
        o.parts.push_back(random_exact(32 * s.depth));
        pj.job.branch = o.parts.back().get();
        pj.job.nbranch = s.depth;
        for (auto& b : pj.job.prevhash) b = rnd8();
        pj.job.version = rnd32();
        pj.job.nbits = s.nbits;
        pj.ntime_lo = s.lo;
        pj.ntime_hi = s.hi;
    }
    return o;
}

const std::vector<Shape> kShapes = {
    {10, 4, 4, 40, 0, 0x2000ffffu, 1000, 2000},       // one tail block, no branch
    {122, 8, 8, 150, 1, 0x1d80ffffu, 5, 7},           // the field across a block edge, an nbits that does not decode
    {33, 1, 1, 170, 3, 0x2000ffffu, 0x7fffffffu, 0xfffffffeu},
    {63, 8, 8, 64 + 55, 32, 0x2100ffffu, 0, 0xffffffffu},
    {0, 1, 8, 9, 2, 0x1d00ffffu, 0, 0},
};

struct Batch {
    std::unique_ptr<bm_pool_session_t[]> sessions;
    size_t nsessions = 0;
    std::unique_ptr<bm_jobs_submit_t[]> submits;
    size_t n = 0;
};

// n submissions over njobs jobs (and some past the table), nsessions sessions (and some past it).
Batch make_batch(const OwnedJobs& o, size_t nsessions, size_t n, bool round_robin) {
    Batch b;
    b.nsessions = nsessions;
    b.sessions.reset(nsessions ? new bm_pool_session_t[nsessions] : nullptr);
    for (size_t s = 0; s < nsessions; ++s) {
        for (auto& x : b.sessions[s].extranonce1) x = rnd8();
        std::memset(b.sessions[s].target, s % 3 == 0 ? 0xFF : s % 3 == 1 ? 0x7F : 0x00, 32);
    }
    b.n = n;
    b.submits.reset(n ? new bm_jobs_submit_t[n] : nullptr);
    for (size_t i = 0; i < n; ++i) {
        bm_jobs_submit_t& s = b.submits[i];
        const uint32_t r = rnd32() % 16;
        s.job = round_robin && o.njobs ? (uint32_t)(i % o.njobs) : (uint32_t)(rnd32() % (o.njobs + 1));
        if (r == 0) s.job = 0xFFFFFFFFu;
        const uint32_t size2 = s.job < o.njobs ? o.jobs[s.job].job.extranonce2_size : 1;
        s.extranonce2 = size2 >= 8 ? rnd64() : rnd64() & ((1ull << (8 * size2)) - 1);
        if (r == 1 && size2 < 8) s.extranonce2 |= 1ull << (8 * size2);  // does not fit
        s.ntime = s.job < o.njobs ? o.jobs[s.job].ntime_lo + (rnd32() % 4) - 1 : rnd32();
        s.nonce = rnd32();
        s.version = rnd32();
        s.session = r == 2 ? (uint32_t)nsessions : (uint32_t)(rnd32() % (nsessions ? nsessions : 1));
        s.reserved = rnd32();
    }
    return b;
}

// ---- bm_jobs_verify_cpu against bm_pool_verify_cpu per submission ----
void cpu_entry_cases() {
    OwnedJobs o = make_jobs(kShapes);
    for (size_t n : {(size_t)1, (size_t)2, (size_t)65, (size_t)300}) {
        Batch b = make_batch(o, 9, n, n == 65);
        std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[n]);
        bm_pool_verify_result_t r;
        expect(bm_jobs_verify_cpu(o.jobs.get(), o.njobs, b.sessions.get(), 9, b.submits.get(), n, v.get(), &r) == BM_OK,
               "bm_jobs_verify_cpu succeeds");
        bool ok = true;
        uint64_t shares = 0, blocks = 0, invalid = 0, ntime = 0;
        for (size_t i = 0; i < n; ++i) {
            const bm_jobs_submit_t& s = b.submits[i];
            bm_job_verdict_t want;
            if (s.job >= o.njobs) {
                std::memset(&want, 0, sizeof want);
                std::memset(want.hash, 0xFF, 32);
                want.status = BM_SUBMIT_INVALID;
            } else {
                std::unique_ptr<bm_pool_submit_t> ps(new bm_pool_submit_t{s.extranonce2, s.ntime, s.nonce, s.version, s.session});
                bm_pool_verify_result_t one;
                const bm_pool_job_t& pj = o.jobs[s.job];
                ok = ok && bm_pool_verify_cpu(&pj.job, b.sessions.get(), 9, ps.get(), 1, pj.ntime_lo, pj.ntime_hi, &want,
                                              &one) == BM_OK;
            }
            ok = ok && std::memcmp(&want, &v[i], sizeof want) == 0;
            shares += (want.status & BM_SUBMIT_SHARE) ? 1 : 0;
            blocks += (want.status & BM_SUBMIT_BLOCK) ? 1 : 0;
            invalid += (want.status & BM_SUBMIT_INVALID) ? 1 : 0;
            ntime += (want.status & BM_SUBMIT_NTIME) ? 1 : 0;
        }
        expect(ok, "every verdict is bm_pool_verify_cpu's under the submission's job and window");
        expect(r.n == n && r.shares == shares && r.blocks == blocks && r.invalid == invalid && r.ntime == ntime,
               "the counts are over the whole batch");
        if (n == 300) expect(shares > 0 && invalid > 0 && ntime > 0, "the batch holds shares, INVALID and NTIME entries");
    }
    // no jobs, no sessions: every entry INVALID, both tables NULL
    Batch b = make_batch(o, 0, 65, false);
    std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[65]);
    bm_pool_verify_result_t r;
    expect(bm_jobs_verify_cpu(nullptr, 0, nullptr, 0, b.submits.get(), 65, v.get(), &r) == BM_OK && r.invalid == 65,
           "njobs == 0 with n > 0: all INVALID");
    expect(bm_jobs_verify_cpu(o.jobs.get(), o.njobs, nullptr, 0, b.submits.get(), 65, v.get(), &r) == BM_OK && r.invalid == 65,
           "no sessions: all INVALID");
}

// ---- the grouping: counting sort, block table, scatter ----
void grouping_case(size_t njobs, size_t n, bool round_robin) {
    Batch b;
    {
        OwnedJobs some = make_jobs(std::vector<Shape>(kShapes.begin(), kShapes.begin() + (njobs < 5 ? njobs : 5)));
        b = make_batch(some, 4, n, round_robin);
    }
    if (njobs > 5)  // only the job field counts here
        for (size_t i = 0; i < n; ++i) b.submits[i].job = rnd32() % 8 == 0 ? 0xFFFFFFF0u : (uint32_t)(rnd32() % njobs);
    bm::host::JobsPlan P;
    bm::host::jobs_plan(b.submits.get(), n, njobs, P);
    std::unique_ptr<bm_jobs_submit_t[]> staged(n ? new bm_jobs_submit_t[n] : nullptr);  // exactly n records
    bm::host::jobs_stage(b.submits.get(), n, njobs, P, staged.get());
    bool ok = P.start.size() == njobs + 2 && P.start[0] == 0 && P.start[njobs + 1] == n;
    // the groups: sizes, content, stability
    std::vector<uint32_t> count(njobs + 1, 0);
    for (size_t i = 0; i < n; ++i) ++count[b.submits[i].job < njobs ? b.submits[i].job : njobs];
    size_t grid = 0;
    for (size_t g = 0; ok && g <= njobs; ++g) {
        ok = ok && P.start[g + 1] - P.start[g] == count[g];
        grid += (count[g] + 63) / 64;
        for (uint32_t k = P.start[g]; ok && k < P.start[g + 1]; ++k) {
            const bm_jobs_submit_t& r = staged[k];
            ok = ok && r.job < n && r.reserved == 0;
            if (!ok) break;
            const bm_jobs_submit_t& s = b.submits[r.job];
            ok = ok && (s.job < njobs ? s.job : njobs) == g && r.extranonce2 == s.extranonce2 && r.ntime == s.ntime &&
                 r.nonce == s.nonce && r.version == s.version && r.session == s.session;
            if (k > P.start[g]) ok = ok && staged[k - 1].job < r.job;  // the caller's order inside a group
        }
    }
    expect(ok, "the stage holds every group in the caller's order, the original index in `job`");
    // the block table: never across two groups, at most 64, every record exactly once, in order
    ok = P.blocks.size() == grid;
    uint32_t at = 0;
    for (const bm::JobsVerifyBlock& blk : P.blocks) {
        const size_t g = blk.job == bm::kJobsNone ? njobs : blk.job;
        ok = ok && g <= njobs && blk.first == at && blk.count >= 1 && blk.count <= 64 && blk.reserved == 0;
        if (!ok) break;
        ok = ok && blk.first >= P.start[g] && blk.first + blk.count <= P.start[g + 1];
        ok = ok && (blk.count == 64 || blk.first + blk.count == P.start[g + 1]);
        at += blk.count;
    }
    expect(ok && at == n, "the block table covers the stage, no entry across two jobs");
}

void grouping_cases() {
    for (size_t njobs : {(size_t)0, (size_t)1, (size_t)3, (size_t)5, (size_t)64})
        for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)129, (size_t)200, (size_t)4097})
            for (int rr = 0; rr < 2; ++rr) grouping_case(njobs, n, rr == 1);
}

// ---- the descriptors and offsets against pool_verify_prepare per job ----
void prepare_cases() {
    OwnedJobs o = make_jobs(kShapes);
    std::vector<bm::JobsVerifyDesc> desc;
    std::vector<uint32_t> words;
    bm::host::jobs_verify_prepare(o.jobs.get(), o.njobs, desc, words);
    bool ok = desc.size() == o.njobs;
    size_t tails = 0, branches = 0;
    for (size_t j = 0; ok && j < o.njobs; ++j) {
        bm::PoolVerifyArgs A;
        std::vector<uint32_t> tail, branch;
        bm::host::pool_verify_prepare(&o.jobs[j].job, A, tail, branch);
        const bm::JobsVerifyDesc& D = desc[j];
        ok = ok && std::memcmp(D.mid, A.mid, 32) == 0 && std::memcmp(D.prev, A.prev, 32) == 0 &&
             std::memcmp(D.btgt, A.btgt, 32) == 0 && D.nbits == A.nbits && D.has_block == A.has_block && D.nb == A.nb &&
             D.j0 == A.j0 && D.boff == A.boff && D.size1 == A.size1 && D.size2 == A.size2 && D.depth == A.depth &&
             D.ntime_lo == o.jobs[j].ntime_lo && D.ntime_hi == o.jobs[j].ntime_hi;
        ok = ok && D.tail_off == tails && (size_t)D.tail_off + tail.size() <= words.size() &&
             std::memcmp(words.data() + D.tail_off, tail.data(), 4 * tail.size()) == 0;
        tails += tail.size();
        branches += branch.size();
    }
    size_t at = tails;  // all tails, then all branches
    for (size_t j = 0; ok && j < o.njobs; ++j) {
        bm::PoolVerifyArgs A;
        std::vector<uint32_t> tail, branch;
        bm::host::pool_verify_prepare(&o.jobs[j].job, A, tail, branch);
        ok = ok && desc[j].branch_off == at && at + branch.size() <= words.size() &&
             (branch.empty() || std::memcmp(words.data() + at, branch.data(), 4 * branch.size()) == 0);
        at += branch.size();
    }
    expect(ok && words.size() == tails + branches && words.size() % 2 == 0,
           "a descriptor is pool_verify_prepare's, its offsets name its own tail and branch");
    bm::host::jobs_verify_prepare(nullptr, 0, desc, words);
    expect(desc.empty() && words.empty(), "no jobs: no descriptors, no words");
}

// ---- the tripwire ----
void tripwire_cases() {
    OwnedJobs o = make_jobs(kShapes);
    const size_t n = 200;
    Batch b = make_batch(o, 9, n, true);
    b.submits[0].job = 4, b.submits[n - 1].job = 4;  // the ends on one job: the others are caught at their first entry only
    for (uint32_t i = 1; i <= 3; ++i) b.submits[i].job = i;
    std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[n]);
    bm_pool_verify_result_t r;
    expect(bm_jobs_verify_cpu(o.jobs.get(), o.njobs, b.sessions.get(), 9, b.submits.get(), n, v.get(), &r) == BM_OK, "cpu");
    bm::host::JobsPlan P;
    bm::host::jobs_plan(b.submits.get(), n, o.njobs, P);
    std::unique_ptr<bm_jobs_submit_t[]> staged(new bm_jobs_submit_t[n]);
    bm::host::jobs_stage(b.submits.get(), n, o.njobs, P, staged.get());
    auto trip = [&](uint32_t ignore) {
        return bm::host::jobs_verify_tripwire(o.jobs.get(), o.njobs, b.sessions.get(), 9, b.submits.get(), n, P, staged.get(),
                                              v.get(), ignore);
    };
    expect(trip(0) == BM_OK, "the tripwire accepts the CPU path's verdicts");
    for (size_t i = 0; i < n; ++i) v[i].status |= BM_SUBMIT_DUPLICATE;
    expect(trip(0) == BM_EINTERNAL && trip(BM_SUBMIT_DUPLICATE) == BM_OK, "the ignored bits do not count");
    for (size_t i = 0; i < n; ++i) v[i].status &= ~BM_SUBMIT_DUPLICATE;
    // the lowest-index entries of jobs 1, 2 and 3 (indices 1, 2 and 3)
    for (size_t i : {(size_t)1, (size_t)2, (size_t)3}) {
        const bm_job_verdict_t keep = v[i];
        v[i].hash[31] ^= 1;
        expect(trip(0) == BM_EINTERNAL, "a wrong verdict at a job's lowest index is caught");
        v[i] = keep;
    }
    const bm_job_verdict_t keep = v[100];
    v[100].hash[31] ^= 1;
    if (!(v[100].status & BM_SUBMIT_BLOCK)) expect(trip(0) == BM_OK, "an entry the tripwire does not visit");
    v[100] = keep;
    expect(trip(0) == BM_OK, "restored");
}

// ---- the refusals, with canaries ----
void refusal_cases() {
    OwnedJobs o = make_jobs(kShapes);
    Batch b = make_batch(o, 3, 3, true);
    bm_job_verdict_t v[3];
    bm_pool_verify_result_t r;
    std::memset(v, 0xA5, sizeof v);
    std::memset(&r, 0x5A, sizeof r);
    bm_job_verdict_t v0[3];
    bm_pool_verify_result_t r0;
    std::memcpy(v0, v, sizeof v);
    std::memcpy(&r0, &r, sizeof r);
    const bm_pool_job_t* J = o.jobs.get();
    const bm_pool_session_t* S = b.sessions.get();
    const bm_jobs_submit_t* U = b.submits.get();
    bool ok = true;
    ok = ok && bm_jobs_verify_cpu(nullptr, 5, S, 3, U, 3, v, &r) == BM_EINVAL;
    ok = ok && bm_jobs_verify_cpu(J, BM_MAX_POOL_JOBS + 1, S, 3, U, 3, v, &r) == BM_EINVAL;  // before a job is read
    ok = ok && bm_jobs_verify_cpu(J, 5, nullptr, 3, U, 3, v, &r) == BM_EINVAL;
    ok = ok && bm_jobs_verify_cpu(J, 5, S, 3, nullptr, 3, v, &r) == BM_EINVAL;
    ok = ok && bm_jobs_verify_cpu(J, 5, S, 3, U, 3, nullptr, &r) == BM_EINVAL;
    ok = ok && bm_jobs_verify_cpu(J, 5, S, 3, U, 3, v, nullptr) == BM_EINVAL;
    ok = ok && bm_jobs_verify_cpu(J, 5, S, 3, U, (size_t)BM_MAX_JOB_SUBMITS + 1, v, &r) == BM_EINVAL;
    ok = ok && bm_jobs_verify_cpu(J, 5, S, (size_t)BM_MAX_POOL_SESSIONS + 1, U, 3, v, &r) == BM_EINVAL;
    expect(ok, "the argument refusals");
    ok = true;
    for (size_t j = 0; j < o.njobs; ++j) {  // a malformed job, named by a submission or not
        bm_pool_job_t& pj = o.jobs[j];
        const bm_job_t keep = pj.job;
        pj.job.extranonce2_size = 9;
        ok = ok && bm_jobs_verify_cpu(J, 5, S, 3, U, 3, v, &r) == BM_EINVAL;
        pj.job = keep;
        pj.job.extranonce1_len = 0;
        ok = ok && bm_jobs_verify_cpu(J, 5, S, 3, U, 3, v, &r) == BM_EINVAL;
        pj.job = keep;
        pj.job.nbranch = BM_MAX_JOB_BRANCH + 1;
        ok = ok && bm_jobs_verify_cpu(J, 5, S, 3, U, 0, nullptr, &r) == BM_EINVAL;
        pj.job = keep;
        pj.job.coinb2_len = BM_MAX_JOB_COINBASE;
        ok = ok && bm_jobs_verify_cpu(J, 5, S, 3, U, 3, v, &r) == BM_EINVAL;
        pj.job = keep;
    }
    expect(ok, "a malformed job is refused whichever it is");
    expect(std::memcmp(v, v0, sizeof v) == 0 && std::memcmp(&r, &r0, sizeof r) == 0, "a refusal touches neither array");
    expect(bm_jobs_verify_cpu(J, 5, S, 3, nullptr, 0, nullptr, &r) == BM_OK && r.n == 0 && r.invalid == 0,
           "n == 0 succeeds and touches no array");
    expect(std::memcmp(v, v0, sizeof v) == 0, "n == 0 leaves the verdicts alone");
}

}  // namespace

int main() {
    cpu_entry_cases();
    grouping_cases();
    prepare_cases();
    tripwire_cases();
    refusal_cases();
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("jobs verify check ok\n");
    return 0;
}
