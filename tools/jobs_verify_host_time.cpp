// jobs_verify_host_time.cpp -- what the host side of bm_jobs_verify_gpu takes on its
// own (no GPU, no HIP): the grouping (host::jobs_plan's count and block table, then
// host::jobs_stage's scatter, which in the library is the copy into the pinned
// buffer) over n submissions assigned at random to J jobs, and the tripwire's J
// per-job entries by the CPU path.  Built and run by tools/bench_jobs_verify.py:
//
//   g++ -std=c++17 -O3 -I distributed_bitcoin_minter_amd/csrc -I include tools/jobs_verify_host_time.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_job.cpp -o jobs_verify_host_time && ./jobs_verify_host_time 131072 64 12
//
// prints one JSON line: the medians, minima and maxima of 10 rounds after 2, in ms.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bm_job.hpp"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void report(const char* name, std::vector<double> v, bool last) {
    std::sort(v.begin(), v.end());
    const double med = (v[v.size() / 2] + v[(v.size() - 1) / 2]) / 2;
    std::printf("\"%s\": {\"median_ms\": %.6f, \"min_ms\": %.6f, \"max_ms\": %.6f}%s", name, med, v.front(), v.back(),
                last ? "" : ", ");
}

}  // namespace

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1u << 17;
    const size_t J = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 64;
    const size_t depth = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 12;
    if (n == 0 || n > BM_MAX_JOB_SUBMITS || J == 0 || J > BM_MAX_POOL_JOBS || depth > BM_MAX_JOB_BRANCH) return 2;
    const int rounds = 10, warmup = 2;
    std::vector<std::vector<uint8_t>> bytes;
    std::vector<bm_pool_job_t> jobs(J);
    for (auto& pj : jobs) {
        pj = bm_pool_job_t();
        for (size_t len : {(size_t)100, (size_t)138, 32 * depth}) {
            bytes.emplace_back(len);
            for (auto& b : bytes.back()) b = (uint8_t)rnd();
        }
        pj.job.coinb1 = bytes[bytes.size() - 3].data(), pj.job.coinb1_len = 100;
        pj.job.extranonce1_len = 4, pj.job.extranonce2_size = 8;
        pj.job.coinb2 = bytes[bytes.size() - 2].data(), pj.job.coinb2_len = 138;
        pj.job.branch = bytes[bytes.size() - 1].data(), pj.job.nbranch = depth;
        pj.job.nbits = 0x1d00ffffu;
        pj.ntime_hi = 0xFFFFFFFFu;
    }
    std::vector<bm_pool_session_t> sessions(1 << 12);
    for (auto& s : sessions)
        for (auto& b : s.extranonce1) b = (uint8_t)rnd();
    std::vector<bm_jobs_submit_t> submits(n), staged(n);
    for (auto& s : submits) {
        s.extranonce2 = rnd(), s.ntime = (uint32_t)rnd(), s.nonce = (uint32_t)rnd(), s.version = (uint32_t)rnd();
        s.session = (uint32_t)(rnd() % sessions.size()), s.job = (uint32_t)(rnd() % J), s.reserved = 0;
    }
    std::vector<double> group, trip;
    bm::host::JobsPlan P;
    uint32_t sink = 0;
    for (int r = 0; r < warmup + rounds; ++r) {
        double t = now_ms();
        bm::host::jobs_plan(submits.data(), n, J, P);
        bm::host::jobs_stage(submits.data(), n, J, P, staged.data());
        const double g = now_ms() - t;
        t = now_ms();
        for (size_t j = 0; j < J; ++j) {  // the lowest-index submission of each job
            if (P.start[j] == P.start[j + 1]) continue;
            bm_job_verdict_t v;
            bm::host::jobs_verify_one(jobs.data(), J, sessions.data(), sessions.size(), submits[staged[P.start[j]].job], v);
            sink += v.hash[31];
        }
        const double w = now_ms() - t;
        if (r >= warmup) group.push_back(g), trip.push_back(w);
    }
    std::printf("{\"n\": %zu, \"jobs\": %zu, \"depth\": %zu, \"blocks\": %zu, \"sink\": %u, ", n, J, depth, P.blocks.size(), sink);
    report("grouping", group, false);
    report("tripwire_per_job", trip, true);
    std::printf("}\n");
    return 0;
}
