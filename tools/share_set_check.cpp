// share_set_check.cpp -- stand-alone CPU check of the share set's host code
// (csrc/bm_share_set.cpp, csrc/bm_share_set_host.hpp over csrc/bm_job.hpp) under
// sanitizers, tools/pool_verify_check.cpp's recipe: the CPU set (the specification
// of bm_share_set_verify) on exactly-sized heap buffers for the job's parts,
// `sessions`, `submits` and `verdicts`, against bm_pool_verify_cpu plus a std::set
// restated here; BM_EFULL and its rollback; the argument checks, with canaries;
// creation, clear and count.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/share_set_check.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_share_set.cpp distributed_bitcoin_minter_amd/csrc/bm_job.cpp
//     -o share_set_check && ./share_set_check
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "bm_share_set_host.hpp"

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

std::unique_ptr<uint8_t[]> random_exact(size_t n) {  // exactly n bytes: the sanitizer sees any access past them
    std::unique_ptr<uint8_t[]> p(n ? new uint8_t[n] : nullptr);
    for (size_t i = 0; i < n; ++i) p[i] = rnd8();
    return p;
}

struct OwnedJob {
    std::unique_ptr<uint8_t[]> c1, c2, br;
    std::unique_ptr<bm_job_t> job;
};

OwnedJob make_job(size_t pos, uint32_t size1, uint32_t size2, size_t total, size_t nbranch, uint32_t nbits) {
    OwnedJob o;
    o.c1 = random_exact(pos);
    o.c2 = random_exact(total - pos - size1 - size2);
    o.br = random_exact(32 * nbranch);
    o.job.reset(new bm_job_t);
    std::memset(o.job.get(), 0, sizeof(bm_job_t));
    o.job->coinb1 = o.c1.get();
    o.job->coinb1_len = pos;
    o.job->extranonce1 = nullptr;  // ignored by the pool entries
    o.job->extranonce1_len = size1;
    o.job->extranonce2_size = size2;
    o.job->coinb2 = o.c2.get();
    o.job->coinb2_len = total - pos - size1 - size2;
    o.job->branch = o.br.get();
    o.job->nbranch = nbranch;
    for (auto& b : o.job->prevhash) b = rnd8();
    o.job->version = 0x20000000u;
    o.job->nbits = nbits;
    return o;
}

using Key = std::array<uint8_t, 32>;

struct SetDeleter {
    void operator()(bm_share_set_t* s) const { bm_share_set_destroy(s); }
};
using SetPtr = std::unique_ptr<bm_share_set_t, SetDeleter>;

SetPtr make_set(size_t capacity) {
    bm_share_set_t* s = nullptr;
    expect(bm_share_set_create_cpu(capacity, &s) == BM_OK && s, "a CPU set");
    return SetPtr(s);
}

bool all_bytes(const void* p, size_t n, uint8_t v) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i)
        if (b[i] != v) return false;
    return true;
}

// Batches on one set against bm_pool_verify_cpu plus a std::set, every array exactly sized.
void batches() {
    OwnedJob o = make_job(61, 4, 4, 200, 2, 0x2000ffffu);
    const size_t nses = 5;
    std::unique_ptr<bm_pool_session_t[]> ses(new bm_pool_session_t[nses]);
    for (size_t s = 0; s < nses; ++s) {
        for (auto& b : ses[s].extranonce1) b = rnd8();
        std::memset(ses[s].target, 0xFF, 32);
        ses[s].target[0] = s == 0 ? 0x7F : s == 1 ? 0x00 : 0xFF;  // about a half, almost none, all
    }
    SetPtr set = make_set(400);
    std::set<Key> model;
    std::vector<bm_pool_submit_t> pool;  // what earlier batches held
    for (size_t n : {(size_t)1, (size_t)64, (size_t)129, (size_t)200}) {
        std::unique_ptr<bm_pool_submit_t[]> subs(new bm_pool_submit_t[n]);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t pick = rnd8() % 4;
            if (pick == 0 && i) {
                subs[i] = subs[rnd32() % i];
            } else if (pick == 1 && !pool.empty()) {
                subs[i] = pool[rnd32() % pool.size()];
            } else {
                subs[i].extranonce2 = rnd32();
                subs[i].ntime = 1000 + rnd8() % 8;
                subs[i].nonce = rnd32();
                subs[i].version = rnd32();
                subs[i].session = rnd8() % (nses + 1);  // one in six is past the table: INVALID
            }
        }
        std::unique_ptr<bm_job_verdict_t[]> plain(new bm_job_verdict_t[n]), got(new bm_job_verdict_t[n]);
        bm_pool_verify_result_t pr;
        expect(bm_pool_verify_cpu(o.job.get(), ses.get(), nses, subs.get(), n, 1002, 1005, plain.get(), &pr) == BM_OK,
               "the plain verdicts");
        bm_share_set_result_t r;
        expect(bm_share_set_verify(set.get(), o.job.get(), ses.get(), nses, subs.get(), n, 1002, 1005, got.get(), &r) == BM_OK,
               "a batch that fits");
        bool same = true;
        uint64_t dups = 0, recorded = 0;
        for (size_t i = 0; i < n; ++i) {
            uint32_t st = plain[i].status;
            if ((st & (BM_SUBMIT_SHARE | BM_SUBMIT_BLOCK)) && !(st & BM_SUBMIT_INVALID)) {
                Key k;
                std::memcpy(k.data(), plain[i].hash, 32);
                if (model.insert(k).second)
                    ++recorded;
                else
                    st |= BM_SUBMIT_DUPLICATE, ++dups;
            }
            same = same && std::memcmp(plain[i].hash, got[i].hash, 32) == 0 && got[i].status == st && got[i].reserved == 0;
        }
        expect(same, "every verdict is bm_pool_verify_cpu's, DUPLICATE where the restated set holds the hash");
        expect(r.n == pr.n && r.shares == pr.shares && r.blocks == pr.blocks && r.invalid == pr.invalid &&
                   r.ntime == pr.ntime && r.duplicates == dups && r.recorded == recorded && r.count == model.size(),
               "the result");
        uint64_t count = 0, capacity = 0;
        expect(bm_share_set_count(set.get(), &count, &capacity) == BM_OK && count == model.size() && capacity == 400,
               "the count");
        for (size_t i = 0; i < n; ++i) pool.push_back(subs[i]);
    }
    expect(model.size() > 100, "the batches recorded something");
    expect(bm_share_set_clear(set.get()) == BM_OK, "clear");
    uint64_t count = 7;
    expect(bm_share_set_count(set.get(), &count, nullptr) == BM_OK && count == 0, "clear forgets");
}

// BM_EFULL: nothing written, nothing recorded; and the refusals, with canaries.
void full_and_refusals() {
    OwnedJob o = make_job(20, 4, 4, 90, 1, 0x1d00ffffu);
    const size_t n = 6, nses = 1;
    std::unique_ptr<bm_pool_session_t[]> ses(new bm_pool_session_t[nses]);
    std::memset(ses.get(), 0xFF, nses * sizeof(bm_pool_session_t));  // every hash a share
    std::unique_ptr<bm_pool_submit_t[]> subs(new bm_pool_submit_t[n]);
    std::memset(subs.get(), 0, n * sizeof(bm_pool_submit_t));
    for (size_t i = 0; i < n; ++i) subs[i].nonce = (uint32_t)(i % 4);  // four distinct hashes, two repeats
    std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[n]);
    std::memset(v.get(), 0xA5, n * sizeof(bm_job_verdict_t));
    bm_share_set_result_t out;
    std::memset(&out, 0x5A, sizeof out);
    const bm_job_t* j = o.job.get();
    const uint32_t U = 0xFFFFFFFFu;
    SetPtr set = make_set(3);
    bm_share_set_t* s = set.get();
    expect(bm_share_set_verify(s, j, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EFULL, "four new hashes into three");
    uint64_t count = 9;
    expect(bm_share_set_count(s, &count, nullptr) == BM_OK && count == 0, "a refused batch records nothing");
    expect(bm_share_set_verify(nullptr, j, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "a NULL set");
    expect(bm_share_set_verify(s, nullptr, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "a NULL job");
    expect(bm_share_set_verify(s, j, nullptr, nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "NULL sessions with nsessions > 0");
    expect(bm_share_set_verify(s, j, ses.get(), nses, nullptr, n, 0, U, v.get(), &out) == BM_EINVAL, "NULL submits with n > 0");
    expect(bm_share_set_verify(s, j, ses.get(), nses, subs.get(), n, 0, U, nullptr, &out) == BM_EINVAL, "NULL verdicts with n > 0");
    expect(bm_share_set_verify(s, j, ses.get(), nses, subs.get(), n, 0, U, v.get(), nullptr) == BM_EINVAL, "a NULL out");
    expect(bm_share_set_verify(s, j, ses.get(), nses, subs.get(), (size_t)BM_MAX_JOB_SUBMITS + 1, 0, U, v.get(), &out) == BM_EINVAL,
           "more than BM_MAX_JOB_SUBMITS (nothing is read)");
    expect(bm_share_set_verify(s, j, ses.get(), (size_t)BM_MAX_POOL_SESSIONS + 1, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL,
           "more than BM_MAX_POOL_SESSIONS (nothing is read)");
    bm_job_t bad = *j;
    bad.extranonce1_len = 9;
    expect(bm_share_set_verify(s, &bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "extranonce1_len 9");
    bad = *j, bad.extranonce2_size = 0;
    expect(bm_share_set_verify(s, &bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "size 0");
    bad = *j, bad.coinb2 = nullptr;
    expect(bm_share_set_verify(s, &bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "a NULL coinb2 with a length");
    expect(all_bytes(v.get(), n * sizeof(bm_job_verdict_t), 0xA5) && all_bytes(&out, sizeof out, 0x5A),
           "verdicts and out are untouched by BM_EFULL and by every refusal");
    // n == 0: legal, changes nothing, needs no array
    expect(bm_share_set_verify(s, j, nullptr, 0, nullptr, 0, 0, U, nullptr, &out) == BM_OK && out.n == 0 && out.count == 0 &&
               out.recorded == 0 && out.duplicates == 0,
           "n == 0 with NULL arrays");
    expect(all_bytes(v.get(), n * sizeof(bm_job_verdict_t), 0xA5), "n == 0 touches no verdict");
    // three of them fit; then the refused batch's fourth still does not, and what is there is a duplicate
    expect(bm_share_set_verify(s, j, ses.get(), nses, subs.get(), 3, 0, U, v.get(), &out) == BM_OK && out.recorded == 3 &&
               out.count == 3 && out.duplicates == 0,
           "three fit");
    expect(all_bytes(v.get() + 3, 3 * sizeof(bm_job_verdict_t), 0xA5), "a batch shorter than its arrays leaves the rest alone");
    std::memset(v.get(), 0xA5, n * sizeof(bm_job_verdict_t));
    expect(bm_share_set_verify(s, j, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EFULL, "a full set");
    expect(all_bytes(v.get(), n * sizeof(bm_job_verdict_t), 0xA5), "BM_EFULL writes no verdict");
    expect(bm_share_set_verify(s, j, ses.get(), nses, subs.get() + 4, 2, 0, U, v.get(), &out) == BM_OK && out.duplicates == 2 &&
               out.recorded == 0 && out.count == 3 && (v[0].status & BM_SUBMIT_DUPLICATE) && (v[1].status & BM_SUBMIT_DUPLICATE),
           "repeats of what the set holds");
}

void creation() {
    bm_share_set_t* s = reinterpret_cast<bm_share_set_t*>(0x5A5A);
    expect(bm_share_set_create_cpu(0, &s) == BM_EINVAL, "capacity 0");
    expect(bm_share_set_create_cpu((size_t)BM_MAX_SHARE_SET + 1, &s) == BM_EINVAL, "capacity above BM_MAX_SHARE_SET");
    expect(bm_share_set_create_cpu(8, nullptr) == BM_EINVAL, "a NULL out");
    expect(s == reinterpret_cast<bm_share_set_t*>(0x5A5A), "a refused creation leaves *out");
    bm_share_set_destroy(nullptr);
    expect(bm_share_set_clear(nullptr) == BM_EINVAL && bm_share_set_count(nullptr, nullptr, nullptr) == BM_EINVAL,
           "a NULL set");
    SetPtr big = make_set(BM_MAX_SHARE_SET);
    uint64_t count = 1, capacity = 0;
    expect(bm_share_set_count(big.get(), &count, &capacity) == BM_OK && count == 0 && capacity == BM_MAX_SHARE_SET,
           "the largest set");
    expect(bm::share_set_slots(1) == 16 && bm::share_set_slots(8) == 16 && bm::share_set_slots(9) == 32 &&
               bm::share_set_slots(BM_MAX_SHARE_SET) == (1u << 25),
           "the slot count: a power of two, at least twice the capacity, at least 16");
}

}  // namespace

int main() {
    static_assert(sizeof(bm_share_set_result_t) == 64, "layout");
    creation();
    batches();
    full_and_refusals();
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("share set check ok\n");
    return 0;
}
