// ledger_check.cpp -- stand-alone CPU check of the ledger's host code
// (csrc/bm_ledger.cpp, csrc/bm_ledger_host.hpp) under sanitizers,
// tools/share_set_check.cpp's recipe: the CPU ledger on exactly-sized heap buffers
// for the jobs' parts, `sessions`, `accounts`, `weights`, `submits`, `verdicts` and
// the rows read back, with a CPU set and without one, against bm_jobs_verify_cpu
// plus a std::set of hashes plus a std::map of rows; BM_EFULL and the refusals, with
// canaries; drain, clear and the wrap-around of `work`.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/ledger_check.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_ledger.cpp distributed_bitcoin_minter_amd/csrc/bm_share_set.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_job.cpp -o ledger_check && ./ledger_check
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "btcminer.h"

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

struct OwnedJobs {
    std::vector<std::unique_ptr<uint8_t[]>> parts;
    std::unique_ptr<bm_pool_job_t[]> jobs;  // exactly njobs entries
    size_t njobs = 0;
};

// Job j: the field (8 + size2 bytes) at byte pos of a coinbase of total bytes.
struct Shape {
    size_t pos, size2, total, depth;
    uint32_t nbits, lo, hi;
};

OwnedJobs make_jobs(const std::vector<Shape>& shapes) {
    OwnedJobs o;
    o.njobs = shapes.size();
    o.jobs.reset(new bm_pool_job_t[o.njobs]);
    for (size_t j = 0; j < o.njobs; ++j) {
        const Shape& s = shapes[j];
        bm_pool_job_t& pj = o.jobs[j];
        std::memset(&pj, 0, sizeof pj);
        const size_t c2 = s.total - s.pos - 8 - s.size2;
        o.parts.push_back(random_exact(s.pos));
        pj.job.coinb1 = o.parts.back().get();
        pj.job.coinb1_len = s.pos;
        pj.job.extranonce1_len = 8;
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
    {10, 4, 40, 0, 0x2100ffffu, 1000, 2000},  // nearly every hash is a block
    {122, 8, 150, 1, 0x1d80ffffu, 5, 7},      // an nbits that does not decode
    {33, 1, 170, 3, 0x2000ffffu, 0, 0xffffffffu},
};

struct Batch {
    std::unique_ptr<bm_pool_session_t[]> sessions;
    std::unique_ptr<uint32_t[]> accounts;
    std::unique_ptr<uint64_t[]> weights;
    size_t nsessions = 0;
    std::unique_ptr<bm_jobs_submit_t[]> submits;
    size_t n = 0;
};

Batch make_batch(const OwnedJobs& o, size_t nsessions, size_t rows, size_t n) {
    Batch b;
    b.nsessions = nsessions;
    b.sessions.reset(nsessions ? new bm_pool_session_t[nsessions] : nullptr);
    b.accounts.reset(nsessions ? new uint32_t[nsessions] : nullptr);
    b.weights.reset(nsessions ? new uint64_t[nsessions] : nullptr);
    for (size_t s = 0; s < nsessions; ++s) {
        for (auto& x : b.sessions[s].extranonce1) x = rnd8();
        std::memset(b.sessions[s].target, s % 3 == 2 ? 0x00 : 0xFF, 32);
        b.accounts[s] = (uint32_t)(s == 0 ? rows - 1 : rnd32() % rows);
        b.weights[s] = s % 2 ? rnd64() : (1ull << 63) + s;
    }
    b.n = n;
    b.submits.reset(n ? new bm_jobs_submit_t[n] : nullptr);
    for (size_t i = 0; i < n; ++i) {
        bm_jobs_submit_t& s = b.submits[i];
        const uint32_t r = rnd32() % 16;
        s.job = (uint32_t)(rnd32() % o.njobs);
        if (r == 0) s.job = 0xFFFFFFFFu;
        const uint32_t size2 = s.job < o.njobs ? o.jobs[s.job].job.extranonce2_size : 1;
        s.extranonce2 = size2 >= 8 ? rnd64() : rnd64() & ((1ull << (8 * size2)) - 1);
        if (r == 1 && size2 < 8) s.extranonce2 |= 1ull << (8 * size2);  // does not fit
        s.ntime = s.job < o.njobs ? o.jobs[s.job].ntime_lo + (rnd32() % 4) - 1 : rnd32();
        s.nonce = rnd32();
        s.version = rnd32();
        s.session = r == 2 ? (uint32_t)nsessions : r == 3 ? 0xFFFFFFFFu : (uint32_t)(rnd32() % (nsessions ? nsessions : 1));
        s.reserved = rnd32();
        if (i > 2 && r >= 12) s = b.submits[rnd32() % i];  // a repeat: a duplicate where it is eligible
    }
    return b;
}

using Row = std::array<uint64_t, 8>;
using Key = std::array<uint8_t, 32>;
const Row kEmpty = {0, 0, 0, 0, 0, 0, 0, ~0ull};

// The model: bm_jobs_verify_cpu's verdicts, a std::set of hashes, a std::map of rows.
struct Model {
    std::map<uint32_t, Row> rows;
    std::set<Key> seen;
    bool with_set = false;
    bm_ledger_result_t step(const OwnedJobs& o, const Batch& b, bool identity, bool ones,
                            std::vector<bm_job_verdict_t>& v) {
        v.assign(b.n, bm_job_verdict_t());
        bm_pool_verify_result_t p;
        expect(bm_jobs_verify_cpu(o.jobs.get(), o.njobs, b.sessions.get(), b.nsessions, b.submits.get(), b.n,
                                  b.n ? v.data() : nullptr, &p) == BM_OK, "the plain verdicts");
        bm_ledger_result_t r;
        std::memset(&r, 0, sizeof r);
        r.n = b.n;
        for (size_t i = 0; i < b.n; ++i) {
            uint32_t& st = v[i].status;
            if (with_set && (st & (BM_SUBMIT_SHARE | BM_SUBMIT_BLOCK)) && !(st & BM_SUBMIT_INVALID)) {
                Key k;
                std::memcpy(k.data(), v[i].hash, 32);
                if (!seen.insert(k).second)
                    st |= BM_SUBMIT_DUPLICATE;
                else
                    ++r.recorded;
            }
            r.shares += (st & BM_SUBMIT_SHARE) ? 1 : 0, r.blocks += (st & BM_SUBMIT_BLOCK) ? 1 : 0;
            r.invalid += (st & BM_SUBMIT_INVALID) ? 1 : 0, r.ntime += (st & BM_SUBMIT_NTIME) ? 1 : 0;
            r.duplicates += (st & BM_SUBMIT_DUPLICATE) ? 1 : 0;
            const uint32_t s = b.submits[i].session;
            if (s >= b.nsessions) {
                ++r.unattributed;
                continue;
            }
            Row& row = rows.emplace(identity ? s : b.accounts[s], kEmpty).first->second;
            const int cls = (st & BM_SUBMIT_INVALID) ? 5 : (st & BM_SUBMIT_NTIME) ? 3 : (st & BM_SUBMIT_DUPLICATE) ? 4
                            : (st & (BM_SUBMIT_SHARE | BM_SUBMIT_BLOCK)) ? 0 : 2;
            ++row[cls];
            if (cls != 0) continue;
            const uint64_t w = ones ? 1 : b.weights[s];
            uint64_t top = 0;
            for (int k = 0; k < 8; ++k) top = (top << 8) | v[i].hash[k];
            row[1] += (st & BM_SUBMIT_BLOCK) ? 1 : 0;
            row[6] += w;
            row[7] = top < row[7] ? top : row[7];
            ++r.credited;
            r.work += w;
        }
        r.count = with_set ? seen.size() : 0;
        return r;
    }
};

// Every row of the ledger, read into an exactly-sized buffer, against the model.
void expect_rows(bm_ledger_t* ledger, const Model& m, size_t rows, const char* what) {
    std::unique_ptr<bm_ledger_row_t[]> got(new bm_ledger_row_t[rows]);
    expect(bm_ledger_read(ledger, 0, rows, got.get()) == BM_OK, what);
    for (size_t i = 0; i < rows; ++i) {
        const auto it = m.rows.find((uint32_t)i);
        const Row& want = it == m.rows.end() ? kEmpty : it->second;
        if (std::memcmp(&got[i], want.data(), 64) != 0) {
            expect(false, what);
            return;
        }
    }
}

void one_call(bm_ledger_t* ledger, bm_share_set_t* set, Model& m, const OwnedJobs& o, const Batch& b, size_t rows,
              bool identity, bool ones) {
    std::vector<bm_job_verdict_t> want;
    const bm_ledger_result_t wr = m.step(o, b, identity, ones, want);
    std::unique_ptr<bm_job_verdict_t[]> got(b.n ? new bm_job_verdict_t[b.n] : nullptr);
    bm_ledger_result_t r;
    std::memset(&r, 0x5A, sizeof r);
    const int rc = bm_ledger_verify_jobs(ledger, set, o.jobs.get(), o.njobs, b.sessions.get(), b.nsessions,
                                         identity ? nullptr : b.accounts.get(), ones ? nullptr : b.weights.get(),
                                         b.submits.get(), b.n, got.get(), &r);
    expect(rc == BM_OK, "the call succeeds");
    expect(b.n == 0 || std::memcmp(got.get(), want.data(), b.n * sizeof(bm_job_verdict_t)) == 0, "every verdict");
    expect(std::memcmp(&r, &wr, sizeof r) == 0, "the result");
    expect_rows(ledger, m, rows, "every row");
}

void scenarios() {
    const OwnedJobs o = make_jobs(kShapes);
    for (int with_set = 0; with_set < 2; ++with_set) {
        const size_t rows = 11;
        bm_ledger_t* ledger = nullptr;
        bm_share_set_t* set = nullptr;
        expect(bm_ledger_create_cpu(rows, &ledger) == BM_OK, "create");
        if (with_set) expect(bm_share_set_create_cpu(4096, &set) == BM_OK, "create a set");
        Model m;
        m.with_set = with_set != 0;
        for (size_t n : {0u, 1u, 2u, 63u, 64u, 65u, 200u, 700u}) {
            const Batch b = make_batch(o, 29, rows, n);
            one_call(ledger, set, m, o, b, rows, false, false);
        }
        {  // the identity and ones; no sessions at all
            const Batch b = make_batch(o, rows, rows, 150);
            one_call(ledger, set, m, o, b, rows, true, true);
            one_call(ledger, set, m, o, b, rows, true, false);
            const Batch none = make_batch(o, 0, rows, 20);
            one_call(ledger, set, m, o, none, rows, true, true);
        }
        // drain a middle range into an exactly-sized buffer: the model's rows, then empty; the neighbours stay
        {
            std::unique_ptr<bm_ledger_row_t[]> out(new bm_ledger_row_t[4]);
            expect(bm_ledger_drain(ledger, 3, 4, out.get()) == BM_OK, "drain");
            for (uint32_t i = 3; i < 7; ++i) {
                const auto it = m.rows.find(i);
                const Row& want = it == m.rows.end() ? kEmpty : it->second;
                expect(std::memcmp(&out[i - 3], want.data(), 64) == 0, "drain returns the rows");
                m.rows.erase(i);
            }
            expect_rows(ledger, m, rows, "drain empties exactly its range");
            expect(bm_ledger_drain(ledger, rows, 0, nullptr) == BM_OK && bm_ledger_read(ledger, 0, 0, nullptr) == BM_OK,
                   "empty ranges");
        }
        // wrap-around: 2^63 and 2^63 + 5 on one row
        {
            Batch b = make_batch(o, 2, rows, 2);
            std::memset(b.sessions[0].target, 0xFF, 32), std::memset(b.sessions[1].target, 0xFF, 32);
            b.accounts[0] = b.accounts[1] = 10;
            b.weights[0] = 1ull << 63, b.weights[1] = (1ull << 63) + 5;
            for (uint32_t i = 0; i < 2; ++i) {
                bm_jobs_submit_t& s = b.submits[i];
                s.job = 2, s.session = i, s.extranonce2 = i, s.ntime = 7, s.nonce = rnd32();
            }
            bm_ledger_row_t before, after;
            expect(bm_ledger_read(ledger, 10, 1, &before) == BM_OK, "read one row");
            one_call(ledger, set, m, o, b, rows, false, false);
            expect(bm_ledger_read(ledger, 10, 1, &after) == BM_OK, "read one row");
            expect(after.work == before.work + 5 && after.accepted == before.accepted + 2, "work wraps modulo 2^64");
        }
        expect(bm_ledger_clear(ledger) == BM_OK, "clear");
        m.rows.clear();
        expect_rows(ledger, m, rows, "clear empties every row");
        {
            const Batch b = make_batch(o, 29, rows, 100);
            one_call(ledger, set, m, o, b, rows, false, false);
        }
        bm_share_set_destroy(set);
        bm_ledger_destroy(ledger);
    }
}

void refusals() {
    const OwnedJobs o = make_jobs(kShapes);
    const size_t rows = 4;
    bm_ledger_t* ledger = nullptr;
    bm_share_set_t* set = nullptr;
    expect(bm_ledger_create_cpu(0, &ledger) == BM_EINVAL && bm_ledger_create_cpu(BM_MAX_LEDGER_ROWS + 1, &ledger) == BM_EINVAL &&
               bm_ledger_create_cpu(1, nullptr) == BM_EINVAL && ledger == nullptr, "creation refusals");
    expect(bm_ledger_create_cpu(rows, &ledger) == BM_OK && bm_share_set_create_cpu(3, &set) == BM_OK, "create");
    Model m;
    m.with_set = true;
    Batch b = make_batch(o, 4, rows, 3);
    for (uint32_t i = 0; i < 3; ++i) {  // three distinct accepted shares: the set is full
        bm_jobs_submit_t& s = b.submits[i];
        s.job = 2, s.session = i % 2, s.extranonce2 = i, s.ntime = 7;
    }
    one_call(ledger, set, m, o, b, rows, false, false);
    uint64_t count = 0;
    expect(bm_share_set_count(set, &count, nullptr) == BM_OK && count == 3, "the set is full");

    std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[3]);
    bm_ledger_result_t r;
    auto canaries = [&] {
        std::memset(v.get(), 0xA5, 3 * sizeof(bm_job_verdict_t));
        std::memset(&r, 0x5A, sizeof r);
    };
    auto intact = [&](const char* what) {
        bool ok = true;
        for (size_t i = 0; i < 3 * sizeof(bm_job_verdict_t); ++i) ok = ok && reinterpret_cast<uint8_t*>(v.get())[i] == 0xA5;
        for (size_t i = 0; i < sizeof r; ++i) ok = ok && reinterpret_cast<uint8_t*>(&r)[i] == 0x5A;
        expect(ok, what);
        expect_rows(ledger, m, rows, what);
        expect(bm_share_set_count(set, &count, nullptr) == BM_OK && count == 3, what);
    };
    auto call = [&](bm_ledger_t* l, bm_share_set_t* s, const Batch& x, const uint32_t* acc, bm_job_verdict_t* out,
                    bm_ledger_result_t* res) {
        return bm_ledger_verify_jobs(l, s, o.jobs.get(), o.njobs, x.sessions.get(), x.nsessions, acc, x.weights.get(),
                                     x.submits.get(), x.n, out, res);
    };
    canaries();
    Batch fresh = make_batch(o, 4, rows, 3);
    for (uint32_t i = 0; i < 3; ++i) {
        bm_jobs_submit_t& s = fresh.submits[i];
        s.job = 2, s.session = 0, s.extranonce2 = 100 + i, s.ntime = 7;
    }
    std::memset(fresh.sessions[0].target, 0xFF, 32);
    expect(call(ledger, set, fresh, fresh.accounts.get(), v.get(), &r) == BM_EFULL, "BM_EFULL from the set");
    intact("BM_EFULL changes nothing");
    fresh.accounts[3] = (uint32_t)rows;  // the last session's, which no submission names
    expect(call(ledger, set, fresh, fresh.accounts.get(), v.get(), &r) == BM_EINVAL, "an account equal to rows");
    expect(call(ledger, nullptr, fresh, fresh.accounts.get(), v.get(), &r) == BM_EINVAL, "an account equal to rows, no set");
    fresh.accounts[3] = 0;
    const Batch wide = make_batch(o, rows + 1, rows, 3);
    expect(call(ledger, nullptr, wide, nullptr, v.get(), &r) == BM_EINVAL, "the identity with more sessions than rows");
    expect(call(nullptr, nullptr, fresh, fresh.accounts.get(), v.get(), &r) == BM_EINVAL, "a NULL ledger");
    expect(call(ledger, nullptr, fresh, fresh.accounts.get(), nullptr, &r) == BM_EINVAL, "NULL verdicts");
    expect(call(ledger, nullptr, fresh, fresh.accounts.get(), v.get(), nullptr) == BM_EINVAL, "a NULL result");
    {
        OwnedJobs bad = make_jobs(kShapes);
        bad.jobs[1].job.nbranch = 33;
        expect(bm_ledger_verify_jobs(ledger, set, bad.jobs.get(), bad.njobs, fresh.sessions.get(), fresh.nsessions,
                                     fresh.accounts.get(), fresh.weights.get(), fresh.submits.get(), fresh.n, v.get(),
                                     &r) == BM_EINVAL, "a malformed job");
    }
    bm_ledger_row_t out[2];
    std::memset(out, 0xA5, sizeof out);
    expect(bm_ledger_read(ledger, 3, 2, out) == BM_EINVAL && bm_ledger_drain(ledger, 3, 2, out) == BM_EINVAL &&
               bm_ledger_read(ledger, rows + 1, 0, out) == BM_EINVAL && bm_ledger_drain(ledger, ~(size_t)0, 2, out) == BM_EINVAL &&
               bm_ledger_read(ledger, 0, 1, nullptr) == BM_EINVAL && bm_ledger_read(nullptr, 0, 1, out) == BM_EINVAL,
           "ranges past the end");
    expect(reinterpret_cast<uint8_t*>(out)[0] == 0xA5 && reinterpret_cast<uint8_t*>(out)[127] == 0xA5, "a refused read writes nothing");
    expect(bm_ledger_set_peel(ledger, 65) == BM_EINVAL && bm_ledger_set_peel(ledger, 64) == BM_OK &&
               bm_ledger_set_peel(ledger, 0) == BM_OK && bm_ledger_set_peel(nullptr, 1) == BM_EINVAL, "peel rounds");
    uint64_t nrows = 0;
    expect(bm_ledger_rows(ledger, &nrows) == BM_OK && nrows == rows && bm_ledger_rows(ledger, nullptr) == BM_EINVAL &&
               bm_ledger_rows(nullptr, &nrows) == BM_EINVAL && bm_ledger_clear(nullptr) == BM_EINVAL, "rows and clear");
    intact("the refusals change nothing");
    // an empty batch is legal: zeros and the set's count
    expect(bm_ledger_verify_jobs(ledger, set, o.jobs.get(), o.njobs, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &r) == BM_OK &&
               r.n == 0 && r.count == 3 && r.credited == 0 && r.unattributed == 0 && r.work == 0, "an empty batch");
    expect_rows(ledger, m, rows, "an empty batch changes nothing");
    bm_ledger_destroy(nullptr);
    bm_share_set_destroy(set);
    bm_ledger_destroy(ledger);
}

}  // namespace

int main() {
    scenarios();
    refusals();
    if (fails) {
        std::printf("%d failure(s)\n", fails);
        return 1;
    }
    std::printf("ledger check ok\n");
    return 0;
}
