// sessions_check.cpp -- stand-alone CPU check of the session table's host code
// (csrc/bm_sessions.cpp, csrc/bm_sessions_host.hpp, csrc/bm_sessions_args.hpp) under
// sanitizers, tools/ledger_check.cpp's recipe: bm_target_from_difficulty_fx and the
// multiword arithmetic the kernels use (compiled for the host here) against a 128-bit
// restatement; the CPU table on exactly-sized heap buffers for `index`, `init`, the
// arrays bm_sessions_get fills, `submits`, `verdicts` and `changes`, against
// bm_ledger_verify_jobs on the arrays it returned and against the rule restated;
// BM_EFULL one entry short and the refusals, with canaries.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/sessions_check.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_sessions.cpp distributed_bitcoin_minter_amd/csrc/bm_ledger.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_share_set.cpp distributed_bitcoin_minter_amd/csrc/bm_job.cpp
//     -o sessions_check && ./sessions_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bm_sessions_args.hpp"
#include "btcminer.h"

namespace {

using u128 = unsigned __int128;
int fails = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++fails;
    }
}

uint32_t rng_state = 0x2545F491u;
uint8_t rnd8() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 16);
}
uint32_t rnd32() { return ((uint32_t)rnd8() << 24) | ((uint32_t)rnd8() << 16) | ((uint32_t)rnd8() << 8) | rnd8(); }
uint64_t rnd64() { return ((uint64_t)rnd32() << 32) | rnd32(); }
// a value of a random width, so that small and large operands both occur
uint64_t rnd_width() { return rnd64() >> (rnd32() % 64); }

template <class T>
std::unique_ptr<T[]> exact(size_t n) {  // exactly n entries on the heap: the sanitizer sees any access past them
    return std::unique_ptr<T[]>(n ? new T[n] : nullptr);
}

// T(d), restated: schoolbook division of 0xffff * 2^240 by d over 32-bit digits.
void target_ref(uint64_t d, uint8_t out[32]) {
    u128 rem = 0;
    for (int i = 0; i < 8; ++i) {
        const uint32_t digit = i == 0 ? 0xffff0000u : 0u;
        rem = (rem << 32) | digit;
        const uint32_t q = (uint32_t)(rem / d);
        rem %= d;
        out[4 * i] = (uint8_t)(q >> 24), out[4 * i + 1] = (uint8_t)(q >> 16);
        out[4 * i + 2] = (uint8_t)(q >> 8), out[4 * i + 3] = (uint8_t)q;
    }
}

const uint64_t kListed[] = {1, 2, 3, 0xffff, 0x10000, 1ull << 32, (1ull << 32) + 1, (1ull << 53) - 1, 1ull << 63, ~0ull};

void targets() {
    std::vector<uint64_t> ds(kListed, kListed + 10);
    for (int i = 0; i < 2000; ++i) ds.push_back(rnd_width() | 1u);
    for (const uint64_t d : ds) {
        auto got = exact<uint8_t>(32);
        uint8_t want[32], words[32];
        expect(bm_target_from_difficulty_fx(d, got.get()) == BM_OK, "T succeeds");
        target_ref(d, want);
        expect(std::memcmp(got.get(), want, 32) == 0, "T against the schoolbook division");
        uint64_t q[4];
        bm::target_words_fx(d, q);
        for (int i = 0; i < 4; ++i)
            for (int b = 0; b < 8; ++b) words[8 * i + b] = (uint8_t)(q[i] >> (56 - 8 * b));
        expect(std::memcmp(words, want, 32) == 0, "the multiword T against the schoolbook division");
        if (d < (1ull << 53)) {
            uint8_t dbl[32];
            expect(bm_target_from_difficulty((double)d / 4294967296.0, dbl) == BM_OK && std::memcmp(dbl, want, 32) == 0,
                   "T against the double function below 2^53");
        }
    }
    uint8_t t[32];
    std::memset(t, 0xA5, 32);
    expect(bm_target_from_difficulty_fx(0, t) == BM_EINVAL && t[0] == 0xA5 && t[31] == 0xA5, "T refuses 0");
    expect(bm_target_from_difficulty_fx(1, nullptr) == BM_EINVAL, "T refuses NULL");
    expect(bm_target_from_difficulty_fx(1ull << 32, t) == BM_OK && t[3] == 0 && t[4] == 0xff && t[5] == 0xff && t[6] == 0,
           "2^32 is difficulty 1");
}

// The rule, restated with a 128-bit type -> evaluated?, and the new difficulty (old where unchanged).
bool rule_ref(const bm_vardiff_policy_t& p, uint64_t now, uint64_t old, uint64_t since, uint64_t accepted, uint64_t& nw) {
    const uint64_t elapsed = now >= since ? now - since : 0;
    nw = old;
    if (!(elapsed >= p.window_ms || (p.burst && accepted >= p.burst))) return false;
    const u128 N = (u128)std::min<uint64_t>(accepted, 0xFFFFFFFFull) * p.target_ms;
    // old * N is below 2^64 * 2^32 * 2^32: inside 128 bits
    const u128 D = std::max<uint64_t>(elapsed, 1);
    const u128 ideal = (u128)old * N / D;
    const u128 lo = std::max<uint64_t>(1, old / p.max_down);
    const u128 hi = std::min<u128>((u128)old * p.max_up, ~0ull);
    u128 v = std::min(std::max(ideal, lo), hi);
    v = std::min<u128>(std::max<u128>(v, p.min_difficulty_fx), p.max_difficulty_fx);
    const uint64_t c = (uint64_t)v;
    const u128 diff = c > old ? c - old : old - c;
    if (diff * 1000 > (u128)old * p.band_permille) nw = c;
    return true;
}

bm_vardiff_policy_t random_policy() {
    bm_vardiff_policy_t p;
    p.target_ms = 1 + rnd_width() % 0xFFFFFFFFull;
    p.window_ms = rnd32() % 4 ? rnd_width() % 100000 : rnd_width();
    p.min_difficulty_fx = 1 + (rnd32() % 3 ? 0 : rnd_width() % 100000);
    p.max_difficulty_fx = rnd32() % 3 ? ~0ull : p.min_difficulty_fx + rnd_width();
    if (p.max_difficulty_fx < p.min_difficulty_fx) p.max_difficulty_fx = ~0ull;
    p.burst = rnd32() % 2 ? 0 : rnd32() % 50;
    p.band_permille = rnd32() % 1001;
    p.max_up = 1 + (rnd32() % 4 ? rnd32() % 8 : rnd32());
    p.max_down = 1 + (rnd32() % 4 ? rnd32() % 8 : rnd32());
    return p;
}

bm::SessionsRetargetArgs args_of(const bm_vardiff_policy_t& p, uint64_t now) {
    bm::SessionsRetargetArgs A;
    std::memset(&A, 0, sizeof A);
    A.now_ms = now, A.target_ms = p.target_ms, A.window_ms = p.window_ms;
    A.min_fx = p.min_difficulty_fx, A.max_fx = p.max_difficulty_fx;
    A.burst = p.burst, A.band_permille = p.band_permille, A.max_up = p.max_up, A.max_down = p.max_down;
    return A;
}

void multiword() {
    for (int i = 0; i < 20000; ++i) {
        const uint64_t a = rnd_width(), b = rnd_width();
        const bm::U128 m = bm::mul_64x64(a, b);
        const u128 want = (u128)a * b;
        expect(m.hi == (uint64_t)(want >> 64) && m.lo == (uint64_t)want, "mul_64x64");
        const uint64_t d = rnd_width() | 1u, hi = rnd64() % d, lo = rnd64();
        uint64_t rem;
        const uint64_t q = bm::div_128by64(hi, lo, d, &rem);
        const u128 num = ((u128)hi << 64) | lo;
        expect(q == (uint64_t)(num / d) && rem == (uint64_t)(num % d), "div_128by64");
    }
    for (int i = 0; i < 20000; ++i) {
        const bm_vardiff_policy_t p = random_policy();
        const uint64_t now = rnd_width(), since = rnd32() % 8 ? now - std::min<uint64_t>(now, rnd_width() % 200000) : rnd_width();
        const uint64_t old = i % 7 == 0 ? ~0ull - rnd32() % 3 : (rnd_width() | 1u);
        const uint64_t accepted = rnd32() % 16 ? rnd_width() % 1000 : rnd_width();
        const bm::SessionsRetargetArgs A = args_of(p, now);
        uint64_t want;
        const bool ev = rule_ref(p, now, old, since, accepted, want);
        expect(bm::vardiff_evaluated(A, since, accepted) == ev, "vardiff_evaluated");
        if (ev) expect(bm::vardiff_new(A, old, since, accepted) == want, "vardiff_new");
    }
}

struct OwnedJob {
    std::unique_ptr<uint8_t[]> c1, c2;
    bm_pool_job_t job;
};

// One job whose block target is 0xffff << 240: nearly every hash is a BLOCK.
void make_job(OwnedJob& o) {
    std::memset(&o.job, 0, sizeof o.job);
    o.c1 = exact<uint8_t>(33), o.c2 = exact<uint8_t>(50);
    for (int i = 0; i < 33; ++i) o.c1[i] = rnd8();
    for (int i = 0; i < 50; ++i) o.c2[i] = rnd8();
    o.job.job.coinb1 = o.c1.get(), o.job.job.coinb1_len = 33;
    o.job.job.coinb2 = o.c2.get(), o.job.job.coinb2_len = 50;
    o.job.job.extranonce1_len = 8, o.job.job.extranonce2_size = 4;
    for (auto& b : o.job.job.prevhash) b = rnd8();
    o.job.job.version = rnd32();
    o.job.job.nbits = 0x2100ffffu;
    o.job.ntime_lo = 0, o.job.ntime_hi = 0xffffffffu;
}

struct Snapshot {
    std::vector<uint8_t> bytes;
    uint64_t count = 0;
    bool operator==(const Snapshot& o) const { return count == o.count && bytes == o.bytes; }
};

// Everything the table holds, through exactly-sized buffers.
Snapshot snapshot(bm_sessions_t* t) {
    Snapshot s;
    uint64_t cap = 0;
    expect(bm_sessions_count(t, &s.count, &cap) == BM_OK, "count");
    auto ses = exact<bm_pool_session_t>(cap);
    auto acc = exact<uint32_t>(cap);
    auto wgt = exact<uint64_t>(cap);
    auto st = exact<bm_session_state_t>(cap);
    expect(bm_sessions_get(t, 0, cap, ses.get(), acc.get(), wgt.get(), st.get()) == BM_OK, "get");
    auto put = [&](const void* p, size_t n) {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        s.bytes.insert(s.bytes.end(), b, b + n);
    };
    put(ses.get(), cap * sizeof(bm_pool_session_t)), put(acc.get(), cap * 4), put(wgt.get(), cap * 8);
    put(st.get(), cap * sizeof(bm_session_state_t));
    return s;
}

void table() {
    OwnedJob o;
    make_job(o);
    const size_t capacity = 70, rows = 5;
    bm_sessions_t* t = nullptr;
    bm_ledger_t *ledger = nullptr, *witness = nullptr;
    bm_share_set_t *set = nullptr, *wset = nullptr;
    expect(bm_sessions_create_cpu(capacity, &t) == BM_OK && bm_ledger_create_cpu(rows, &ledger) == BM_OK &&
               bm_ledger_create_cpu(rows, &witness) == BM_OK && bm_share_set_create_cpu(4096, &set) == BM_OK &&
               bm_share_set_create_cpu(4096, &wset) == BM_OK, "create");
    // set through an exactly-sized index with repeats: the later entry wins
    const size_t k = 40;
    auto index = exact<uint32_t>(k);
    auto init = exact<bm_session_init_t>(k);
    std::vector<bm_session_init_t> last(capacity);
    std::vector<bool> touched(capacity, false);
    for (size_t j = 0; j < k; ++j) {
        index[j] = j < 3 ? (uint32_t)(capacity - 1) : rnd32() % capacity;
        std::memset(&init[j], 0, sizeof init[j]);
        for (auto& b : init[j].extranonce1) b = rnd8();
        init[j].difficulty_fx = j % 5 == 4 ? 0 : rnd_width() | 1u;
        init[j].account = rnd32() % rows;
        last[index[j]] = init[j], touched[index[j]] = true;
    }
    expect(bm_sessions_set(t, index.get(), k, init.get(), 1000) == BM_OK, "set");
    uint64_t count = 0;
    expect(bm_sessions_count(t, &count, nullptr) == BM_OK && count == capacity, "count is 1 + the highest index");
    auto ses = exact<bm_pool_session_t>(capacity);
    auto acc = exact<uint32_t>(capacity);
    auto wgt = exact<uint64_t>(capacity);
    auto st = exact<bm_session_state_t>(capacity);
    expect(bm_sessions_get(t, 0, capacity, ses.get(), acc.get(), wgt.get(), st.get()) == BM_OK, "get");
    for (size_t s = 0; s < capacity; ++s) {
        uint8_t want[32] = {};
        if (touched[s] && last[s].difficulty_fx) target_ref(last[s].difficulty_fx, want);
        const bool ok = touched[s] ? std::memcmp(ses[s].extranonce1, last[s].extranonce1, 8) == 0 && acc[s] == last[s].account &&
                                         wgt[s] == last[s].difficulty_fx && st[s].difficulty_fx == wgt[s] && st[s].since_ms == 1000
                                   : acc[s] == 0 && wgt[s] == 0 && st[s].since_ms == 0;
        expect(ok && std::memcmp(ses[s].target, want, 32) == 0 && st[s].accepted == 0 && st[s].retargets == 0, "a slot after set");
    }
    // verify, with a ledger and a set and without either, against bm_ledger_verify_jobs on those arrays
    std::vector<uint64_t> tally(capacity, 0);
    for (int round = 0; round < 4; ++round) {
        const size_t n = round == 3 ? 1 : 150 + round;
        auto subs = exact<bm_jobs_submit_t>(n);
        for (size_t i = 0; i < n; ++i) {
            bm_jobs_submit_t& s = subs[i];
            s.extranonce2 = rnd32(), s.ntime = rnd32(), s.nonce = rnd32(), s.version = rnd32();
            s.session = rnd32() % 9 == 0 ? (uint32_t)capacity + rnd32() % 3 : rnd32() % capacity;
            s.job = rnd32() % 11 == 0 ? 1 : 0, s.reserved = rnd32();
            if (i > 3 && rnd32() % 6 == 0) s = subs[rnd32() % i];
        }
        const bool with = round % 2 == 0;
        auto got = exact<bm_job_verdict_t>(n);
        auto want = exact<bm_job_verdict_t>(n);
        bm_ledger_result_t r, wr;
        expect(bm_sessions_verify_jobs(t, with ? ledger : nullptr, with ? set : nullptr, &o.job, 1, subs.get(), n, got.get(), &r) == BM_OK,
               "verify through the table");
        bm_ledger_t* scratch = nullptr;
        expect(bm_ledger_create_cpu(rows, &scratch) == BM_OK, "a scratch ledger");
        expect(bm_ledger_verify_jobs(with ? witness : scratch, with ? wset : nullptr, &o.job, 1, ses.get(), capacity, acc.get(),
                                     wgt.get(), subs.get(), n, want.get(), &wr) == BM_OK, "verify on the arrays");
        bm_ledger_destroy(scratch);
        expect(std::memcmp(got.get(), want.get(), n * sizeof(bm_job_verdict_t)) == 0 && std::memcmp(&r, &wr, sizeof r) == 0,
               "the verdicts and the result");
        for (size_t i = 0; i < n; ++i) {
            const uint32_t stt = got[i].status;
            const bool accepted = !(stt & (BM_SUBMIT_INVALID | BM_SUBMIT_NTIME | BM_SUBMIT_DUPLICATE)) &&
                                  (stt & (BM_SUBMIT_SHARE | BM_SUBMIT_BLOCK));
            if (subs[i].session < capacity && accepted) ++tally[subs[i].session];
        }
    }
    {
        auto a = exact<bm_ledger_row_t>(rows);
        auto b = exact<bm_ledger_row_t>(rows);
        expect(bm_ledger_read(ledger, 0, rows, a.get()) == BM_OK && bm_ledger_read(witness, 0, rows, b.get()) == BM_OK &&
                   std::memcmp(a.get(), b.get(), rows * sizeof(bm_ledger_row_t)) == 0, "the ledger's rows");
        expect(bm_sessions_get(t, 0, capacity, nullptr, nullptr, nullptr, st.get()) == BM_OK, "the states alone");
        uint64_t total = 0;
        for (size_t s = 0; s < capacity; ++s) {
            expect(st[s].accepted == tally[s], "the tally");
            total += tally[s];
        }
        expect(total > 100, "the batches tallied");
    }
    // retarget: the rule restated, one entry short first
    bm_vardiff_policy_t p = {1000, 5000, 1, ~0ull, 0, 0, 4, 4};
    const uint64_t now = 9000;
    std::vector<bm_vardiff_change_t> want;
    bm_vardiff_result_t wr = {0, 0, 0, 0, 0};
    for (size_t s = 0; s < capacity; ++s) {
        if (!st[s].difficulty_fx) continue;
        ++wr.open;
        uint64_t nw;
        if (!rule_ref(p, now, st[s].difficulty_fx, st[s].since_ms, st[s].accepted, nw)) continue;
        ++wr.evaluated;
        if (nw == st[s].difficulty_fx) continue;
        ++wr.changed, ++(nw > st[s].difficulty_fx ? wr.raised : wr.lowered);
        bm_vardiff_change_t c;
        std::memset(&c, 0, sizeof c);
        c.session = (uint32_t)s, c.old_fx = st[s].difficulty_fx, c.new_fx = nw;
        target_ref(nw, c.target);
        want.push_back(c);
    }
    expect(wr.changed >= 5, "the retarget has changes");
    {
        const Snapshot before = snapshot(t);
        const size_t cap = (size_t)wr.changed - 1;
        auto changes = exact<bm_vardiff_change_t>(cap);
        std::memset(changes.get(), 0xA5, cap * sizeof(bm_vardiff_change_t));
        bm_vardiff_result_t r;
        expect(bm_sessions_retarget(t, now, &p, changes.get(), cap, &r) == BM_EFULL && std::memcmp(&r, &wr, sizeof r) == 0,
               "one entry short: BM_EFULL and the exact counts");
        bool intact = true;
        for (size_t i = 0; i < cap * sizeof(bm_vardiff_change_t); ++i) intact = intact && reinterpret_cast<uint8_t*>(changes.get())[i] == 0xA5;
        expect(intact && snapshot(t) == before, "BM_EFULL changes nothing");
    }
    {
        const size_t cap = (size_t)wr.changed;
        auto changes = exact<bm_vardiff_change_t>(cap);
        bm_vardiff_result_t r;
        expect(bm_sessions_retarget(t, now, &p, changes.get(), cap, &r) == BM_OK && std::memcmp(&r, &wr, sizeof r) == 0,
               "cap == changed");
        expect(std::memcmp(changes.get(), want.data(), cap * sizeof(bm_vardiff_change_t)) == 0, "the change list");
        auto after = exact<bm_session_state_t>(capacity);
        expect(bm_sessions_get(t, 0, capacity, ses.get(), nullptr, wgt.get(), after.get()) == BM_OK, "get after the retarget");
        for (const bm_vardiff_change_t& c : want)
            expect(after[c.session].difficulty_fx == c.new_fx && wgt[c.session] == c.new_fx && after[c.session].retargets == 1 &&
                       after[c.session].since_ms == now && after[c.session].accepted == 0 &&
                       std::memcmp(ses[c.session].target, c.target, 32) == 0, "a changed slot");
    }
    // refusals, with canaries
    {
        const Snapshot before = snapshot(t);
        bm_job_verdict_t v[2];
        bm_ledger_result_t r;
        std::memset(v, 0xA5, sizeof v), std::memset(&r, 0x5A, sizeof r);
        bm_jobs_submit_t s = {};
        bm_ledger_t* small = nullptr;
        expect(bm_ledger_create_cpu(rows - 1, &small) == BM_OK, "a ledger one row short");
        expect(bm_sessions_verify_jobs(t, small, nullptr, &o.job, 1, &s, 1, v, &r) == BM_EINVAL, "an account past the rows");
        expect(bm_sessions_verify_jobs(nullptr, nullptr, nullptr, &o.job, 1, &s, 1, v, &r) == BM_EINVAL, "a NULL table");
        expect(bm_sessions_verify_jobs(t, nullptr, nullptr, &o.job, 1, &s, 1, nullptr, &r) == BM_EINVAL, "NULL verdicts");
        expect(bm_sessions_verify_jobs(t, nullptr, nullptr, &o.job, 1, &s, 1, v, nullptr) == BM_EINVAL, "a NULL result");
        bm_ledger_destroy(small);
        bool ok = true;
        for (size_t i = 0; i < sizeof v; ++i) ok = ok && reinterpret_cast<uint8_t*>(v)[i] == 0xA5;
        for (size_t i = 0; i < sizeof r; ++i) ok = ok && reinterpret_cast<uint8_t*>(&r)[i] == 0x5A;
        expect(ok, "the refusals write nothing");
        const uint32_t past = (uint32_t)capacity;
        bm_session_init_t one = {};
        one.difficulty_fx = 5;
        expect(bm_sessions_set(t, &past, 1, &one, 1) == BM_EINVAL && bm_sessions_set(t, nullptr, 1, nullptr, 1) == BM_EINVAL,
               "set refusals");
        bm_vardiff_result_t vr;
        bm_vardiff_change_t c;
        bm_vardiff_policy_t bad = p;
        bad.target_ms = 0;
        expect(bm_sessions_retarget(t, now, &bad, &c, 1, &vr) == BM_EINVAL, "target_ms = 0");
        bad = p, bad.target_ms = 1ull << 32;
        expect(bm_sessions_retarget(t, now, &bad, &c, 1, &vr) == BM_EINVAL, "target_ms = 2^32");
        bad = p, bad.min_difficulty_fx = 0;
        expect(bm_sessions_retarget(t, now, &bad, &c, 1, &vr) == BM_EINVAL, "min = 0");
        bad = p, bad.min_difficulty_fx = 9, bad.max_difficulty_fx = 8;
        expect(bm_sessions_retarget(t, now, &bad, &c, 1, &vr) == BM_EINVAL, "min > max");
        bad = p, bad.max_up = 0;
        expect(bm_sessions_retarget(t, now, &bad, &c, 1, &vr) == BM_EINVAL, "max_up = 0");
        bad = p, bad.max_down = 0;
        expect(bm_sessions_retarget(t, now, &bad, &c, 1, &vr) == BM_EINVAL, "max_down = 0");
        bad = p, bad.band_permille = 1001;
        expect(bm_sessions_retarget(t, now, &bad, &c, 1, &vr) == BM_EINVAL, "band = 1001");
        expect(bm_sessions_retarget(t, now, &p, nullptr, 1, &vr) == BM_EINVAL && bm_sessions_retarget(t, now, nullptr, &c, 1, &vr) == BM_EINVAL &&
                   bm_sessions_retarget(t, now, &p, &c, 1, nullptr) == BM_EINVAL, "NULL pointers");
        expect(bm_sessions_get(t, 1, capacity, nullptr, nullptr, nullptr, nullptr) == BM_EINVAL &&
                   bm_sessions_get(t, capacity + 1, 0, nullptr, nullptr, nullptr, nullptr) == BM_EINVAL, "ranges past the end");
        expect(snapshot(t) == before, "the refusals change nothing");
    }
    expect(bm_sessions_clear(t) == BM_OK && bm_sessions_count(t, &count, nullptr) == BM_OK && count == 0, "clear");
    {
        const Snapshot s = snapshot(t);
        expect(std::all_of(s.bytes.begin(), s.bytes.end(), [](uint8_t b) { return b == 0; }), "clear zeroes every slot");
    }
    bm_sessions_destroy(nullptr);
    bm_sessions_destroy(t);
    bm_ledger_destroy(ledger), bm_ledger_destroy(witness);
    bm_share_set_destroy(set), bm_share_set_destroy(wset);
}

}  // namespace

int main() {
    targets();
    multiword();
    table();
    if (fails) {
        std::printf("%d failure(s)\n", fails);
        return 1;
    }
    std::printf("sessions check ok\n");
    return 0;
}
