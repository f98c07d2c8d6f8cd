// pool_verify_check.cpp -- stand-alone CPU check of the pool verifier's host code
// (csrc/bm_job.hpp, csrc/bm_job.cpp) under sanitizers, tools/verify_check.cpp's
// recipe: field_words over all 8 x 8 x 4 (size1, size2, boff) combinations against
// a byte-wise restatement; what the GPU entry's host side prepares
// (host::pool_verify_prepare), replayed as a lane of pool_verify_kernel with the
// host compression, against bm_job_header; bm_pool_verify_cpu on exactly-sized heap
// buffers for the job, `sessions`, `submits` and `verdicts`; and the refusals, with
// canaries.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/pool_verify_check.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_job.cpp -o pool_verify_check && ./pool_verify_check
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

uint32_t rng_state = 0x2545F491u;
uint8_t rnd8() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 16);
}
uint32_t rnd32() { return ((uint32_t)rnd8() << 24) | ((uint32_t)rnd8() << 16) | ((uint32_t)rnd8() << 8) | rnd8(); }
uint64_t rnd64() { return ((uint64_t)rnd32() << 32) | rnd32(); }

std::vector<uint8_t> random_bytes(size_t n) {
    std::vector<uint8_t> v(n);
    for (auto& b : v) b = rnd8();
    return v;
}

// A heap copy of exactly n bytes (nullptr for none): the sanitizer sees any access past it.
std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
    std::unique_ptr<uint8_t[]> p(v.empty() ? nullptr : new uint8_t[v.size()]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size());
    return p;
}

// ---- field_words against its bytes ----
void field_words_cases() {
    bool ok = true;
    for (uint32_t size1 = 1; size1 <= 8; ++size1)
        for (uint32_t size2 = 1; size2 <= 8; ++size2)
            for (uint32_t boff = 0; boff < 4; ++boff)
                for (int round = 0; round < 4; ++round) {
                    uint8_t en1[8];
                    for (auto& b : en1) b = round == 0 ? 0x00 : round == 1 ? 0xFF : rnd8();
                    const uint64_t top = size2 == 8 ? UINT64_MAX : (1ull << (8 * size2)) - 1;
                    const uint64_t en2 = round == 0 ? top : round == 1 ? 0 : rnd64() & top;
                    // the 20-byte window, byte by byte: only the first size1 bytes of en1 count
                    uint8_t window[20] = {0};
                    for (uint32_t i = 0; i < size1; ++i) window[boff + i] = en1[i];
                    for (uint32_t i = 0; i < size2; ++i)
                        window[boff + size1 + i] = (uint8_t)(en2 >> (8 * (size2 - 1 - i)));
                    bm_pool_session_t s;
                    std::memcpy(s.extranonce1, en1, 8);
                    uint32_t e[bm::kFieldWords];
                    bm::field_words(bm::host::session_en1(s), size1, en2, size2, boff, e);
                    for (int k = 0; k < bm::kFieldWords; ++k) ok = ok && e[k] == bm::host::load_be32(window + 4 * k);
                    if (!ok) {
                        std::printf("field_words size1 %u size2 %u boff %u round %d\n", size1, size2, boff, round);
                        expect(false, "field_words gives the window's words");
                        return;
                    }
                }
    expect(ok, "field_words over every (size1, size2, boff)");
}

// A job that owns exactly-sized copies of its parts; its own extranonce1 pointer is NULL.
struct OwnedJob {
    std::vector<uint8_t> c1, c2, br;
    std::unique_ptr<uint8_t[]> p1, p2, pb;
    std::unique_ptr<bm_job_t> job;
};

// The field (size1 + size2 bytes) at byte `pos` of a coinbase of `total` bytes.
OwnedJob make_job(size_t pos, uint32_t size1, uint32_t size2, size_t total, size_t nbranch, uint32_t nbits) {
    OwnedJob o;
    o.c1 = random_bytes(pos);
    o.c2 = random_bytes(total - pos - size1 - size2);
    o.br = random_bytes(32 * nbranch);
    o.p1 = exact(o.c1), o.p2 = exact(o.c2), o.pb = exact(o.br);
    o.job.reset(new bm_job_t);
    std::memset(o.job.get(), 0, sizeof(bm_job_t));
    o.job->coinb1 = o.p1.get();
    o.job->coinb1_len = o.c1.size();
    o.job->extranonce1 = nullptr;  // ignored by the pool entries
    o.job->extranonce1_len = size1;
    o.job->extranonce2_size = size2;
    o.job->coinb2 = o.p2.get();
    o.job->coinb2_len = o.c2.size();
    o.job->branch = o.pb.get();
    o.job->nbranch = nbranch;
    for (auto& b : o.job->prevhash) b = rnd8();
    o.job->version = 0x20000000u;
    o.job->nbits = nbits;
    return o;
}

// The header of a submission by bm_job_header over a copy of the job that holds the session's extranonce1.
bool restated_header(const OwnedJob& o, const bm_pool_session_t& ses, const bm_pool_submit_t& s, uint8_t header[80]) {
    bm_job_t j = *o.job;
    std::vector<uint8_t> en1(ses.extranonce1, ses.extranonce1 + j.extranonce1_len);  // exactly its size
    j.extranonce1 = en1.data();
    if (bm_job_header(&j, s.extranonce2, s.ntime, s.version, header) != BM_OK) return false;
    bm::host::store_le32(header + 76, s.nonce);
    return true;
}

// The root a lane of pool_verify_kernel computes from what pool_verify_prepare made, with the host compression.
void lane_root(const bm::PoolVerifyArgs& A, const std::vector<uint32_t>& tail, const std::vector<uint32_t>& branch,
               const bm_pool_session_t& ses, uint64_t extranonce2, uint8_t root[32]) {
    uint32_t e[bm::kFieldWords];
    bm::field_words(bm::host::session_en1(ses), A.size1, extranonce2, A.size2, A.boff, e);
    uint32_t st[8], w[16];
    for (int k = 0; k < 8; ++k) st[k] = A.mid[k];
    for (uint32_t b = 0; b < A.nb; ++b) {
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t idx = 16 * b + k;
            w[k] = tail[idx];  // (a vector: a read past the template is caught)
            for (uint32_t i = 0; i < (uint32_t)bm::kFieldWords; ++i)
                if (idx == A.j0 + i) w[k] |= e[i];
        }
        bm::host::compress(st, w);
    }
    auto second = [&] {
        for (int k = 0; k < 8; ++k) w[k] = st[k];
        w[8] = 0x80000000u;
        for (int k = 9; k < 15; ++k) w[k] = 0;
        w[15] = 256;
        for (int k = 0; k < 8; ++k) st[k] = bm::kIV256[k];
        bm::host::compress(st, w);
    };
    second();
    for (uint32_t d = 0; d < A.depth; ++d) {
        for (int k = 0; k < 8; ++k) w[k] = st[k];
        for (int k = 0; k < 8; ++k) w[8 + k] = branch[8 * d + k];
        for (int k = 0; k < 8; ++k) st[k] = bm::kIV256[k];
        bm::host::compress(st, w);
        std::memset(w, 0, sizeof w);
        w[0] = 0x80000000u;
        w[15] = 512;
        bm::host::compress(st, w);
        second();
    }
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 4; ++b) root[4 * i + b] = (uint8_t)(st[i] >> (24 - 8 * b));
}

// One layout: bm_pool_verify_cpu on exactly-sized arrays against bm_job_header and the header's double hash, and
// the prepared template against bm_job_header's root.
void layout_case(size_t pos, uint32_t size1, uint32_t size2, size_t total, size_t nbranch) {
    OwnedJob o = make_job(pos, size1, size2, total, nbranch, 0x1f00ffffu);
    const uint64_t top = size2 == 8 ? UINT64_MAX : (1ull << (8 * size2)) - 1;
    const size_t n = 6, nses = 3;
    std::unique_ptr<bm_pool_session_t[]> ses(new bm_pool_session_t[nses]);
    for (size_t s = 0; s < nses; ++s) {
        for (auto& b : ses[s].extranonce1) b = s == 0 ? 0x00 : s == 1 ? 0xFF : rnd8();
        std::memset(ses[s].target, 0xFF, 32);
        ses[s].target[0] = s == 0 ? 0x7F : s == 1 ? 0x00 : 0xFF;  // about a half, almost none, all
    }
    std::unique_ptr<bm_pool_submit_t[]> subs(new bm_pool_submit_t[n]);
    std::unique_ptr<bm_job_verdict_t[]> verdicts(new bm_job_verdict_t[n]);
    const uint64_t en2s[n] = {0, top, rnd64() & top, 0x0102030405060708ull & top, rnd64() & top, 1};
    for (size_t i = 0; i < n; ++i) {
        subs[i].extranonce2 = en2s[i];
        subs[i].ntime = i % 2 ? 1000 + (uint32_t)i : rnd32() | 0x80000000u;
        subs[i].nonce = rnd32();
        subs[i].version = rnd32();
        subs[i].session = (uint32_t)(i % nses);
    }
    const uint32_t lo = 1000, hi = 1003;
    bm_pool_verify_result_t out;
    expect(bm_pool_verify_cpu(o.job.get(), ses.get(), nses, subs.get(), n, lo, hi, verdicts.get(), &out) == BM_OK,
           "a legal batch");
    uint8_t bt[32];
    expect(bm::host::target_from_bits(o.job->nbits, bt), "the case's nbits decodes");
    uint64_t shares = 0, blocks = 0, ntimes = 0;
    bool same = true;
    for (size_t i = 0; i < n; ++i) {
        uint8_t header[80], h[32];
        expect(restated_header(o, ses[subs[i].session], subs[i], header), "the header of a legal submission");
        bm::host::header_hash_msb(header, subs[i].nonce, h);
        uint32_t st = 0;
        if (std::memcmp(h, ses[subs[i].session].target, 32) <= 0) st |= BM_SUBMIT_SHARE, ++shares;
        if (std::memcmp(h, bt, 32) <= 0) st |= BM_SUBMIT_BLOCK, ++blocks;
        if (subs[i].ntime < lo || subs[i].ntime > hi) st |= BM_SUBMIT_NTIME, ++ntimes;
        same = same && std::memcmp(h, verdicts[i].hash, 32) == 0 && verdicts[i].status == st && verdicts[i].reserved == 0;
    }
    if (!same) std::printf("layout pos %zu sizes %u %u total %zu depth %zu\n", pos, size1, size2, total, nbranch);
    expect(same, "every verdict is the restatement's");
    expect(out.n == n && out.shares == shares && out.blocks == blocks && out.invalid == 0 && out.ntime == ntimes,
           "the counts");

    bm::PoolVerifyArgs A;
    std::vector<uint32_t> tail, branch;
    bm::host::pool_verify_prepare(o.job.get(), A, tail, branch);
    expect(A.nb >= 1 && tail.size() == 16 * (size_t)A.nb && branch.size() == 8 * nbranch && A.j0 < 16 && A.boff < 4 &&
               64 * (pos / 64) + 4 * A.j0 + A.boff == pos && A.size1 == size1 && A.size2 == size2 &&
               A.depth == nbranch && A.has_block == 1 && A.nbits == o.job->nbits,
           "the prepared shape");
    // the field's last word lies inside the template: j0 + 4 may pass it only where the field does not reach
    expect(4 * (size_t)A.j0 + A.boff + size1 + size2 <= 4 * tail.size(), "the field lies inside the template");
    bool roots = true;
    for (size_t i = 0; i < n; ++i) {
        uint8_t header[80], root[32];
        restated_header(o, ses[subs[i].session], subs[i], header);
        lane_root(A, tail, branch, ses[subs[i].session], en2s[i], root);
        roots = roots && std::memcmp(root, header + 36, 32) == 0;
    }
    if (!roots) std::printf("layout pos %zu sizes %u %u total %zu depth %zu\n", pos, size1, size2, total, nbranch);
    expect(roots, "the lane's steps over the prepared template give bm_job_header's root");
    bool words = true;
    for (int k = 0; k < 8; ++k)
        words = words && A.prev[k] == bm::host::load_be32(o.job->prevhash + 4 * k) &&
                A.btgt[k] == bm::host::load_be32(bt + 4 * k);
    expect(words, "prevhash and the block target as words");
}

void invalid_entries() {
    OwnedJob o = make_job(70, 2, 2, 150, 1, 0x207fffffu);
    const size_t n = 5, nses = 2;
    std::unique_ptr<bm_pool_session_t[]> ses(new bm_pool_session_t[nses]);
    std::memset(ses.get(), 0xFF, nses * sizeof(bm_pool_session_t));
    std::unique_ptr<bm_pool_submit_t[]> subs(new bm_pool_submit_t[n]);
    std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[n]);
    std::memset(subs.get(), 0, n * sizeof(bm_pool_submit_t));
    subs[0].extranonce2 = 0xffff, subs[0].session = 1;
    subs[1].extranonce2 = 0x10000, subs[1].session = 1;
    subs[2].session = 2;            // == nsessions
    subs[3].session = 0xFFFFFFFFu;
    subs[4].extranonce2 = UINT64_MAX;
    bm_pool_verify_result_t out;
    expect(bm_pool_verify_cpu(o.job.get(), ses.get(), nses, subs.get(), n, 5, 9, v.get(), &out) == BM_OK,
           "a batch with INVALID entries");
    bool ones = true;
    for (int i = 1; i < 5; ++i) {
        for (uint8_t b : v[i].hash) ones = ones && b == 0xFF;
        ones = ones && v[i].status == BM_SUBMIT_INVALID && v[i].reserved == 0;
    }
    expect(ones, "an INVALID entry: hash all ones, status exactly INVALID");
    expect((v[0].status & ~BM_SUBMIT_BLOCK) == (BM_SUBMIT_SHARE | BM_SUBMIT_NTIME),
           "0xffff fits two bytes; ntime 0 lies outside 5..9");
    expect(out.n == 5 && out.invalid == 4 && out.shares == 1 && out.ntime == 1, "the counts with INVALID entries");
    // no sessions at all, the table a NULL pointer: every entry INVALID
    expect(bm_pool_verify_cpu(o.job.get(), nullptr, 0, subs.get(), n, 0, 0xFFFFFFFFu, v.get(), &out) == BM_OK &&
               out.invalid == 5 && out.shares == 0 && out.ntime == 0 && v[0].status == BM_SUBMIT_INVALID,
           "nsessions == 0");
}

void refusals() {
    OwnedJob o = make_job(20, 4, 4, 90, 2, 0x1d00ffffu);
    const size_t n = 2, nses = 2;
    std::unique_ptr<bm_pool_session_t[]> ses(new bm_pool_session_t[nses]);
    std::memset(ses.get(), 0, nses * sizeof(bm_pool_session_t));
    std::unique_ptr<bm_pool_submit_t[]> subs(new bm_pool_submit_t[n]);
    std::memset(subs.get(), 0, n * sizeof(bm_pool_submit_t));
    std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[n]);
    std::memset(v.get(), 0xA5, n * sizeof(bm_job_verdict_t));
    bm_pool_verify_result_t out;
    std::memset(&out, 0x5A, sizeof out);
    const bm_job_t* j = o.job.get();
    const uint32_t U = 0xFFFFFFFFu;
    expect(bm_pool_verify_cpu(nullptr, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "a NULL job");
    expect(bm_pool_verify_cpu(j, nullptr, nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "NULL sessions with nsessions > 0");
    expect(bm_pool_verify_cpu(j, ses.get(), nses, nullptr, n, 0, U, v.get(), &out) == BM_EINVAL, "NULL submits with n > 0");
    expect(bm_pool_verify_cpu(j, ses.get(), nses, subs.get(), n, 0, U, nullptr, &out) == BM_EINVAL, "NULL verdicts with n > 0");
    expect(bm_pool_verify_cpu(j, ses.get(), nses, subs.get(), n, 0, U, v.get(), nullptr) == BM_EINVAL, "a NULL out");
    expect(bm_pool_verify_cpu(j, ses.get(), nses, subs.get(), (size_t)BM_MAX_JOB_SUBMITS + 1, 0, U, v.get(), &out) == BM_EINVAL,
           "more than BM_MAX_JOB_SUBMITS (nothing is read)");
    expect(bm_pool_verify_cpu(j, ses.get(), (size_t)BM_MAX_POOL_SESSIONS + 1, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL,
           "more than BM_MAX_POOL_SESSIONS (nothing is read)");
    bm_job_t bad = *j;
    bad.extranonce1_len = 0;
    expect(bm_pool_verify_cpu(&bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "extranonce1_len 0");
    bad = *j, bad.extranonce1_len = 9;
    expect(bm_pool_verify_cpu(&bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "extranonce1_len 9");
    bad = *j, bad.extranonce2_size = 9;
    expect(bm_pool_verify_cpu(&bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "size 9");
    bad = *j, bad.nbranch = BM_MAX_JOB_BRANCH + 1;
    expect(bm_pool_verify_cpu(&bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "33 branch entries");
    bad = *j, bad.coinb2 = nullptr;
    expect(bm_pool_verify_cpu(&bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "a NULL coinb2 with a length");
    bad = *j, bad.coinb2_len = BM_MAX_JOB_COINBASE;
    expect(bm_pool_verify_cpu(&bad, ses.get(), nses, subs.get(), n, 0, U, v.get(), &out) == BM_EINVAL, "a coinbase over the limit");
    bool untouched = true;
    const uint8_t* pv = (const uint8_t*)v.get();
    for (size_t i = 0; i < n * sizeof(bm_job_verdict_t); ++i) untouched = untouched && pv[i] == 0xA5;
    const uint8_t* po = (const uint8_t*)&out;
    for (size_t i = 0; i < sizeof out; ++i) untouched = untouched && po[i] == 0x5A;
    expect(untouched, "verdicts and out are untouched by every refusal");
    // n == 0: zeros, no array touched or needed
    expect(bm_pool_verify_cpu(j, nullptr, 0, nullptr, 0, 0, U, nullptr, &out) == BM_OK && out.n == 0 && out.shares == 0 &&
               out.blocks == 0 && out.invalid == 0 && out.ntime == 0,
           "n == 0 with NULL arrays");
    expect(bm_pool_verify_cpu(j, ses.get(), nses, subs.get(), 0, 0, U, v.get(), &out) == BM_OK, "n == 0 with arrays");
    untouched = true;
    for (size_t i = 0; i < n * sizeof(bm_job_verdict_t); ++i) untouched = untouched && pv[i] == 0xA5;
    expect(untouched, "n == 0 touches no verdict");
    expect(bm_pool_verify_cpu(nullptr, ses.get(), nses, nullptr, 0, 0, U, nullptr, &out) == BM_EINVAL, "a NULL job at n == 0");
}

}  // namespace

int main() {
    static_assert(sizeof(bm_pool_session_t) == 40 && sizeof(bm_pool_submit_t) == 24 && sizeof(bm_pool_verify_result_t) == 40,
                  "layouts");
    field_words_cases();
    // the field's offset mod 64 x whole blocks before it x both sizes x the coinbase's length mod 64
    const size_t offs[] = {0, 1, 3, 47, 48, 49, 56, 60, 61, 63}, lens[] = {55, 56, 63, 0, 1};
    const uint32_t sizes[] = {1, 4, 8};
    for (size_t off : offs)
        for (size_t pre : {(size_t)0, (size_t)2})
            for (uint32_t size1 : sizes)
                for (uint32_t size2 : sizes)
                    for (size_t len : lens) {
                        const size_t pos = 64 * pre + off, end = pos + size1 + size2;
                        const size_t total = end + (len + 64 - end % 64) % 64;  // the first length of that residue from the field's end
                        layout_case(pos, size1, size2, total, (off + size1 + size2 + len) % 3);
                    }
    for (size_t depth : {(size_t)12, (size_t)32}) layout_case(45, 4, 4, 250, depth);
    // the limit: the bulk after the field (1,025 tail blocks), and before it (two)
    layout_case(39, 8, 8, BM_MAX_JOB_COINBASE, 1);
    layout_case(BM_MAX_JOB_COINBASE - 30, 8, 8, BM_MAX_JOB_COINBASE, 1);
    invalid_entries();
    refusals();
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("pool verify check ok\n");
    return 0;
}
