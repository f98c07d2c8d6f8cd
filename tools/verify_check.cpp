// verify_check.cpp -- stand-alone CPU check of the share verifier's host code
// (csrc/bm_job.hpp, csrc/bm_job.cpp) under sanitizers: bm_job_verify_cpu on
// exactly-sized heap buffers for the job, `submits` and `verdicts`, over the
// layouts at which extranonce2 meets a word or block edge, against a one-shot
// restatement of the hashing; the refusals, with canaries; INVALID entries; and
// what the GPU entry's host side prepares (host::verify_prepare, en2_words): the
// lane's steps replayed with the host compression must give bm_job_header's bytes.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/verify_check.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_job.cpp -o verify_check && ./verify_check
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

// SHA-256 in one shot: the whole padded message is laid out first.
std::vector<uint8_t> sha256_once(const std::vector<uint8_t>& msg) {
    std::vector<uint8_t> m = msg;
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    const uint64_t bits = (uint64_t)msg.size() * 8;
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(bits >> (8 * i)));
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = bm::kIV256[i];
    for (size_t o = 0; o < m.size(); o += 64) bm::host::compress_bytes(st, m.data() + o);
    std::vector<uint8_t> d(32);
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 4; ++b) d[4 * i + b] = (uint8_t)(st[i] >> (24 - 8 * b));
    return d;
}
std::vector<uint8_t> sha256d_once(const std::vector<uint8_t>& msg) { return sha256_once(sha256_once(msg)); }

// A heap copy of exactly n bytes (nullptr for none): the sanitizer sees any access past it.
std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
    std::unique_ptr<uint8_t[]> p(v.empty() ? nullptr : new uint8_t[v.size()]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size());
    return p;
}

std::vector<uint8_t> random_bytes(size_t n) {
    std::vector<uint8_t> v(n);
    for (auto& b : v) b = rnd8();
    return v;
}

// A job that owns exactly-sized copies of its parts.
struct OwnedJob {
    std::vector<uint8_t> c1, en1, c2, br;
    std::unique_ptr<uint8_t[]> p1, pe, p2, pb;
    std::unique_ptr<bm_job_t> job;
};

// extranonce2 at byte `pos` of a coinbase of `total` bytes.
OwnedJob make_job(size_t pos, uint32_t size, size_t total, size_t nbranch, uint32_t nbits) {
    OwnedJob o;
    const size_t en1_len = pos < 4 ? pos : 4;
    o.c1 = random_bytes(pos - en1_len);
    o.en1 = random_bytes(en1_len);
    o.c2 = random_bytes(total - pos - size);
    o.br = random_bytes(32 * nbranch);
    o.p1 = exact(o.c1), o.pe = exact(o.en1), o.p2 = exact(o.c2), o.pb = exact(o.br);
    o.job.reset(new bm_job_t);
    std::memset(o.job.get(), 0, sizeof(bm_job_t));
    o.job->coinb1 = o.p1.get();
    o.job->coinb1_len = o.c1.size();
    o.job->extranonce1 = o.pe.get();
    o.job->extranonce1_len = o.en1.size();
    o.job->extranonce2_size = size;
    o.job->coinb2 = o.p2.get();
    o.job->coinb2_len = o.c2.size();
    o.job->branch = o.pb.get();
    o.job->nbranch = nbranch;
    for (auto& b : o.job->prevhash) b = rnd8();
    o.job->version = 0x20000000u;
    o.job->nbits = nbits;
    return o;
}

// The hash of a submission, most significant byte first, by the restatement.
std::vector<uint8_t> restated_hash(const OwnedJob& o, const bm_job_submit_t& s) {
    const uint32_t size = o.job->extranonce2_size;
    std::vector<uint8_t> coinbase = o.c1;
    coinbase.insert(coinbase.end(), o.en1.begin(), o.en1.end());
    for (uint32_t i = 0; i < size; ++i) coinbase.push_back((uint8_t)(s.extranonce2 >> (8 * (size - 1 - i))));
    coinbase.insert(coinbase.end(), o.c2.begin(), o.c2.end());
    std::vector<uint8_t> root = sha256d_once(coinbase);
    for (size_t b = 0; b < o.job->nbranch; ++b) {
        root.insert(root.end(), o.br.begin() + 32 * b, o.br.begin() + 32 * b + 32);
        root = sha256d_once(root);
    }
    std::vector<uint8_t> h(80);
    bm::host::store_le32(h.data(), s.version);
    std::memcpy(h.data() + 4, o.job->prevhash, 32);
    std::memcpy(h.data() + 36, root.data(), 32);
    bm::host::store_le32(h.data() + 68, s.ntime);
    bm::host::store_le32(h.data() + 72, o.job->nbits);
    bm::host::store_le32(h.data() + 76, s.nonce);
    std::vector<uint8_t> d = sha256d_once(h);
    return std::vector<uint8_t>(d.rbegin(), d.rend());
}

// The root a lane of job_verify_kernel computes from what verify_prepare made,
// with the host compression: steps 1 to 4 of bm_job_verify.hpp.
void lane_root(const bm::JobVerifyArgs& A, const std::vector<uint32_t>& tail, const std::vector<uint32_t>& branch,
               uint64_t extranonce2, uint8_t root[32]) {
    uint32_t e[3];
    bm::en2_words(extranonce2, A.size, A.boff, e[0], e[1], e[2]);
    uint32_t st[8], w[16];
    for (int k = 0; k < 8; ++k) st[k] = A.mid[k];
    for (uint32_t b = 0; b < A.nb; ++b) {
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t idx = 16 * b + k;
            w[k] = tail[idx];  // (a vector: a read past the template is caught)
            for (uint32_t i = 0; i < 3; ++i)
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

// One layout: bm_job_verify_cpu on exactly-sized arrays against the restatement,
// and the prepared template against bm_job_header.
void layout_case(size_t pos, uint32_t size, size_t total, size_t nbranch) {
    OwnedJob o = make_job(pos, size, total, nbranch, 0x1f00ffffu);
    const uint64_t top = size == 8 ? UINT64_MAX : (1ull << (8 * size)) - 1;
    const size_t n = 6;
    std::unique_ptr<bm_job_submit_t[]> subs(new bm_job_submit_t[n]);
    std::unique_ptr<bm_job_verdict_t[]> verdicts(new bm_job_verdict_t[n]);
    const uint64_t en2s[n] = {0, top, rnd64() & top, 0x0102030405060708ull & top, rnd64() & top, 1};
    for (size_t i = 0; i < n; ++i) {
        subs[i].extranonce2 = en2s[i];
        subs[i].ntime = rnd32();
        subs[i].nonce = rnd32();
        subs[i].version = rnd32();
        subs[i].reserved = rnd32();  // ignored
    }
    // a share target that about half of the hashes meet; the block target of 1f00ffff, about one in 2^9
    std::unique_ptr<uint8_t[]> target(new uint8_t[32]);
    std::memset(target.get(), 0xFF, 32);
    target[0] = 0x7F;
    bm_job_verify_result_t out;
    expect(bm_job_verify_cpu(o.job.get(), target.get(), subs.get(), n, verdicts.get(), &out) == BM_OK, "a legal batch");
    uint8_t bt[32];
    const bool has_block = bm::host::target_from_bits(o.job->nbits, bt);
    expect(has_block, "the case's nbits decodes");
    uint64_t shares = 0, blocks = 0;
    bool same = true;
    for (size_t i = 0; i < n; ++i) {
        const std::vector<uint8_t> h = restated_hash(o, subs[i]);
        uint32_t st = 0;
        if (std::memcmp(h.data(), target.get(), 32) <= 0) st |= BM_SUBMIT_SHARE, ++shares;
        if (std::memcmp(h.data(), bt, 32) <= 0) st |= BM_SUBMIT_BLOCK, ++blocks;
        same = same && std::memcmp(h.data(), verdicts[i].hash, 32) == 0 && verdicts[i].status == st &&
               verdicts[i].reserved == 0;
    }
    if (!same) std::printf("layout pos %zu size %u total %zu depth %zu\n", pos, size, total, nbranch);
    expect(same, "every verdict is the restatement's");
    expect(out.n == n && out.shares == shares && out.blocks == blocks && out.invalid == 0, "the counts");

    bm::JobVerifyArgs A;
    std::vector<uint32_t> tail, branch;
    bm::host::verify_prepare(o.job.get(), target.get(), A, tail, branch);
    expect(A.nb >= 1 && tail.size() == 16 * (size_t)A.nb && branch.size() == 8 * nbranch && A.j0 < 16 && A.boff < 4 &&
               64 * (pos / 64) + 4 * A.j0 + A.boff == pos && A.size == size && A.depth == nbranch && A.has_block == 1,
           "the prepared shape");
    bool roots = true;
    for (size_t i = 0; i < n; ++i) {
        uint8_t header[80], root[32];
        expect(bm_job_header(o.job.get(), en2s[i], 1, 2, header) == BM_OK, "the header of a legal extranonce2");
        lane_root(A, tail, branch, en2s[i], root);
        roots = roots && std::memcmp(root, header + 36, 32) == 0;
    }
    if (!roots) std::printf("layout pos %zu size %u total %zu depth %zu\n", pos, size, total, nbranch);
    expect(roots, "the lane's steps over the prepared template give bm_job_header's root");
    bool words = true;
    for (int k = 0; k < 8; ++k)
        words = words && A.prev[k] == bm::host::load_be32(o.job->prevhash + 4 * k) &&
                A.tgt[k] == bm::host::load_be32(target.get() + 4 * k) && A.btgt[k] == bm::host::load_be32(bt + 4 * k);
    expect(words && A.nbits == o.job->nbits, "prevhash, targets and nbits as words");
}

void invalid_and_flags() {
    {   // size 2: 0x10000 is INVALID, not hashed; its neighbours are judged as usual
        OwnedJob o = make_job(70, 2, 150, 1, 0x207fffffu);
        std::unique_ptr<bm_job_submit_t[]> subs(new bm_job_submit_t[3]);
        std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[3]);
        std::memset(subs.get(), 0, 3 * sizeof(bm_job_submit_t));
        subs[0].extranonce2 = 0xffff;
        subs[1].extranonce2 = 0x10000;
        subs[2].extranonce2 = UINT64_MAX;
        uint8_t target[32];
        std::memset(target, 0xFF, sizeof target);
        bm_job_verify_result_t out;
        expect(bm_job_verify_cpu(o.job.get(), target, subs.get(), 3, v.get(), &out) == BM_OK, "a batch with INVALID entries");
        bool ones = true;
        for (int i = 1; i < 3; ++i)
            for (uint8_t b : v[i].hash) ones = ones && b == 0xFF;
        expect(ones && v[1].status == BM_SUBMIT_INVALID && v[2].status == BM_SUBMIT_INVALID && v[1].reserved == 0,
               "an INVALID entry: hash all ones, status exactly INVALID");
        expect((v[0].status & BM_SUBMIT_SHARE) && !(v[0].status & BM_SUBMIT_INVALID), "0xffff fits two bytes");
        expect(out.n == 3 && out.invalid == 2 && out.shares == 1, "the counts with INVALID entries");
    }
    {   // size 8 accepts 2^64 - 1
        OwnedJob o = make_job(61, 8, 130, 0, 0x1d00ffffu);
        bm_job_submit_t s;
        std::memset(&s, 0, sizeof s);
        s.extranonce2 = UINT64_MAX;
        bm_job_verdict_t v;
        bm_job_verify_result_t out;
        uint8_t target[32];
        std::memset(target, 0xFF, sizeof target);
        expect(bm_job_verify_cpu(o.job.get(), target, &s, 1, &v, &out) == BM_OK && v.status == BM_SUBMIT_SHARE &&
                   out.invalid == 0,
               "2^64 - 1 at size 8");
        expect(std::memcmp(restated_hash(o, s).data(), v.hash, 32) == 0, "its hash");
    }
    {   // flag independence, and an nbits that does not decode
        OwnedJob o = make_job(10, 4, 100, 0, 0x2100ffffu);  // the block target: 0xffff << 240
        bm_job_submit_t s;
        std::memset(&s, 0, sizeof s);
        bm_job_verdict_t v;
        bm_job_verify_result_t out;
        uint8_t zero[32] = {0}, bt[32];
        expect(bm::host::target_from_bits(o.job->nbits, bt), "nbits 2100ffff decodes");
        s.nonce = 0;
        while (true) {  // a nonce whose hash is at or below the block target
            const std::vector<uint8_t> h = restated_hash(o, s);
            if (std::memcmp(h.data(), bt, 32) <= 0) break;
            ++s.nonce;
        }
        expect(bm_job_verify_cpu(o.job.get(), zero, &s, 1, &v, &out) == BM_OK && v.status == BM_SUBMIT_BLOCK &&
                   out.blocks == 1 && out.shares == 0,
               "BLOCK without SHARE");
        o.job->nbits = 0x1d80ffffu;  // the sign bit: no block target
        uint8_t ones[32];
        std::memset(ones, 0xFF, sizeof ones);
        expect(bm_job_verify_cpu(o.job.get(), ones, &s, 1, &v, &out) == BM_OK && v.status == BM_SUBMIT_SHARE &&
                   out.blocks == 0,
               "an nbits that does not decode leaves BLOCK clear");
        bm::JobVerifyArgs A;
        std::vector<uint32_t> tail, branch;
        bm::host::verify_prepare(o.job.get(), ones, A, tail, branch);
        expect(A.has_block == 0, "and the prepared arguments say so");
    }
}

void refusals() {
    OwnedJob o = make_job(20, 4, 90, 2, 0x1d00ffffu);
    const size_t n = 2;
    std::unique_ptr<bm_job_submit_t[]> subs(new bm_job_submit_t[n]);
    std::memset(subs.get(), 0, n * sizeof(bm_job_submit_t));
    std::unique_ptr<bm_job_verdict_t[]> v(new bm_job_verdict_t[n]);
    std::memset(v.get(), 0xA5, n * sizeof(bm_job_verdict_t));
    bm_job_verify_result_t out;
    std::memset(&out, 0x5A, sizeof out);
    uint8_t target[32] = {0};
    const bm_job_t* j = o.job.get();
    expect(bm_job_verify_cpu(nullptr, target, subs.get(), n, v.get(), &out) == BM_EINVAL, "a NULL job");
    expect(bm_job_verify_cpu(j, nullptr, subs.get(), n, v.get(), &out) == BM_EINVAL, "a NULL target");
    expect(bm_job_verify_cpu(j, target, nullptr, n, v.get(), &out) == BM_EINVAL, "NULL submits with n > 0");
    expect(bm_job_verify_cpu(j, target, subs.get(), n, nullptr, &out) == BM_EINVAL, "NULL verdicts with n > 0");
    expect(bm_job_verify_cpu(j, target, subs.get(), n, v.get(), nullptr) == BM_EINVAL, "a NULL out");
    expect(bm_job_verify_cpu(j, target, subs.get(), (size_t)BM_MAX_JOB_SUBMITS + 1, v.get(), &out) == BM_EINVAL,
           "more than BM_MAX_JOB_SUBMITS (nothing is read)");
    bm_job_t bad = *j;
    bad.extranonce2_size = 9;
    expect(bm_job_verify_cpu(&bad, target, subs.get(), n, v.get(), &out) == BM_EINVAL, "size 9");
    bad = *j, bad.nbranch = BM_MAX_JOB_BRANCH + 1;
    expect(bm_job_verify_cpu(&bad, target, subs.get(), n, v.get(), &out) == BM_EINVAL, "33 branch entries");
    bad = *j, bad.coinb2 = nullptr;
    expect(bm_job_verify_cpu(&bad, target, subs.get(), n, v.get(), &out) == BM_EINVAL, "a NULL coinb2 with a length");
    bad = *j, bad.coinb2_len = BM_MAX_JOB_COINBASE;
    expect(bm_job_verify_cpu(&bad, target, subs.get(), n, v.get(), &out) == BM_EINVAL, "a coinbase over the limit");
    bool untouched = true;
    const uint8_t* pv = (const uint8_t*)v.get();
    for (size_t i = 0; i < n * sizeof(bm_job_verdict_t); ++i) untouched = untouched && pv[i] == 0xA5;
    const uint8_t* po = (const uint8_t*)&out;
    for (size_t i = 0; i < sizeof out; ++i) untouched = untouched && po[i] == 0x5A;
    expect(untouched, "verdicts and out are untouched by every refusal");
    // n == 0: zeros, no array touched or needed
    expect(bm_job_verify_cpu(j, target, nullptr, 0, nullptr, &out) == BM_OK && out.n == 0 && out.shares == 0 &&
               out.blocks == 0 && out.invalid == 0,
           "n == 0 with NULL arrays");
    expect(bm_job_verify_cpu(j, target, subs.get(), 0, v.get(), &out) == BM_OK, "n == 0 with arrays");
    untouched = true;
    for (size_t i = 0; i < n * sizeof(bm_job_verdict_t); ++i) untouched = untouched && pv[i] == 0xA5;
    expect(untouched, "n == 0 touches no verdict");
    expect(bm_job_verify_cpu(nullptr, target, nullptr, 0, nullptr, &out) == BM_EINVAL, "a NULL job at n == 0");
}

}  // namespace

int main() {
    static_assert(sizeof(bm_job_submit_t) == 24 && sizeof(bm_job_verdict_t) == 40 && sizeof(bm_job_verify_result_t) == 32,
                  "layouts");
    // extranonce2's offset mod 64 x whole blocks before it x its size x the coinbase's length mod 64
    const size_t offs[] = {0, 1, 3, 56, 57, 60, 61, 63}, lens[] = {55, 56, 63, 0, 1};
    const uint32_t sizes[] = {1, 2, 4, 7, 8};
    for (size_t off : offs)
        for (size_t pre : {(size_t)0, (size_t)2})
            for (uint32_t size : sizes)
                for (size_t len : lens) {
                    const size_t pos = 64 * pre + off;
                    size_t total = (pos + size + 63) / 64 * 64 + len;  // the first length of that residue past extranonce2
                    if (total >= 64 && total - 64 >= pos + size) total -= 64;
                    layout_case(pos, size, total, (off + size + len) % 3);
                }
    for (size_t depth : {(size_t)12, (size_t)32}) layout_case(45, 4, 250, depth);
    // the limit: the bulk after extranonce2 (1,025 tail blocks), and before it (two)
    layout_case(42, 8, BM_MAX_JOB_COINBASE, 1);
    layout_case(BM_MAX_JOB_COINBASE - 30, 8, BM_MAX_JOB_COINBASE, 1);
    invalid_and_flags();
    refusals();
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("verify check ok\n");
    return 0;
}
