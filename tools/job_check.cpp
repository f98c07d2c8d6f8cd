// job_check.cpp -- stand-alone CPU check of the Stratum job layer's host code
// (csrc/bm_job.hpp, csrc/bm_job.cpp): bm_job_header on exactly-sized heap
// buffers at coinbase lengths around the 64-byte block edges and at the limit,
// with 0, 1 and 32 branch entries and every extranonce2 size, against a one-shot
// restatement of the padding; the refusals; the share merge (host::JobMerge) on
// synthetic per-header results: order, all or nothing, the best share, what it
// refuses; bm_target_from_difficulty at denormals, powers of two and the
// saturating edge.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/job_check.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_job.cpp -o job_check && ./job_check
#include <cfloat>
#include <cmath>
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

// SHA-256 in one shot: the whole padded message is laid out first.
void sha256_once(const std::vector<uint8_t>& msg, uint8_t digest[32]) {
    std::vector<uint8_t> m = msg;
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    const uint64_t bits = (uint64_t)msg.size() * 8;
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(bits >> (8 * i)));
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = bm::kIV256[i];
    for (size_t o = 0; o < m.size(); o += 64) bm::host::compress_bytes(st, m.data() + o);
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 4; ++b) digest[4 * i + b] = (uint8_t)(st[i] >> (24 - 8 * b));
}

std::vector<uint8_t> sha256d_once(const std::vector<uint8_t>& msg) {
    uint8_t d[32];
    sha256_once(msg, d);
    sha256_once(std::vector<uint8_t>(d, d + 32), d);
    return std::vector<uint8_t>(d, d + 32);
}

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

// bm_job_header of a job whose coinbase is `total` bytes long, against the restatement.
void header_case(size_t total, uint32_t size, size_t nbranch, size_t en1_len) {
    const size_t rest = total - size - en1_len;
    const std::vector<uint8_t> c1 = random_bytes(rest / 2), c2 = random_bytes(rest - rest / 2);
    const std::vector<uint8_t> en1 = random_bytes(en1_len), br = random_bytes(32 * nbranch);
    const auto p1 = exact(c1), p2 = exact(c2), pe = exact(en1), pb = exact(br);
    std::unique_ptr<bm_job_t> job(new bm_job_t);
    std::memset(job.get(), 0, sizeof(bm_job_t));
    job->coinb1 = p1.get();
    job->coinb1_len = c1.size();
    job->extranonce1 = pe.get();
    job->extranonce1_len = en1.size();
    job->extranonce2_size = size;
    job->coinb2 = p2.get();
    job->coinb2_len = c2.size();
    job->branch = pb.get();
    job->nbranch = nbranch;
    for (auto& b : job->prevhash) b = rnd8();
    job->version = 0x20000000u;
    job->nbits = 0x1d00ffffu;
    const uint64_t top = size == 8 ? UINT64_MAX : (1ull << (8 * size)) - 1;
    const uint64_t en2 = size == 8 ? 0x0102030405060708ull : top - 1;
    const uint32_t ntime = 0x495fab29u, version = 0x2000e000u;
    std::unique_ptr<uint8_t[]> header(new uint8_t[80]);
    expect(bm_job_header(job.get(), en2, ntime, version, header.get()) == BM_OK, "a legal job is accepted");

    std::vector<uint8_t> coinbase = c1;
    coinbase.insert(coinbase.end(), en1.begin(), en1.end());
    for (uint32_t i = 0; i < size; ++i) coinbase.push_back((uint8_t)(en2 >> (8 * (size - 1 - i))));
    coinbase.insert(coinbase.end(), c2.begin(), c2.end());
    expect(coinbase.size() == total, "the case has the length it is about");
    std::vector<uint8_t> root = sha256d_once(coinbase);
    for (size_t b = 0; b < nbranch; ++b) {
        root.insert(root.end(), br.begin() + 32 * b, br.begin() + 32 * b + 32);
        root = sha256d_once(root);
    }
    uint8_t want[80];
    bm::host::store_le32(want, version);
    std::memcpy(want + 4, job->prevhash, 32);
    std::memcpy(want + 36, root.data(), 32);
    bm::host::store_le32(want + 68, ntime);
    bm::host::store_le32(want + 72, job->nbits);
    bm::host::store_le32(want + 76, 0);
    expect(std::memcmp(header.get(), want, 80) == 0, "the header is the restatement's");
    expect(bm_job_header(job.get(), top, ntime, version, header.get()) == BM_OK, "the largest extranonce2 of the size");
    if (size < 8) {
        std::memset(header.get(), 0xA5, 80);
        expect(bm_job_header(job.get(), top + 1, ntime, version, header.get()) == BM_EINVAL && header[0] == 0xA5 &&
                   header[79] == 0xA5,
               "an extranonce2 past its size is refused, the header untouched");
    }
}

void refusals() {
    const std::vector<uint8_t> bytes = random_bytes(64);
    const auto p = exact(bytes);
    bm_job_t ok;
    std::memset(&ok, 0, sizeof ok);
    ok.coinb1 = p.get();
    ok.coinb1_len = 10;
    ok.extranonce1 = p.get();
    ok.extranonce1_len = 4;
    ok.extranonce2_size = 4;
    ok.coinb2 = p.get();
    ok.coinb2_len = 20;
    ok.branch = p.get();
    ok.nbranch = 2;
    uint8_t h[80];
    std::memset(h, 0xA5, sizeof h);
    expect(bm_job_header(&ok, 1, 2, 3, h) == BM_OK, "the base job is legal");
    std::memset(h, 0xA5, sizeof h);
    bm_job_t j;
    expect(bm_job_header(nullptr, 1, 2, 3, h) == BM_EINVAL, "a NULL job");
    expect(bm_job_header(&ok, 1, 2, 3, nullptr) == BM_EINVAL, "a NULL header");
    j = ok, j.coinb1 = nullptr;
    expect(bm_job_header(&j, 1, 2, 3, h) == BM_EINVAL, "a NULL coinb1 with a length");
    j = ok, j.extranonce1 = nullptr;
    expect(bm_job_header(&j, 1, 2, 3, h) == BM_EINVAL, "a NULL extranonce1 with a length");
    j = ok, j.coinb2 = nullptr;
    expect(bm_job_header(&j, 1, 2, 3, h) == BM_EINVAL, "a NULL coinb2 with a length");
    j = ok, j.branch = nullptr;
    expect(bm_job_header(&j, 1, 2, 3, h) == BM_EINVAL, "a NULL branch with entries");
    j = ok, j.extranonce2_size = 0;
    expect(bm_job_header(&j, 0, 2, 3, h) == BM_EINVAL, "size 0");
    j = ok, j.extranonce2_size = 9;
    expect(bm_job_header(&j, 0, 2, 3, h) == BM_EINVAL, "size 9");
    j = ok, j.nbranch = BM_MAX_JOB_BRANCH + 1;
    expect(bm_job_header(&j, 0, 2, 3, h) == BM_EINVAL, "33 branch entries");
    j = ok, j.coinb2_len = BM_MAX_JOB_COINBASE - 10 - 4 - 4 + 1;
    expect(bm_job_header(&j, 0, 2, 3, h) == BM_EINVAL, "a coinbase one byte over the limit");
    j = ok, j.coinb1_len = SIZE_MAX, j.coinb2_len = 2;  // the sum of the lengths wraps
    expect(bm_job_header(&j, 0, 2, 3, h) == BM_EINVAL, "lengths whose sum wraps");
    expect(bm_job_header(&ok, 1ull << 32, 2, 3, h) == BM_EINVAL, "extranonce2 = 2^32 at size 4");
    bool untouched = true;
    for (uint8_t b : h) untouched = untouched && b == 0xA5;
    expect(untouched, "the header is untouched by every refusal");
    j = ok, j.coinb1 = nullptr, j.coinb1_len = 0, j.extranonce1 = nullptr, j.extranonce1_len = 0, j.coinb2 = nullptr,
    j.coinb2_len = 0, j.branch = nullptr, j.nbranch = 0;
    expect(bm_job_header(&j, 1, 2, 3, h) == BM_OK, "NULL pointers with zero lengths are legal");

    uint8_t sw[32], back[32];
    for (int i = 0; i < 32; ++i) sw[i] = (uint8_t)i;
    expect(bm_job_prevhash_from_stratum(sw, back) == BM_OK && back[0] == 3 && back[3] == 0 && back[28] == 31 &&
               back[31] == 28,
           "each 4-byte word is reversed");
    expect(bm_job_prevhash_from_stratum(back, back) == BM_OK && std::memcmp(back, sw, 32) == 0, "in place, and back");
    expect(bm_job_prevhash_from_stratum(nullptr, back) == BM_EINVAL && bm_job_prevhash_from_stratum(sw, nullptr) == BM_EINVAL,
           "NULL arrays");
}

// A synthetic per-header answer: n hits at nonces base, base + step, ... under
// alternating indices, the best share's top 64 bits `best_top`.
struct Synth {
    std::unique_ptr<bm_header_version_hit_t[]> hits;
    bm_header_versions_hits_result_t r;
};

Synth synth(size_t n, size_t room, uint32_t base, uint64_t best_top, uint8_t hash_byte) {
    Synth s;
    std::memset(&s.r, 0, sizeof s.r);
    s.r.count = n;
    s.r.stored = n <= room ? n : 0;
    for (int i = 0; i < 8; ++i) s.r.hash[i] = (uint8_t)(best_top >> (8 * (7 - i)));
    s.r.nonce = base;
    s.r.version_index = 1;
    s.r.version = 0x2000;
    if (s.r.stored) s.hits.reset(new bm_header_version_hit_t[s.r.stored]);  // exactly the stored entries
    for (size_t i = 0; i < s.r.stored; ++i) {
        bm_header_version_hit_t& h = s.hits[i];
        std::memset(&h, 0, sizeof h);
        std::memset(h.hash, hash_byte, sizeof h.hash);
        h.hash[0] = 0;
        h.hash[31] = (uint8_t)i;
        h.nonce = base + (uint32_t)(i / 2);
        h.version_index = (uint32_t)(i % 2);
        h.version = h.version_index ? 0x2000 : 0;
    }
    return s;
}

void merge_checks() {
    static_assert(sizeof(bm_job_share_t) == 64, "share layout");
    static_assert(sizeof(bm_job_shares_result_t) == 80, "result layout");
    uint8_t block[32];
    std::memset(block, 0, sizeof block);
    std::memset(block + 1, 0x40, 31);  // hashes of byte 0x30 are blocks, of 0x50 are not
    const size_t per[3] = {5, 0, 7};
    const uint8_t fill[3] = {0x30, 0x50, 0x50};
    const uint64_t tops[3] = {900, 700, 700};  // the best: the earlier of the two equal ones
    for (size_t cap : {(size_t)12, (size_t)13, (size_t)11, (size_t)5, (size_t)4, (size_t)0}) {
        bm::host::JobMerge m(cap, block, 0x495fab29u, 40, 7);
        std::unique_ptr<bm_job_share_t[]> shares(cap ? new bm_job_share_t[cap] : nullptr);
        if (cap) std::memset(shares.get(), 0xA5, cap * sizeof(bm_job_share_t));
        bool ok = true;
        uint64_t running = 0;
        for (int k = 0; k < 3; ++k) {
            const size_t room = m.room();
            ok = ok && room == (running <= cap ? cap - running : 0);
            Synth s = synth(per[k], room, 1000 * (uint32_t)(3 - k), tops[k], fill[k]);
            ok = ok && m.add(40 + 2 * (uint64_t)k, s.hits.get(), s.r) == BM_OK;
            running += per[k];
        }
        expect(ok, "three headers are merged, each with what is left of the cap");
        bm_job_shares_result_t out;
        m.finish(shares.get(), &out);
        expect(out.count == 12 && out.headers == 3, "the count is exact whatever the cap");
        expect(out.stored == (cap >= 12 ? 12u : 0u), "all or nothing over the whole call");
        expect(bm::host::hash_top64(out.hash) == 700 && out.extranonce2 == 42 && out.nonce == 2000 &&
                   out.version_index == 1 && out.version == 0x2000 && out.reserved == 0,
               "the best share: the smallest top 64 bits, then the smallest extranonce2");
        if (cap >= 12) {
            bool order = true, fields = true;
            for (size_t i = 0; i < 12; ++i) {
                const bm_job_share_t& s = shares[i];
                const uint64_t en2 = i < 5 ? 40 : 44;
                const size_t k = i < 5 ? i : i - 5;
                fields = fields && s.extranonce2 == en2 && s.ntime == 0x495fab29u && s.reserved == 0 &&
                         s.nonce == (i < 5 ? 3000u : 1000u) + k / 2 && s.version_index == k % 2 &&
                         s.version == (k % 2 ? 0x2000u : 0u) && s.is_block == (i < 5 ? 1u : 0u) && s.hash[31] == k;
                if (i > 0) {
                    const bm_job_share_t& p = shares[i - 1];
                    order = order && (p.extranonce2 < s.extranonce2 ||
                                      (p.extranonce2 == s.extranonce2 &&
                                       (p.nonce < s.nonce || (p.nonce == s.nonce && p.version_index < s.version_index))));
                }
            }
            expect(order, "ascending by (extranonce2, nonce, index)");
            expect(fields, "every field of every share");
            if (cap == 13) {
                bool tail = true;
                const uint8_t* t = (const uint8_t*)&shares[12];
                for (size_t i = 0; i < sizeof(bm_job_share_t); ++i) tail = tail && t[i] == 0xA5;
                expect(tail, "nothing past the stored entries is written");
            }
        } else if (cap) {
            bool clean = true;
            const uint8_t* t = (const uint8_t*)shares.get();
            for (size_t i = 0; i < cap * sizeof(bm_job_share_t); ++i) clean = clean && t[i] == 0xA5;
            expect(clean, "a count above the cap leaves the array untouched");
        }
    }

    {   // nothing added: the empty answer
        bm::host::JobMerge m(4, nullptr, 1, 77, 0x20000000u);
        bm_job_shares_result_t out;
        m.finish(nullptr, &out);
        bool ones = true;
        for (uint8_t b : out.hash) ones = ones && b == 0xFF;
        expect(ones && out.nonce == 0xFFFFFFFFu && out.extranonce2 == 77 && out.version_index == 0 &&
                   out.version == 0x20000000u && out.count == 0 && out.stored == 0 && out.headers == 0,
               "the empty answer");
    }
    {   // no block target: is_block stays 0
        bm::host::JobMerge m(4, nullptr, 1, 0, 0);
        Synth s = synth(2, 4, 5, 1, 0x00);
        bm_job_share_t shares[4];
        bm_job_shares_result_t out;
        expect(m.add(0, s.hits.get(), s.r) == BM_OK, "a header without a block target");
        m.finish(shares, &out);
        expect(out.stored == 2 && shares[0].is_block == 0 && shares[1].is_block == 0, "is_block stays 0");
    }
    {   // what add refuses
        bm::host::JobMerge m(8, block, 1, 0, 0);
        Synth s = synth(3, 8, 5, 10, 0x30);
        expect(m.add(5, s.hits.get(), s.r) == BM_OK, "a first header");
        Synth again = synth(2, m.room(), 5, 10, 0x30);
        expect(m.add(5, again.hits.get(), again.r) == BM_EINTERNAL, "the same extranonce2 twice");
        expect(m.add(4, again.hits.get(), again.r) == BM_EINTERNAL, "a smaller extranonce2");
        Synth over = synth(6, 8, 5, 10, 0x30);  // claims to have stored 6 with room for 5
        expect(m.add(6, over.hits.get(), over.r) == BM_EINTERNAL, "more stored than there was room for");
        Synth none = synth(2, m.room(), 5, 10, 0x30);
        none.r.stored = 0;
        expect(m.add(6, none.hits.get(), none.r) == BM_EINTERNAL, "nothing stored though the count fits");
        Synth swapped = synth(3, m.room(), 5, 10, 0x30);
        std::swap(swapped.hits[0], swapped.hits[1]);
        expect(m.add(6, swapped.hits.get(), swapped.r) == BM_EINTERNAL, "entries out of order");
        Synth twice = synth(3, m.room(), 5, 10, 0x30);
        twice.hits[1] = twice.hits[0];
        expect(m.add(6, twice.hits.get(), twice.r) == BM_EINTERNAL, "a pair twice");
        Synth null = synth(2, m.room(), 5, 10, 0x30);
        expect(m.add(6, nullptr, null.r) == BM_EINTERNAL, "stored entries without an array");
        bm_job_share_t shares[8];
        bm_job_shares_result_t out;
        m.finish(shares, &out);
        expect(out.count == 3 && out.stored == 3 && out.headers == 1, "a refused header changes nothing");
    }
    {   // 2^64 - 1 is a legal last extranonce2
        bm::host::JobMerge m(2, nullptr, 1, UINT64_MAX - 1, 0);
        Synth a = synth(1, 2, 5, 10, 0x30), b = synth(1, 1, 5, 9, 0x30);
        bm_job_share_t shares[2];
        bm_job_shares_result_t out;
        expect(m.add(UINT64_MAX - 1, a.hits.get(), a.r) == BM_OK && m.add(UINT64_MAX, b.hits.get(), b.r) == BM_OK,
               "the last two extranonce2 values");
        m.finish(shares, &out);
        expect(out.stored == 2 && shares[1].extranonce2 == UINT64_MAX && out.extranonce2 == UINT64_MAX, "2^64 - 1");
    }
}

// 0xffff << shift as a 256-bit number (a right shift for shift < 0), or all ones when it does not fit.
void shifted_ffff(int shift, uint8_t t[32]) {
    std::memset(t, 0, 32);
    if (shift + 16 > 256) {
        std::memset(t, 0xFF, 32);
        return;
    }
    for (int b = 0; b < 16; ++b) {
        const int pos = shift + b;  // bit position from the least significant end
        if (pos >= 0) t[31 - pos / 8] |= (uint8_t)(1u << (pos % 8));
    }
}

void difficulty_checks() {
    uint8_t t[32], want[32];
    for (int k = -60; k <= 240; ++k) {
        expect(bm_target_from_difficulty(std::ldexp(1.0, k), t) == BM_OK, "a power of two is accepted");
        shifted_ffff(208 - k, want);
        if (std::memcmp(t, want, 32) != 0) {
            std::printf("FAIL: difficulty 2^%d\n", k);
            ++fails;
        }
    }
    uint8_t ones[32], zero[32] = {0};
    std::memset(ones, 0xFF, sizeof ones);
    const double tiny[] = {5e-324 /* the smallest denormal */, 2.2250738585072009e-308 /* the largest */, DBL_MIN, 1e-30,
                           std::ldexp(1.0, -40)};
    for (double d : tiny)
        expect(bm_target_from_difficulty(d, t) == BM_OK && std::memcmp(t, ones, 32) == 0, "a tiny difficulty saturates");
    expect(bm_target_from_difficulty(DBL_MAX, t) == BM_OK && std::memcmp(t, zero, 32) == 0, "the largest double gives 0");
    // diff1 / d = 2^256 exactly at d = 0xffff * 2^-48: the last difficulty that saturates
    const double edge = std::ldexp(65535.0, -48);
    expect(bm_target_from_difficulty(edge, t) == BM_OK && std::memcmp(t, ones, 32) == 0, "the saturating edge");
    expect(bm_target_from_difficulty(std::nextafter(edge, 1.0), t) == BM_OK && std::memcmp(t, ones, 32) != 0 &&
               t[0] == 0xFF && t[5] == 0xFF,
           "one step above the edge fits 256 bits");
    expect(bm_target_from_difficulty(std::nextafter(edge, 0.0), t) == BM_OK && std::memcmp(t, ones, 32) == 0,
           "one step below it saturates");
    // diff1 itself gives 1, one step above gives 0
    const double diff1 = std::ldexp(65535.0, 208);
    expect(bm_target_from_difficulty(diff1, t) == BM_OK && t[31] == 1 && std::memcmp(t, zero, 31) == 0, "diff1 gives 1");
    expect(bm_target_from_difficulty(std::nextafter(diff1, DBL_MAX), t) == BM_OK && std::memcmp(t, zero, 32) == 0,
           "above diff1 gives 0");
    // 3.0: 0xffff / 3 = 0x5555 exactly, shifted by 208
    expect(bm_target_from_difficulty(3.0, t) == BM_OK && t[4] == 0x55 && t[5] == 0x55 && t[3] == 0 && t[6] == 0 && t[31] == 0,
           "difficulty 3");
    std::memset(t, 0xA5, sizeof t);
    const double bad[] = {0.0, -0.0, -1.0, std::nan(""), HUGE_VAL, -HUGE_VAL};
    for (double d : bad) expect(bm_target_from_difficulty(d, t) == BM_EINVAL, "a refused difficulty");
    expect(bm_target_from_difficulty(1.0, nullptr) == BM_EINVAL, "a NULL target");
    bool untouched = true;
    for (uint8_t b : t) untouched = untouched && b == 0xA5;
    expect(untouched, "the target is untouched by every refusal");
}

}  // namespace

int main() {
    const size_t lengths[] = {55, 56, 63, 64, 65, 119, 120, BM_MAX_JOB_COINBASE};
    for (size_t total : lengths)
        for (size_t nbranch : {(size_t)0, (size_t)1, (size_t)32}) header_case(total, 4, nbranch, 4);
    for (uint32_t size = 1; size <= 8; ++size) {
        header_case(64, size, 1, 0);   // no extranonce1: a NULL pointer with a zero length
        header_case(120, size, 0, 8);
    }
    refusals();
    merge_checks();
    difficulty_checks();
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("job check ok\n");
    return 0;
}
