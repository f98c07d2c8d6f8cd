// header_versions_hits_check.cpp -- stand-alone CPU check of the host half of
// the version-rolling share enumeration (csrc/bm_header_versions_hits.hpp:
// header_versions_hits_collect, header_versions_hits_best): entries as 1 to 3
// devices running several groups of versions would leave them (shuffled, some
// devices empty) come back sorted by (nonce, index) with their full hashes; a
// forged entry of each kind is refused; a buffer filled exactly to its capacity
// is written to its last entry and not past it; the best share is checked
// against the host's hash and against the count.  With --one-version: the same
// collect as bm_search_header_hits_gpu uses it (one_version below).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/header_versions_hits_check.cpp -o vh_check && ./vh_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bm_header_versions_hits.hpp"

namespace {

using bm::host::hash_top64;

int fails = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++fails;
    }
}

const char* kGenesis =
    "0100000000000000000000000000000000000000000000000000000000000000000000003ba3edfd7a7b12b27ac72c3e67768f617f"
    "c81bc3888a51323a9fb8aa4b1e5e4a29ab5f49ffff001d1dac2b7c";

// seven versions (groups 4 + 2 + 1), one of them twice (indices 1 and 5)
const uint32_t kVersions[] = {0x20000000u, 0x20002000u, 1u, 0x3fffe000u, 0u, 0x20002000u, 0xffffffffu};
constexpr size_t kNver = sizeof kVersions / sizeof kVersions[0];

uint32_t rng_state = 0x9E3779B9u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

void pair_hash(const uint8_t* header, uint32_t vi, uint32_t nonce, uint8_t out[32]) {
    uint8_t hv[bm::kHeaderBytes];
    bm::host::header_with_version(header, kVersions[vi], hv);
    bm::host::header_hash_msb(hv, nonce, out);
}

// Every hit of [lo, hi] x versions at `target`, ascending by (n, i): what the devices report.
std::vector<bm::Partial> true_hits(const uint8_t* header, const uint8_t* target, uint32_t lo, uint32_t hi) {
    std::vector<bm::Partial> v;
    for (uint64_t n = lo; n <= hi; ++n)
        for (uint32_t i = 0; i < kNver; ++i) {
            uint8_t h[32];
            pair_hash(header, i, (uint32_t)n, h);
            if (std::memcmp(h, target, 32) <= 0) v.push_back(bm::Partial{hash_top64(h), bm::host::versions_key((uint32_t)n, i)});
        }
    return v;
}

// The collect over exactly-sized heap arrays (the sanitizer sees any access past them).
template <class Hit>
int collect(const uint8_t* header, const uint8_t* target, uint32_t lo, uint32_t hi, const uint32_t* versions,
            size_t nver, const std::vector<bm::Partial>& in, const std::vector<size_t>& counts,
            std::vector<Hit>& out) {
    std::unique_ptr<bm::Partial[]> e(new bm::Partial[in.size()]);
    std::unique_ptr<Hit[]> o(new Hit[in.size()]);
    std::unique_ptr<uint32_t[]> vers(new uint32_t[nver]);
    std::memcpy(vers.get(), versions, nver * sizeof(uint32_t));
    std::memset(o.get(), 0xA5, in.size() * sizeof(Hit));
    for (size_t i = 0; i < in.size(); ++i) e[i] = in[i];
    const int rc = bm::host::header_versions_hits_collect(header, vers.get(), nver, target, lo, hi, e.get(),
                                                          counts.data(), (int)counts.size(), o.get());
    out.assign(o.get(), o.get() + in.size());
    return rc;
}
int collect(const uint8_t* header, const uint8_t* target, uint32_t lo, uint32_t hi, size_t nver,
            const std::vector<bm::Partial>& in, const std::vector<size_t>& counts,
            std::vector<bm_header_version_hit_t>& out) {
    return collect(header, target, lo, hi, kVersions, nver, in, counts, out);
}

// --one-version: the host half of bm_search_header_hits_gpu, the same collect
// over the header's own version alone with bm_header_hit_t output.  Entries as
// 1 to 3 devices would leave them (shuffled, some devices empty) come back
// sorted by nonce with their full hashes; a forged entry of each kind is
// refused; a buffer filled exactly to its capacity is written to its last entry
// and not past it.
int one_version(const uint8_t* header) {
    static_assert(sizeof(bm_header_hit_t) == 40, "hit entry layout");
    static_assert(sizeof(bm_header_hits_result_t) == 56, "result layout");
    using bm::host::versions_key;
    const uint32_t own = bm::host::header_version(header);
    expect(own == 1, "the genesis header's version field, le32(header[0..3])");
    const uint32_t lo = 1000, hi = 20999;
    uint8_t target[32], h[32];
    std::memset(target, 0xFF, sizeof target);
    target[0] = 0x03;  // 6 leading zero bits: about 300 of 20000
    auto entry = [&](uint32_t n) {
        bm::host::header_hash_msb(header, n, h);
        return bm::Partial{hash_top64(h), versions_key(n, 0)};
    };
    std::vector<bm::Partial> truth;  // every hit of [lo, hi], ascending: what the devices report
    for (uint32_t n = lo; n <= hi; ++n)
        if (entry(n), std::memcmp(h, target, 32) <= 0) truth.push_back(entry(n));
    expect(truth.size() > 100 && truth.size() < 1000, "the window holds a few hundred hits");
    auto run = [&](const uint8_t* tgt, const std::vector<bm::Partial>& in, const std::vector<size_t>& counts,
                   std::vector<bm_header_hit_t>& out) { return collect(header, tgt, lo, hi, &own, 1, in, counts, out); };

    // 1..3 devices, each with a contiguous piece in shuffled order; cuts at the
    // ends leave the first, the middle or the last device empty
    for (int ndev = 1; ndev <= 3; ++ndev) {
        for (int round = 0; round < 8; ++round) {
            std::vector<size_t> cut(ndev + 1, 0);
            cut[ndev] = truth.size();
            for (int d = 1; d < ndev; ++d) cut[d] = round == 0 ? 0 : round == 1 ? truth.size() : rnd() % (truth.size() + 1);
            if (ndev == 3 && round == 2) cut[1] = cut[2] = truth.size() / 2;  // the middle one empty
            std::sort(cut.begin(), cut.end());
            std::vector<bm::Partial> in = truth;
            std::vector<size_t> counts(ndev);
            for (int d = 0; d < ndev; ++d) {
                counts[d] = cut[d + 1] - cut[d];
                for (size_t i = cut[d + 1]; i > cut[d] + 1; --i) std::swap(in[i - 1], in[cut[d] + rnd() % (i - cut[d])]);
            }
            std::vector<bm_header_hit_t> out;
            expect(run(target, in, counts, out) == BM_OK, "true entries are accepted");
            bool same = out.size() == truth.size();
            for (size_t i = 0; same && i < out.size(); ++i) {
                const uint32_t n = bm::host::key_nonce(truth[i].nonce);
                bm::host::header_hash_msb(header, n, h);
                same = out[i].nonce == n && out[i].reserved == 0 && std::memcmp(out[i].hash, h, 32) == 0;
            }
            expect(same, "sorted by nonce with the full hashes");
        }
    }

    // no entries at all: nothing is read or written (null arrays)
    {
        const size_t none[3] = {0, 0, 0};
        expect(bm::host::header_versions_hits_collect(header, &own, 1, target, lo, hi, nullptr, none, 3,
                                                      (bm_header_hit_t*)nullptr) == BM_OK,
               "no entries");
    }

    // a forged entry of each kind, in a list that is otherwise true
    struct Forge {
        const char* what;
        bm::Partial entry;
        bool replace;  // put it in place of entry 5 (else: append it)
        bool alone;    // the one entry of a list at target all-ones: the range check stands alone
    };
    uint32_t miss = lo;  // a nonce of the range that is no hit
    while (entry(miss), std::memcmp(h, target, 32) <= 0) ++miss;
    uint8_t ones[32];
    std::memset(ones, 0xFF, sizeof ones);
    const Forge forges[] = {
        {"a nonce whose hash is above the target", entry(miss), true, false},
        {"a wrong top 64 bits", {truth[5].hash ^ 1, truth[5].nonce}, true, false},
        {"a wrong top 64 bits, high word", {truth[5].hash ^ (1ull << 63), truth[5].nonce}, true, false},
        {"a nonce below the range", entry(lo - 1), false, true},
        {"a nonce above the range", entry(hi + 1), false, true},
        // the key's nonce field is 32 bits wide; what lies past it is the index, and one version has index 0 alone
        {"an index past the one version", {truth[5].hash, truth[5].nonce | 1}, true, false},
        {"an entry in the old layout, the bare nonce", {truth[5].hash, bm::host::key_nonce(truth[5].nonce)}, true, false},
        {"a nonce twice", truth[7], false, false},
        {"a nonce twice, across devices", truth.back(), true, false},
    };
    for (const Forge& f : forges) {
        std::vector<bm::Partial> in = truth;
        if (f.replace)
            in[5] = f.entry;
        else
            in.push_back(f.entry);
        for (size_t i = in.size(); i > 1; --i) std::swap(in[i - 1], in[rnd() % i]);
        const std::vector<size_t> counts = {in.size() / 2, in.size() - in.size() / 2};
        std::vector<bm_header_hit_t> out;
        expect(run(f.alone ? ones : target, f.alone ? std::vector<bm::Partial>{f.entry} : in,
                   f.alone ? std::vector<size_t>{1} : counts, out) == BM_EINTERNAL,
               f.what);
    }

    // count == cap: the caller's array has exactly as many entries as there are hits
    {
        std::vector<bm::Partial> in(truth.rbegin(), truth.rend());
        std::vector<bm_header_hit_t> out;
        expect(run(target, in, {in.size()}, out) == BM_OK && out.back().nonce == bm::host::key_nonce(truth.back().nonce) &&
                   out.front().nonce == bm::host::key_nonce(truth.front().nonce),
               "a buffer filled to its last entry");
    }

    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("header hits check ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    static_assert(sizeof(bm_header_version_hit_t) == 48, "hit entry layout");
    static_assert(sizeof(bm_header_versions_hits_result_t) == 64, "result layout");
    uint8_t header[bm::kHeaderBytes];
    for (int i = 0; i < bm::kHeaderBytes; ++i) {
        unsigned v = 0;
        std::sscanf(kGenesis + 2 * i, "%2x", &v);
        header[i] = (uint8_t)v;
    }
    if (argc > 1 && std::strcmp(argv[1], "--one-version") == 0) return one_version(header);
    const uint32_t lo = 1000, hi = 3999;
    uint8_t target[32];
    std::memset(target, 0xFF, sizeof target);
    target[0] = 0x03;  // 6 leading zero bits: about 330 of 21000 pairs
    const std::vector<bm::Partial> truth = true_hits(header, target, lo, hi);
    expect(truth.size() > 100 && truth.size() < 1000, "the window holds a few hundred hits");
    bool twice = false;  // the repeated version hits under both of its indices
    for (size_t i = 0; i + 1 < truth.size(); ++i)
        for (size_t k = i + 1; k < truth.size() && (truth[k].nonce >> 32) == (truth[i].nonce >> 32); ++k)
            twice = twice || ((uint32_t)truth[i].nonce == 1 && (uint32_t)truth[k].nonce == 5 && truth[i].hash == truth[k].hash);
    expect(twice, "a repeated version gives two entries");

    // 1..3 devices, each with a contiguous piece of the nonce range whose entries
    // (of all its groups' launches) lie in shuffled order; cuts at the ends leave
    // the first, the middle or the last device empty
    for (int ndev = 1; ndev <= 3; ++ndev) {
        for (int round = 0; round < 8; ++round) {
            std::vector<size_t> cut(ndev + 1, 0);
            cut[ndev] = truth.size();
            for (int d = 1; d < ndev; ++d) cut[d] = round == 0 ? 0 : round == 1 ? truth.size() : rnd() % (truth.size() + 1);
            if (ndev == 3 && round == 2) cut[1] = cut[2] = truth.size() / 2;  // the middle one empty
            std::sort(cut.begin(), cut.end());
            std::vector<bm::Partial> in = truth;
            std::vector<size_t> counts(ndev);
            for (int d = 0; d < ndev; ++d) {
                counts[d] = cut[d + 1] - cut[d];
                for (size_t i = cut[d + 1]; i > cut[d] + 1; --i) std::swap(in[i - 1], in[cut[d] + rnd() % (i - cut[d])]);
            }
            std::vector<bm_header_version_hit_t> out;
            expect(collect(header, target, lo, hi, kNver, in, counts, out) == BM_OK, "true entries are accepted");
            bool same = out.size() == truth.size();
            for (size_t i = 0; same && i < out.size(); ++i) {
                uint8_t h[32];
                const uint32_t n = bm::host::key_nonce(truth[i].nonce), vi = bm::host::key_index(truth[i].nonce);
                pair_hash(header, vi, n, h);
                same = out[i].nonce == n && out[i].version_index == vi && out[i].version == kVersions[vi] &&
                       out[i].reserved == 0 && std::memcmp(out[i].hash, h, 32) == 0;
            }
            expect(same, "sorted by (nonce, index) with the full hashes");
        }
    }

    // no entries at all: nothing is read or written (null arrays)
    {
        const size_t none[3] = {0, 0, 0};
        expect(bm::host::header_versions_hits_collect(header, kVersions, kNver, target, lo, hi, nullptr, none, 3,
                                                      (bm_header_version_hit_t*)nullptr) == BM_OK,
               "no entries");
    }

    // a forged entry of each kind, in a list that is otherwise true
    struct Forge {
        const char* what;
        bm::Partial entry;
        bool replace;  // put it in place of entry 5 (else: append it)
        bool alone;    // the one entry of a list at target all-ones: the check stands alone
    };
    uint8_t h[32];
    uint32_t miss = lo;  // a nonce of the range that is no hit under version 0
    for (;; ++miss) {
        pair_hash(header, 0, miss, h);
        if (std::memcmp(h, target, 32) > 0) break;
    }
    const uint64_t miss_top = hash_top64(h);
    const uint32_t below = lo - 1, above = hi + 1;
    uint8_t ones[32];
    std::memset(ones, 0xFF, sizeof ones);
    pair_hash(header, 2, below, h);
    const uint64_t below_top = hash_top64(h);
    pair_hash(header, 2, above, h);
    const uint64_t above_top = hash_top64(h);
    // index 5 of a list cut to 5 versions: a true hash of the full list, but no index of this call
    size_t at5 = 0;
    while ((uint32_t)truth[at5].nonce != 5) ++at5;
    const uint32_t n5 = bm::host::key_nonce(truth[5].nonce), i5 = bm::host::key_index(truth[5].nonce);
    pair_hash(header, i5 == 0 ? 2 : 0, n5, h);  // entry 5's nonce under another version
    const Forge forges[] = {
        {"a pair whose hash is above the target", {miss_top, bm::host::versions_key(miss, 0)}, true, false},
        {"a wrong top 64 bits", {truth[5].hash ^ 1, truth[5].nonce}, true, false},
        {"a wrong top 64 bits, high word", {truth[5].hash ^ (1ull << 63), truth[5].nonce}, true, false},
        {"the top 64 bits of another version's hash", {hash_top64(h), truth[5].nonce}, true, false},
        {"a nonce below the range", {below_top, bm::host::versions_key(below, 2)}, false, true},
        {"a nonce above the range", {above_top, bm::host::versions_key(above, 2)}, false, true},
        {"an index at nver", {truth[5].hash, bm::host::versions_key(n5, (uint32_t)kNver)}, true, false},
        {"an index past 6 bits", {truth[5].hash, truth[5].nonce | (1ull << 31)}, true, false},
        {"a key twice", truth[7], false, false},
        {"a key twice, across devices", truth.back(), true, false},
    };
    for (const Forge& f : forges) {
        std::vector<bm::Partial> in = truth;
        if (f.replace)
            in[5] = f.entry;
        else
            in.push_back(f.entry);
        for (size_t i = in.size(); i > 1; --i) std::swap(in[i - 1], in[rnd() % i]);
        const std::vector<size_t> counts = {in.size() / 2, in.size() - in.size() / 2};
        std::vector<bm_header_version_hit_t> out;
        expect(collect(header, f.alone ? ones : target, lo, hi, kNver, f.alone ? std::vector<bm::Partial>{f.entry} : in,
                       f.alone ? std::vector<size_t>{1} : counts, out) == BM_EINTERNAL,
               f.what);
    }
    {   // a true entry of index 5 when the call has 5 versions only
        std::vector<bm_header_version_hit_t> out;
        expect(collect(header, target, lo, hi, 5, {truth[at5]}, {1}, out) == BM_EINTERNAL, "an index of a longer list");
        expect(collect(header, target, lo, hi, 6, {truth[at5]}, {1}, out) == BM_OK, "the last index of the list");
    }

    // count == cap: the caller's array has exactly as many entries as there are hits
    {
        std::vector<bm::Partial> in(truth.rbegin(), truth.rend());
        std::vector<bm_header_version_hit_t> out;
        expect(collect(header, target, lo, hi, kNver, in, {in.size()}, out) == BM_OK &&
                   bm::host::versions_key(out.back().nonce, out.back().version_index) == truth.back().nonce &&
                   bm::host::versions_key(out.front().nonce, out.front().version_index) == truth.front().nonce,
               "a buffer filled to its last entry");
    }

    // the best share: the minimum of (top 64 bits, key) over every pair of the range
    {
        bm::Partial best{UINT64_MAX, UINT64_MAX};
        for (uint32_t n = lo; n <= hi; ++n)
            for (uint32_t i = 0; i < kNver; ++i) {
                pair_hash(header, i, n, h);
                const bm::Partial p{hash_top64(h), bm::host::versions_key(n, i)};
                if (p.hash < best.hash || (p.hash == best.hash && p.nonce < best.nonce)) best = p;
            }
        bm_header_versions_hits_result_t r;
        std::memset(&r, 0xA5, sizeof r);
        const bm_header_versions_hits_result_t before = r;
        expect(bm::host::header_versions_hits_best(header, kVersions, kNver, target, best, truth.size(), &r) == BM_OK,
               "the true best share is accepted");
        pair_hash(header, r.version_index, r.nonce, h);
        expect(std::memcmp(r.hash, h, 32) == 0 && bm::host::versions_key(r.nonce, r.version_index) == best.nonce &&
                   r.version == kVersions[r.version_index] && r.reserved == 0,
               "with its full hash, nonce, index and version");
        expect(r.count == before.count && r.stored == before.stored, "count and stored are left to the caller");
        r = before;
        expect(bm::host::header_versions_hits_best(header, kVersions, kNver, target, best, 0, &r) == BM_EINTERNAL,
               "a best share at or below the target with a count of zero");
        uint8_t zero[32] = {0};
        expect(bm::host::header_versions_hits_best(header, kVersions, kNver, zero, best, 0, &r) == BM_OK,
               "a best share above the target with a count of zero");
        r = before;
        expect(bm::host::header_versions_hits_best(header, kVersions, kNver, target, {best.hash ^ 1, best.nonce},
                                                   truth.size(), &r) == BM_EINTERNAL,
               "a best share with other top 64 bits");
        expect(bm::host::header_versions_hits_best(header, kVersions, kNver, target,
                                                   {best.hash, bm::host::versions_key(lo, (uint32_t)kNver)},
                                                   truth.size(), &r) == BM_EINTERNAL,
               "a best share with an index at nver");
        expect(bm::host::header_versions_hits_best(header, kVersions, kNver, target, {UINT64_MAX, UINT64_MAX},
                                                   truth.size(), &r) == BM_EINTERNAL,
               "no best share for a non-empty range");
        expect(std::memcmp(&r, &before, sizeof r) == 0, "out is untouched on failure");
    }

    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("header versions hits check ok\n");
    return 0;
}
