// header_hits_check.cpp -- stand-alone CPU check of the host half of the
// block-header share enumeration (csrc/bm_header_hits.hpp, header_hits_collect):
// entries as 1 to 3 devices would leave them (shuffled, some devices empty)
// come back sorted with their full hashes; a forged entry of each kind is
// refused; a buffer filled exactly to its capacity is written to its last
// entry and not past it.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/header_hits_check.cpp -o hits_check && ./hits_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bm_header_hits.hpp"

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

uint32_t rng_state = 0x9E3779B9u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// Every hit of [lo, hi] at `target`, ascending: what the devices report.
std::vector<bm::Partial> true_hits(const uint8_t* header, const uint8_t* target, uint32_t lo, uint32_t hi) {
    std::vector<bm::Partial> v;
    for (uint64_t n = lo; n <= hi; ++n) {
        uint8_t h[32];
        bm::host::header_hash_msb(header, (uint32_t)n, h);
        if (std::memcmp(h, target, 32) <= 0) v.push_back(bm::Partial{hash_top64(h), n});
    }
    return v;
}

// The collect over exactly-sized heap arrays (the sanitizer sees any access past them).
int collect(const uint8_t* header, const uint8_t* target, uint32_t lo, uint32_t hi, const std::vector<bm::Partial>& in,
            const std::vector<size_t>& counts, std::vector<bm_header_hit_t>& out) {
    std::unique_ptr<bm::Partial[]> e(new bm::Partial[in.size()]);
    std::unique_ptr<bm_header_hit_t[]> o(new bm_header_hit_t[in.size()]);
    std::memset(o.get(), 0xA5, in.size() * sizeof(bm_header_hit_t));
    for (size_t i = 0; i < in.size(); ++i) e[i] = in[i];
    const int rc = bm::host::header_hits_collect(header, target, lo, hi, e.get(), counts.data(), (int)counts.size(),
                                                 o.get());
    out.assign(o.get(), o.get() + in.size());
    return rc;
}

}  // namespace

int main() {
    static_assert(sizeof(bm_header_hit_t) == 40, "hit entry layout");
    static_assert(sizeof(bm_header_hits_result_t) == 56, "result layout");
    uint8_t header[bm::kHeaderBytes];
    for (int i = 0; i < bm::kHeaderBytes; ++i) {
        unsigned v = 0;
        std::sscanf(kGenesis + 2 * i, "%2x", &v);
        header[i] = (uint8_t)v;
    }
    const uint32_t lo = 1000, hi = 20999;
    uint8_t target[32];
    std::memset(target, 0xFF, sizeof target);
    target[0] = 0x03;  // 6 leading zero bits: about 300 of 20000
    const std::vector<bm::Partial> truth = true_hits(header, target, lo, hi);
    expect(truth.size() > 100 && truth.size() < 1000, "the window holds a few hundred hits");

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
            expect(collect(header, target, lo, hi, in, counts, out) == BM_OK, "true entries are accepted");
            bool same = out.size() == truth.size();
            for (size_t i = 0; same && i < out.size(); ++i) {
                uint8_t h[32];
                bm::host::header_hash_msb(header, (uint32_t)truth[i].nonce, h);
                same = out[i].nonce == truth[i].nonce && out[i].reserved == 0 && std::memcmp(out[i].hash, h, 32) == 0;
            }
            expect(same, "sorted by nonce with the full hashes");
        }
    }

    // no entries at all: nothing is read or written (null arrays)
    {
        const size_t none[3] = {0, 0, 0};
        expect(bm::host::header_hits_collect(header, target, lo, hi, nullptr, none, 3, nullptr) == BM_OK, "no entries");
    }

    // a forged entry of each kind, in a list that is otherwise true
    struct Forge {
        const char* what;
        bm::Partial entry;
        bool replace;  // put it in place of entry 5 (else: append it)
    };
    uint8_t h[32];
    uint32_t miss = lo;  // a nonce of the range that is no hit
    for (;; ++miss) {
        bm::host::header_hash_msb(header, miss, h);
        if (std::memcmp(h, target, 32) > 0) break;
    }
    const uint64_t miss_top = hash_top64(h);
    uint32_t below = lo - 1, above = hi + 1;  // hits outside the range, if they were in it
    uint8_t ones[32];
    std::memset(ones, 0xFF, sizeof ones);
    bm::host::header_hash_msb(header, below, h);
    const uint64_t below_top = hash_top64(h);
    bm::host::header_hash_msb(header, above, h);
    const uint64_t above_top = hash_top64(h);
    const Forge forges[] = {
        {"a nonce whose hash is above the target", {miss_top, miss}, true},
        {"a wrong top 64 bits", {truth[5].hash ^ 1, truth[5].nonce}, true},
        {"a wrong top 64 bits, high word", {truth[5].hash ^ (1ull << 63), truth[5].nonce}, true},
        {"a nonce below the range", {below_top, below}, false},
        {"a nonce above the range", {above_top, above}, false},
        {"a nonce past 32 bits", {truth[5].hash, truth[5].nonce | (1ull << 32)}, true},
        {"a nonce twice", truth[7], false},
        {"a nonce twice, across devices", truth.back(), true},
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
        // with every nonce a hit (target all ones) the range and the duplicate checks stand alone
        const bool range_only = f.entry.nonce == below || f.entry.nonce == above;
        expect(collect(header, range_only ? ones : target, lo, hi, range_only ? std::vector<bm::Partial>{f.entry} : in,
                       range_only ? std::vector<size_t>{1} : counts, out) == BM_EINTERNAL,
               f.what);
    }

    // count == cap: the caller's array has exactly as many entries as there are hits
    {
        std::vector<bm::Partial> in(truth.rbegin(), truth.rend());
        std::vector<bm_header_hit_t> out;
        expect(collect(header, target, lo, hi, in, {in.size()}, out) == BM_OK && out.back().nonce == truth.back().nonce &&
                   out.front().nonce == truth.front().nonce,
               "a buffer filled to its last entry");
    }

    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("header hits check ok\n");
    return 0;
}
