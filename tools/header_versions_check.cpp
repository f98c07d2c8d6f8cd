// header_versions_check.cpp -- stand-alone CPU check of the host half of the
// version-rolling block-header search (csrc/bm_header_versions.hpp):
//   * the schedule terms a kernel shares between its slots are the same for
//     every version, and the hash rebuilt from the shared and the slot terms
//     is the plain sha256d of the header with that version;
//   * the (nonce, version index) key packs and unpacks;
//   * the grouping into launches of 4, 2 and 1 versions covers each index once
//     and in order, for every list length and group cap;
//   * header_versions_select returns the pair the devices report and refuses a
//     forged report of each kind.
// Every array is an exactly-sized heap array, so the sanitizer sees any access
// past one.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc -I include tools/header_versions_check.cpp -o versions_check
//     && ./versions_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "bm_header_versions.hpp"

namespace {

using bm::host::hash_top64;

int fails = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++fails;
    }
}

const char* kHeaders[2] = {
    // the genesis block
    "0100000000000000000000000000000000000000000000000000000000000000000000003ba3edfd7a7b12b27ac72c3e67768f617f"
    "c81bc3888a51323a9fb8aa4b1e5e4a29ab5f49ffff001d1dac2b7c",
    // block 125552
    "0100000081cd02ab7e569e8bcd9317e2fe99f2de44d49ab2b8851ba4a308000000000000e320b6c2fffc8d750423db8b1eb942ae71"
    "0e951ed797f7affc8892b0f1fc122bc7f5d74df2b9441a42a14695"};
const uint32_t kFirstNonce[2] = {2083236893u - 10000u, 0xFFFFFFFFu - 19999u};  // the second window ends at 2^32 - 1

constexpr int kVersions = 5;
const uint32_t kVersionList[kVersions] = {0u, 1u, 0x20000000u, 0x3fffe000u, 0xffffffffu};
constexpr uint32_t kNoncesPerVersion = 20000;

template <int M>
void check_group(const uint8_t* header, const uint32_t* versions, size_t first, int m, uint32_t n0,
                 const bm::HeaderArgs& ref) {
    std::unique_ptr<bm::HeaderVersionsArgs<M>> A(new bm::HeaderVersionsArgs<M>);
    std::memset(A.get(), 0, sizeof *A);
    expect(bm::host::header_versions_precompute(header, versions, first, m, *A), "shared terms equal across a group");
    expect(A->w16 == ref.w16 && A->w17 == ref.w17 && A->k18 == ref.k18 && A->k19 == ref.k19 && A->k31 == ref.k31 &&
               A->k32 == ref.k32,
           "shared terms equal those of the caller's own header");
    for (int k = 0; k < m; ++k) {
        expect(A->slot[k].vidx == first + (size_t)k, "slot index");
        std::unique_ptr<uint8_t[]> h(new uint8_t[bm::kHeaderBytes]);
        bm::host::header_with_version(header, versions[first + (size_t)k], h.get());
        bool same = true;
        for (uint32_t i = 0; i < kNoncesPerVersion && same; ++i) {
            const uint32_t n = n0 + i;
            uint8_t a[32], b[32];
            bm::host::sha256d_header(h.get(), n, a);
            bm::host::sha256d_from_slot(*A, k, n, b);
            same = std::memcmp(a, b, 32) == 0;
        }
        expect(same, "hash from shared + slot terms == plain sha256d");
    }
}

}  // namespace

int main() {
    static_assert(sizeof(bm_header_versions_result_t) == 48, "result layout");
    static_assert(sizeof(bm::HeaderVersionSlot) == 17 * 4, "slot layout");
    static_assert(sizeof(bm::HeaderVersionsArgs<1>) == (20 + 17) * 4 && sizeof(bm::HeaderVersionsArgs<4>) == (20 + 68) * 4,
                  "argument layout: the shared part, then M slots");
    static_assert(BM_MAX_HEADER_VERSIONS == 64, "indices stay below 64");

    // ---- 1. shared terms and the rebuilt hash, both golden headers ----
    std::unique_ptr<uint8_t[]> header(new uint8_t[bm::kHeaderBytes]);
    std::unique_ptr<uint32_t[]> versions(new uint32_t[kVersions]);
    for (int i = 0; i < kVersions; ++i) versions[i] = kVersionList[i];
    for (int hi = 0; hi < 2; ++hi) {
        for (int i = 0; i < bm::kHeaderBytes; ++i) {
            unsigned v = 0;
            std::sscanf(kHeaders[hi] + 2 * i, "%2x", &v);
            header[i] = (uint8_t)v;
        }
        bm::HeaderArgs ref;
        std::memset(&ref, 0, sizeof ref);
        bm::host::header_precompute(header.get(), ref);
        for (int i = 0; i < kVersions; ++i) {  // one by one against the caller's header
            std::unique_ptr<uint8_t[]> h(new uint8_t[bm::kHeaderBytes]);
            bm::host::header_with_version(header.get(), versions[i], h.get());
            expect(std::memcmp(h.get() + 4, header.get() + 4, bm::kHeaderBytes - 4) == 0 && h[0] == (uint8_t)versions[i] &&
                       h[3] == (uint8_t)(versions[i] >> 24),
                   "only bytes 0..3 change");
            bm::HeaderArgs one;
            std::memset(&one, 0, sizeof one);
            bm::host::header_precompute(h.get(), one);
            expect(one.w16 == ref.w16 && one.w17 == ref.w17 && one.k18 == ref.k18 && one.k19 == ref.k19 &&
                       one.k31 == ref.k31 && one.k32 == ref.k32,
                   "schedule terms identical across versions");
            if (versions[i] != 1u)  // both golden headers carry version 1
                expect(std::memcmp(one.mid, ref.mid, sizeof one.mid) != 0, "the midstate does change");
        }
        // the groups a 5-version call makes: 4 + 1, and under caps 2 and 1
        check_group<4>(header.get(), versions.get(), 0, 4, kFirstNonce[hi], ref);
        check_group<1>(header.get(), versions.get(), 4, 1, kFirstNonce[hi], ref);
        check_group<2>(header.get(), versions.get(), 2, 2, kFirstNonce[hi], ref);
    }

    // ---- 2. key packing ----
    {
        const uint32_t ns[] = {0u, 1u, 255u, 256u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
        for (uint32_t n : ns)
            for (uint32_t i = 0; i < BM_MAX_HEADER_VERSIONS; ++i) {
                const uint64_t k = bm::host::versions_key(n, i);
                expect(bm::host::key_nonce(k) == n && bm::host::key_index(k) == i && k != UINT64_MAX, "key round trip");
            }
        expect(bm::host::versions_key(5, 63) < bm::host::versions_key(6, 0), "ordered by nonce first");
        expect(bm::host::versions_key(5, 2) < bm::host::versions_key(5, 3), "then by index");
    }

    // ---- 3. grouping ----
    for (int cap = 1; cap <= 4; cap *= 2)
        for (size_t nver = 1; nver <= BM_MAX_HEADER_VERSIONS; ++nver) {
            std::unique_ptr<uint8_t[]> sizes(new uint8_t[BM_MAX_HEADER_VERSIONS]);
            const int ng = bm::host::versions_groups(nver, cap, sizes.get());
            size_t at = 0;
            bool ok = ng >= 1 && ng <= BM_MAX_HEADER_VERSIONS;
            for (int g = 0; ok && g < ng; ++g) {
                ok = (sizes[g] == 1 || sizes[g] == 2 || sizes[g] == 4) && sizes[g] <= cap &&
                     (g == 0 || sizes[g] <= sizes[g - 1]);  // 4s, then 2s, then 1s
                at += sizes[g];  // group g holds indices [at - size, at): once each, in order
            }
            expect(ok && at == nver, "groups cover every index once, in order");
            if (cap == 4) expect((size_t)ng == nver / 4 + (nver % 4) / 2 + nver % 2, "greedy: as few launches as possible");
        }

    // ---- 4. the host's selection, true and forged reports ----
    {
        for (int i = 0; i < bm::kHeaderBytes; ++i) {
            unsigned v = 0;
            std::sscanf(kHeaders[0] + 2 * i, "%2x", &v);
            header[i] = (uint8_t)v;
        }
        // truth over a small window: every pair's hash
        const uint32_t lo = 1000, n = 2000;
        uint8_t target[32];
        std::memset(target, 0xFF, sizeof target);
        target[0] = 0x00;
        target[1] = 0x3F;  // 10 leading zero bits: about 10 of the 10000 pairs
        uint64_t hit = UINT64_MAX;
        bm::Partial best{UINT64_MAX, UINT64_MAX};
        uint64_t miss = UINT64_MAX;  // some pair above the target
        for (uint32_t k = 0; k < n; ++k)
            for (uint32_t i = 0; i < (uint32_t)kVersions; ++i) {
                std::unique_ptr<uint8_t[]> h(new uint8_t[bm::kHeaderBytes]);
                bm::host::header_with_version(header.get(), versions[i], h.get());
                uint8_t hash[32];
                bm::host::header_hash_msb(h.get(), lo + k, hash);
                const uint64_t key = bm::host::versions_key(lo + k, i);
                if (std::memcmp(hash, target, 32) <= 0) {
                    if (key < hit) hit = key;
                } else if (miss == UINT64_MAX) {
                    miss = key;
                }
                const uint64_t top = hash_top64(hash);
                if (top < best.hash || (top == best.hash && key < best.nonce)) best = bm::Partial{top, key};
            }
        expect(hit != UINT64_MAX, "the window holds a hit");
        std::unique_ptr<bm_header_versions_result_t> out(new bm_header_versions_result_t);
        std::memset(out.get(), 0xA5, sizeof *out);
        const bm_header_versions_result_t untouched = *out;

        expect(bm::host::header_versions_select(header.get(), versions.get(), kVersions, target, hit, best, out.get()) ==
                       BM_OK &&
                   out->found == 1 && out->nonce == bm::host::key_nonce(hit) &&
                   out->version_index == bm::host::key_index(hit) && out->version == versions[out->version_index] &&
                   std::memcmp(out->hash, target, 32) <= 0,
               "a true hit is returned");
        uint8_t zero[32] = {};
        std::memset(out.get(), 0xA5, sizeof *out);
        expect(bm::host::header_versions_select(header.get(), versions.get(), kVersions, zero, UINT64_MAX, best,
                                                out.get()) == BM_OK &&
                   out->found == 0 && bm::host::versions_key(out->nonce, out->version_index) == best.nonce &&
                   hash_top64(out->hash) == best.hash && out->version == versions[out->version_index],
               "a true best share is returned");

        std::memset(out.get(), 0xA5, sizeof *out);
        struct Forge {
            const char* what;
            const uint8_t* target;
            uint64_t hit;
            bm::Partial best;
        };
        const Forge forges[] = {
            {"a hit above the target", target, miss, best},
            {"a hit whose index is out of range", target, bm::host::versions_key(bm::host::key_nonce(hit), kVersions),
             best},
            {"a hit whose index is far out of range", target, bm::host::versions_key(bm::host::key_nonce(hit), 0xFFFFFFFEu),
             best},
            {"a best share at or below the target with no hit", target, UINT64_MAX, best},
            {"a best share whose index is out of range", zero, UINT64_MAX,
             bm::Partial{best.hash, bm::host::versions_key(bm::host::key_nonce(best.nonce), kVersions)}},
            {"a best share with wrong top 64 bits", zero, UINT64_MAX, bm::Partial{best.hash ^ 1, best.nonce}},
            {"no partial at all", zero, UINT64_MAX, bm::Partial{UINT64_MAX, UINT64_MAX}},
        };
        for (const Forge& f : forges) {
            expect(bm::host::header_versions_select(header.get(), versions.get(), kVersions, f.target, f.hit, f.best,
                                                    out.get()) == BM_EINTERNAL,
                   f.what);
            expect(std::memcmp(out.get(), &untouched, sizeof untouched) == 0, "a refused report leaves out untouched");
        }
        // one version: index 0 is the only legal one
        expect(bm::host::header_versions_select(header.get(), versions.get(), 1, zero, UINT64_MAX,
                                                bm::Partial{best.hash, bm::host::versions_key(lo, 1)},
                                                out.get()) == BM_EINTERNAL,
               "index 1 of a one-version list");
    }

    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("header versions check ok\n");
    return 0;
}
