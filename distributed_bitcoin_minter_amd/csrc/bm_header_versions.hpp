// bm_header_versions.hpp -- version-rolling block-header search
// (bm_search_header_versions_gpu): what the host works out per call and how it
// selects and checks the answer, shared by the launcher (bm_search.cpp), the
// kernel (bm_header_versions_inst.hip) and a stand-alone CPU check
// (tools/header_versions_check.cpp).  Plain C++: no HIP in here.
//
// H(i, n) is bm_header.hpp's H(n) of the header whose bytes 0..3 are
// le32(versions[i]).  The version lies in block 1, so it changes the midstate
// and what follows from it (rounds 0..3 of block 2: mid, a3k, e3k, r4), never
// the words of block 2: w16, w17, k18, k19, k31, k32 and with them the whole
// 48-word schedule of block 2 are the same for every version.  A kernel that
// runs M versions ("slots") through block 2 in lock-step computes that
// schedule once per nonce (overt AsicBoost).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "bm_common.h"
#include "bm_header.hpp"
#include "btcminer.h"

namespace bm {

constexpr int kMaxVersionSlots = 4;  // header_versions_kernel<M>: M = 1, 2, 4

// What one slot (one version) of a launch adds to the shared terms.
struct HeaderVersionSlot {
    uint32_t mid[8];    // state after block 1 with this version
    uint32_t a3k, e3k;  // round 3 of block 2: a = a3k + W3, e = e3k + W3
    uint32_t r4[6];     // roles b, c, d, f, g, h entering round 4
    uint32_t vidx;      // index of the version in the caller's list
};

// Kernel argument of header_versions_kernel<M>, by value (SGPRs).  The shared
// part comes first, so HeaderVersionsArgs<M> is a prefix of HeaderVersionsArgs<4>.
template <int M>
struct HeaderVersionsArgs {
    uint32_t w16, w17;  // HeaderArgs' schedule terms: the same for every version
    uint32_t k18, k19;
    uint32_t k31, k32;
    uint32_t tgt[8];    // the target, most significant word first
    uint32_t lo, hi;    // inclusive nonce range of this launch
    uint32_t t0;        // first task: task t covers nonces [t << 8, (t << 8) + 255]
    uint32_t ntask;     // tasks t0 .. t0 + ntask - 1
    uint32_t chunk_m;   // tasks per lane per dequeued chunk
    uint32_t part_off;  // first partial slot written by this launch
    HeaderVersionSlot slot[M];
};

namespace host {

// A (nonce, version index) pair as one 64-bit key: ordered as (n, i), and below
// all-ones for every index the ABI allows (i < 64), so all-ones means "none".
inline uint64_t versions_key(uint32_t nonce, uint32_t vidx) { return ((uint64_t)nonce << 32) | vidx; }
inline uint32_t key_nonce(uint64_t key) { return (uint32_t)(key >> 32); }
inline uint32_t key_index(uint64_t key) { return (uint32_t)key; }

// The version list cut greedily into groups of 4, then 2, then 1 slots, none
// above cap (1, 2 or 4): sizes[] gets the group sizes in list order; returns
// how many.  No padded slots: the sizes add up to nver.
inline int versions_groups(size_t nver, int cap, uint8_t sizes[BM_MAX_HEADER_VERSIONS]) {
    int n = 0;
    size_t left = nver;
    for (int m = kMaxVersionSlots; m >= 1; m /= 2) {
        if (m > cap) continue;
        while (left >= (size_t)m) {
            sizes[n++] = (uint8_t)m;
            left -= (size_t)m;
        }
    }
    return n;
}

// The version field of a header as it stands, le32(header[0..3]): the one-entry
// list under which a search hashes the caller's bytes unchanged.
inline uint32_t header_version(const uint8_t header[kHeaderBytes]) {
    return (uint32_t)header[0] | (uint32_t)header[1] << 8 | (uint32_t)header[2] << 16 | (uint32_t)header[3] << 24;
}

// The caller's header with le32(version) in bytes 0..3.
inline void header_with_version(const uint8_t header[kHeaderBytes], uint32_t version, uint8_t out[kHeaderBytes]) {
    std::memcpy(out, header, kHeaderBytes);
    out[0] = (uint8_t)version;
    out[1] = (uint8_t)(version >> 8);
    out[2] = (uint8_t)(version >> 16);
    out[3] = (uint8_t)(version >> 24);
}

// One header_precompute per version: slot k of A gets version first + k, the
// shared terms are taken from the first.  false when a later version gives
// other shared terms (it cannot: they depend on bytes 64..75 alone).
template <int M>
inline bool header_versions_precompute(const uint8_t header[kHeaderBytes], const uint32_t* versions, size_t first,
                                       int m, HeaderVersionsArgs<M>& A) {
    bool same = true;
    for (int k = 0; k < m && k < M; ++k) {
        uint8_t h[kHeaderBytes];
        header_with_version(header, versions[first + (size_t)k], h);
        HeaderArgs one;
        std::memset(&one, 0, sizeof one);
        header_precompute(h, one);
        if (k == 0) {
            A.w16 = one.w16;
            A.w17 = one.w17;
            A.k18 = one.k18;
            A.k19 = one.k19;
            A.k31 = one.k31;
            A.k32 = one.k32;
        } else {
            same = same && A.w16 == one.w16 && A.w17 == one.w17 && A.k18 == one.k18 && A.k19 == one.k19 &&
                   A.k31 == one.k31 && A.k32 == one.k32;
        }
        HeaderVersionSlot& s = A.slot[k];
        std::memcpy(s.mid, one.mid, sizeof s.mid);
        s.a3k = one.a3k;
        s.e3k = one.e3k;
        std::memcpy(s.r4, one.r4, sizeof s.r4);
        s.vidx = (uint32_t)(first + (size_t)k);
    }
    return same;
}

// The double hash of one slot's nonce the way the kernel computes it, from the
// shared and the slot terms.  Only for checking the precompute on the CPU.
template <int M>
inline void sha256d_from_slot(const HeaderVersionsArgs<M>& A, int k, uint32_t nonce, uint8_t digest[32]) {
    HeaderArgs one;
    std::memset(&one, 0, sizeof one);
    const HeaderVersionSlot& s = A.slot[k];
    std::memcpy(one.mid, s.mid, sizeof one.mid);
    one.a3k = s.a3k;
    one.e3k = s.e3k;
    std::memcpy(one.r4, s.r4, sizeof one.r4);
    one.w16 = A.w16;
    one.w17 = A.w17;
    one.k18 = A.k18;
    one.k19 = A.k19;
    one.k31 = A.k31;
    one.k32 = A.k32;
    sha256d_from_args(one, nonce, digest);
}

// The answer of a call from what the devices report, checked against the
// host's own hash.  hit: the smallest key any device recorded (all-ones:
// none); best: the lexicographic minimum of the (top 64 bits, key) partials.
// BM_EINTERNAL when the claim does not hold: an index out of range, a hit
// whose hash is above the target, a best share whose top 64 bits differ or
// that meets the target although no hit was recorded.  out is written on
// BM_OK only.
inline int header_versions_select(const uint8_t header[kHeaderBytes], const uint32_t* versions, size_t nver,
                                  const uint8_t target[32], uint64_t hit, const Partial& best,
                                  bm_header_versions_result_t* out) {
    const bool found = hit != UINT64_MAX;
    const uint64_t key = found ? hit : best.nonce;
    const uint32_t vi = key_index(key);
    if (key == UINT64_MAX || vi >= nver) return BM_EINTERNAL;  // a non-empty range always has a minimum
    bm_header_versions_result_t r;
    std::memset(&r, 0, sizeof r);
    uint8_t h[kHeaderBytes];
    header_with_version(header, versions[vi], h);
    header_hash_msb(h, key_nonce(key), r.hash);
    r.nonce = key_nonce(key);
    r.version_index = vi;
    r.version = versions[vi];
    r.found = found ? 1 : 0;
    const bool meets = std::memcmp(r.hash, target, 32) <= 0;
    if (found ? !meets : (meets || hash_top64(r.hash) != best.hash)) return BM_EINTERNAL;
    *out = r;
    return BM_OK;
}

}  // namespace host
}  // namespace bm
