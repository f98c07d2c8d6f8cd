// bm_header_versions_hits.hpp -- the host's half of
// bm_search_header_versions_hits_gpu and of bm_search_header_hits_gpu, its
// one-version case: what the devices appended (16-byte entries
// {top 64 bits of H(i, n), (n << 32) | i}, in whatever order the lanes of all
// their group launches took their slots) becomes the caller's list, and every
// entry's claim is checked on the way; so is the best share.  Shared by the
// launcher (bm_search.cpp) and a stand-alone CPU check
// (tools/header_versions_hits_check.cpp).  Plain C++: no HIP in here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "bm_common.h"
#include "bm_header.hpp"
#include "bm_header_versions.hpp"
#include "btcminer.h"

namespace bm {
namespace host {

// One entry of the caller's list from a checked pair (h.hash is filled already):
// bm_search_header_versions_hits_gpu's entry carries the version,
// bm_search_header_hits_gpu's (one version, the header's own) does not.
inline void fill_hit(bm_header_version_hit_t& h, uint32_t nonce, uint32_t vi, uint32_t version) {
    h.nonce = nonce;
    h.version_index = vi;
    h.version = version;
    h.reserved = 0;
}
inline void fill_hit(bm_header_hit_t& h, uint32_t nonce, uint32_t, uint32_t) {
    h.nonce = nonce;
    h.reserved = 0;
}

// entries: device 0's counts[0] entries, then device 1's counts[1], ... (ndev
// devices); they are sorted by key, that is by (nonce, version index), in
// place.  out gets one Hit (bm_header_version_hit_t or bm_header_hit_t) per
// entry in that order, with the full hash recomputed here under that entry's
// version (header_with_version, header_hash_msb).  BM_EINTERNAL unless every
// entry is what the kernel may write: an index below nver, a nonce of [lo, hi],
// a key that appears once, a hash at or below the target (256 bits, most
// significant byte first) that has the entry's top 64 bits.
template <class Hit>
inline int header_versions_hits_collect(const uint8_t header[kHeaderBytes], const uint32_t* versions, size_t nver,
                                        const uint8_t target[32], uint32_t lo, uint32_t hi, Partial* entries,
                                        const size_t* counts, int ndev, Hit* out) {
    size_t n = 0;
    for (int di = 0; di < ndev; ++di) n += counts[di];
    std::sort(entries, entries + n, [](const Partial& a, const Partial& b) { return a.nonce < b.nonce; });
    for (size_t i = 0; i < n; ++i) {
        const Partial& e = entries[i];
        const uint32_t nonce = key_nonce(e.nonce), vi = key_index(e.nonce);
        if (vi >= nver) return BM_EINTERNAL;
        if (nonce < lo || nonce > hi) return BM_EINTERNAL;
        if (i > 0 && e.nonce == entries[i - 1].nonce) return BM_EINTERNAL;
        Hit h;
        uint8_t hv[kHeaderBytes];
        header_with_version(header, versions[vi], hv);
        header_hash_msb(hv, nonce, h.hash);
        fill_hit(h, nonce, vi, versions[vi]);
        if (std::memcmp(h.hash, target, 32) > 0) return BM_EINTERNAL;
        if (hash_top64(h.hash) != e.hash) return BM_EINTERNAL;
        out[i] = h;
    }
    return BM_OK;
}

// The best share of a call from the minimum of the devices' (top 64 bits, key)
// partials, checked as header_versions_select checks its not-found answer, and
// against the count: a best share at or below the target is itself a hit, so
// with a count of zero it is BM_EINTERNAL.  out's hash, nonce, version_index,
// version and reserved are written on BM_OK only; count and stored are the
// caller's.
inline int header_versions_hits_best(const uint8_t header[kHeaderBytes], const uint32_t* versions, size_t nver,
                                     const uint8_t target[32], const Partial& best, uint64_t count,
                                     bm_header_versions_hits_result_t* out) {
    const uint32_t vi = key_index(best.nonce);
    if (best.nonce == UINT64_MAX || vi >= nver) return BM_EINTERNAL;  // a non-empty range always has a minimum
    uint8_t hash[32], hv[kHeaderBytes];
    header_with_version(header, versions[vi], hv);
    header_hash_msb(hv, key_nonce(best.nonce), hash);
    if (hash_top64(hash) != best.hash) return BM_EINTERNAL;
    if (count == 0 && std::memcmp(hash, target, 32) <= 0) return BM_EINTERNAL;
    std::memcpy(out->hash, hash, sizeof hash);
    out->nonce = key_nonce(best.nonce);
    out->version_index = vi;
    out->version = versions[vi];
    out->reserved = 0;
    return BM_OK;
}

}  // namespace host
}  // namespace bm
