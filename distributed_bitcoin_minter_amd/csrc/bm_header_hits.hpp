// bm_header_hits.hpp -- the host's half of bm_search_header_hits_gpu: what the
// devices appended (16-byte entries {top 64 bits of H(n), n}, in whatever order
// their lanes took their slots) becomes the caller's list, and every entry's
// claim is checked on the way.  Shared by the launcher (bm_search.cpp) and a
// stand-alone CPU check (tools/header_hits_check.cpp).  Plain C++: no HIP in here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "bm_common.h"
#include "bm_header.hpp"
#include "btcminer.h"

namespace bm {
namespace host {

// entries: device 0's counts[0] entries, then device 1's counts[1], ... (ndev
// devices); they are sorted by nonce in place.  out gets one bm_header_hit_t
// per entry, ascending by nonce, with the full hash recomputed here
// (header_hash_msb).  BM_EINTERNAL unless every entry is what the kernel may
// write: a nonce of [lo, hi] that appears once, whose hash is at or below the
// target (256 bits, most significant byte first) and has the entry's top 64 bits.
inline int header_hits_collect(const uint8_t header[kHeaderBytes], const uint8_t target[32], uint32_t lo,
                               uint32_t hi, Partial* entries, const size_t* counts, int ndev,
                               bm_header_hit_t* out) {
    size_t n = 0;
    for (int di = 0; di < ndev; ++di) n += counts[di];
    std::sort(entries, entries + n, [](const Partial& a, const Partial& b) { return a.nonce < b.nonce; });
    for (size_t i = 0; i < n; ++i) {
        const Partial& e = entries[i];
        if (e.nonce < lo || e.nonce > hi) return BM_EINTERNAL;
        if (i > 0 && e.nonce == entries[i - 1].nonce) return BM_EINTERNAL;
        bm_header_hit_t h;
        header_hash_msb(header, (uint32_t)e.nonce, h.hash);
        h.nonce = (uint32_t)e.nonce;
        h.reserved = 0;
        if (std::memcmp(h.hash, target, 32) > 0) return BM_EINTERNAL;
        if (hash_top64(h.hash) != e.hash) return BM_EINTERNAL;
        out[i] = h;
    }
    return BM_OK;
}

}  // namespace host
}  // namespace bm
