// sessions_host_share.cpp -- the host's part of bm_sessions_retarget on a device table,
// alone, for tools/bench_sessions.py: the ordering of the change list by session, the
// recheck of every target with bm_target_from_difficulty_fx and the list applied to
// the mirror arrays (csrc/bm_aux.hip's sessions_retarget_impl and
// csrc/bm_sessions_host.hpp's sessions_apply_changes, restated over plain arrays).
//
//   g++ -O2 -std=c++17 -fPIC -shared -I include tools/sessions_host_share.cpp
//     distributed_bitcoin_minter_amd/csrc/bm_job.cpp -I distributed_bitcoin_minter_amd/csrc -o sessions_host_share.so
#include <algorithm>
#include <cstring>
#include <vector>

#include "btcminer.h"

extern "C" int bench_sessions_host_share(const bm_vardiff_change_t* list, size_t k, uint32_t count, bm_vardiff_change_t* changes,
                                         bm_pool_session_t* sessions, uint64_t* weights) {
    if (k * 16 < count) {  // sessions_order_changes: a short list is sorted, a long one placed by session
        std::memcpy(changes, list, k * sizeof(bm_vardiff_change_t));
        std::sort(changes, changes + k,
                  [](const bm_vardiff_change_t& a, const bm_vardiff_change_t& b) { return a.session < b.session; });
    } else {
        std::vector<uint32_t> at(count, 0xFFFFFFFFu);
        size_t placed = 0;
        for (size_t i = 0; i < k; ++i) at[list[i].session] = (uint32_t)i;
        for (uint32_t s = 0; s < count; ++s)
            if (at[s] != 0xFFFFFFFFu) changes[placed++] = list[at[s]];
    }
    int bad = 0;
    for (size_t i = 0; i < k; ++i) {
        const bm_vardiff_change_t& c = changes[i];
        uint8_t want[32];
        bad += (i && changes[i - 1].session >= c.session) || c.old_fx != weights[c.session] ||
               bm_target_from_difficulty_fx(c.new_fx, want) != BM_OK || std::memcmp(want, c.target, 32) != 0;
    }
    for (size_t i = 0; i < k; ++i) {
        weights[changes[i].session] = changes[i].new_fx;
        std::memcpy(sessions[changes[i].session].target, changes[i].target, 32);
    }
    return bad;
}
