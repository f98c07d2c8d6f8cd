// bm_share_set_args.hpp -- what the share set's kernels (bm_share_set.hpp) and their
// launcher (bm_aux.hip) agree on: ids, the control words of a call and the kernels'
// argument block.  Plain C++: no HIP in here.
#pragma once
#include <cstdint>

#include "bm_sha256.hpp"  // BM_HD
#include "btcminer.h"

namespace bm {

constexpr int kShareSetThreads = 64;           // one wave: the resolve kernel's ballot covers the workgroup
constexpr uint32_t kShareEmpty = 0xFFFFFFFFu;  // a free slot
constexpr uint32_t kShareCandidate = 0x80000000u;  // | the lane's index: this call's ids, above every persistent id
constexpr uint32_t kShareNone = 0xFFFFFFFFu;   // a lane without a slot / without a rank
constexpr int kShareVerdictWords = 10;         // bm_job_verdict_t: eight words of hash, status, reserved
constexpr int kShareKeyWords = 8;
// the control words of a call, zeroed by the host's copy up
constexpr int kShareCtlFault = 0;              // bit 0: a probe ran out; bit 1: an id out of range (a bug)
constexpr int kShareCtlWinners = 1;            // lanes that own their slot
constexpr int kShareCtlWords = 2;
constexpr uint32_t kShareFaultFull = 1u, kShareFaultId = 2u;

// Kernel argument of the four kernels, by value (SGPRs).
struct ShareSetArgs {
    uint32_t n;         // submissions
    uint32_t nslots;    // a power of two
    uint32_t count;     // persistent entries before the call
    uint32_t capacity;  // entries of keys[]
};

// A submission takes part in the set when it is a share or a block and was hashed.
BM_HD inline bool share_eligible(uint32_t status) {
    return (status & (BM_SUBMIT_SHARE | BM_SUBMIT_BLOCK)) != 0 && (status & BM_SUBMIT_INVALID) == 0;
}

}  // namespace bm
