// bm_share_set.hpp -- the kernels of bm_share_set_verify on a device set: the
// per-job set of header hashes behind duplicate-share detection (include/btcminer.h
// has the semantics; bm_aux.hip the host part).  They run after pool_verify_kernel
// on the same stream, one lane per submission, over its verdicts in device memory.
//
// The set is an insert-only open-addressing table of 32-bit entry ids:
//   keys[capacity]  the persistent hashes, eight words each as pool_verify_kernel
//                   stores them (bm_job_verdict_t.hash read as little-endian words),
//                   indexed by id; ids 0 .. count - 1 are in use (below 2^24);
//   slots[nslots]   ids, kShareEmpty where free; nslots a power of two, at least
//                   twice the capacity.
// During a call lane i's candidate id is kShareCandidate | i and its key is
// verdicts[i].hash: persistent ids order below every candidate, candidates by index.
//
//   share_insert_kernel   eligible lanes (SHARE or BLOCK, not INVALID) probe from
//       their home slot (the hash's least significant 32 bits mod nslots) with
//       old = atomicCAS(slot, EMPTY, id).  EMPTY: the slot is theirs.  Else they
//       compare their key with old's: equal -> atomicMin(slot, id), so the lowest
//       index wins or the persistent entry stays; different -> the next slot.  A
//       slot's key never changes once it is taken, so every lane of one key ends on
//       the same slot, whatever the order of arrival.  The lane remembers its slot.
//       At most nslots probes: a lane that runs out sets bit 0 of the overflow word.
//   share_resolve_kernel  a later launch, so plain loads see the final owners: a
//       lane whose slot holds its id is a winner; any other eligible lane ORs
//       BM_SUBMIT_DUPLICATE into its verdict.  Winners take a rank from one
//       atomicAdd per wave on the winner count.
//   share_commit_kernel   winners copy their key to keys[count + rank] and store
//       that id in their slot.
//   share_rollback_kernel winners store EMPTY.  After the insert only winners' ids
//       are candidates in the table, so this restores it exactly.
// Within share_insert_kernel a slot word is read only through the value an atomic
// returns; every other word is read in a later launch than the one that wrote it
// (the keys of earlier calls, this batch's hashes, the final owners).  Nothing
// spins, retries or waits on another lane; every loop is bounded by an argument.
// All stores are ordinary vector stores.  No LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bm_share_set_args.hpp"

namespace bm {

__global__ __launch_bounds__(kShareSetThreads) void share_insert_kernel(const ShareSetArgs A,
                                                                        const uint32_t* __restrict__ verdicts,
                                                                        const uint32_t* __restrict__ keys,
                                                                        uint32_t* __restrict__ slots,
                                                                        uint32_t* __restrict__ lane_slot,
                                                                        uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * kShareSetThreads + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t* v = verdicts + (size_t)kShareVerdictWords * i;
    uint32_t mine = kShareNone;
    if (share_eligible(v[8])) {
        uint32_t key[kShareKeyWords];
#pragma unroll
        for (int k = 0; k < kShareKeyWords; ++k) key[k] = v[k];
        const uint32_t id = kShareCandidate | i;
        const uint32_t mask = A.nslots - 1;
        uint32_t s = __builtin_bswap32(key[7]) & mask;  // hash[28..31], most significant byte first
        uint32_t fault = kShareFaultFull;               // the probes ran out, unless the loop says otherwise
        for (uint32_t probe = 0; probe < A.nslots; ++probe, s = (s + 1) & mask) {
            const uint32_t old = atomicCAS(&slots[s], kShareEmpty, id);
            if (old == kShareEmpty) {
                mine = s;
                fault = 0;
                break;
            }
            const uint32_t* other;
            if (old & kShareCandidate) {
                const uint32_t j = old & ~kShareCandidate;
                if (j >= A.n) {
                    fault = kShareFaultId;
                    break;
                }
                other = verdicts + (size_t)kShareVerdictWords * j;
            } else {
                if (old >= A.count) {
                    fault = kShareFaultId;
                    break;
                }
                other = keys + (size_t)kShareKeyWords * old;
            }
            uint32_t diff = 0;
#pragma unroll
            for (int k = 0; k < kShareKeyWords; ++k) diff |= other[k] ^ key[k];
            if (diff == 0) {
                atomicMin(&slots[s], id);
                mine = s;
                fault = 0;
                break;
            }
        }
        if (fault) atomicOr(&ctl[kShareCtlFault], fault);
    }
    lane_slot[i] = mine;
}

__global__ __launch_bounds__(kShareSetThreads) void share_resolve_kernel(const ShareSetArgs A,
                                                                         uint32_t* __restrict__ verdicts,
                                                                         const uint32_t* __restrict__ slots,
                                                                         const uint32_t* __restrict__ lane_slot,
                                                                         uint32_t* __restrict__ lane_rank,
                                                                         uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * kShareSetThreads + threadIdx.x;
    const bool live = i < A.n;  // no early return: the whole wave reaches the ballot
    const uint32_t s = live ? lane_slot[i] : kShareNone;
    const bool placed = s < A.nslots;
    const bool win = placed && slots[s] == (kShareCandidate | i);
    if (placed && !win) verdicts[(size_t)kShareVerdictWords * i + 8] |= BM_SUBMIT_DUPLICATE;
    const unsigned long long won = __ballot(win);
    uint32_t rank = kShareNone;
    if (won) {  // wave-uniform
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(won >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)won, 0u));
        uint32_t base = 0;
        if (win && before == 0) base = atomicAdd(&ctl[kShareCtlWinners], (uint32_t)__popcll(won));
        base = (uint32_t)__shfl((int)base, __ffsll((long long)won) - 1);
        if (win) rank = base + before;
    }
    if (live) lane_rank[i] = rank;
}

__global__ __launch_bounds__(kShareSetThreads) void share_commit_kernel(const ShareSetArgs A,
                                                                        const uint32_t* __restrict__ verdicts,
                                                                        uint32_t* __restrict__ keys,
                                                                        uint32_t* __restrict__ slots,
                                                                        const uint32_t* __restrict__ lane_slot,
                                                                        const uint32_t* __restrict__ lane_rank) {
    const uint32_t i = blockIdx.x * kShareSetThreads + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t rank = lane_rank[i], s = lane_slot[i];
    if (rank == kShareNone || s >= A.nslots) return;
    const uint32_t id = A.count + rank;
    if (id >= A.capacity) return;  // the host has checked count + winners <= capacity
    const uint32_t* v = verdicts + (size_t)kShareVerdictWords * i;
    uint32_t* key = keys + (size_t)kShareKeyWords * id;
#pragma unroll
    for (int k = 0; k < kShareKeyWords; ++k) key[k] = v[k];
    slots[s] = id;
}

__global__ __launch_bounds__(kShareSetThreads) void share_rollback_kernel(const ShareSetArgs A,
                                                                          uint32_t* __restrict__ slots,
                                                                          const uint32_t* __restrict__ lane_slot,
                                                                          const uint32_t* __restrict__ lane_rank) {
    const uint32_t i = blockIdx.x * kShareSetThreads + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t s = lane_slot[i];
    if (lane_rank[i] != kShareNone && s < A.nslots) slots[s] = kShareEmpty;
}

}  // namespace bm
