// bm_header_kernels.hpp -- the device pieces of the Bitcoin block-header
// kernels, built from the SHA-256 pieces of bm_kernels.hpp: blocks with
// compile-time words (HeaderBlock2, DigestBlock, block_const, sched_word,
// block_round) and the 256-bit compare (le256).  No kernel in here: the units
// that include it hold their own (bm_header_versions_inst.hip and
// bm_header_versions_hits_inst.hip over bm_header_versions_body.inc, which run
// all four block-header searches; bm_job_verify_inst.hip; bm_header_inst.hip
// uses none of this, on purpose).
//
// What the body makes of these pieces, per nonce n and per version slot
// (bm_header.hpp has the per-call host part):
//   * W3 = bswap32(n).  n = (task << 8) | j: the task part is per lane, the
//     low byte j is the wave-uniform inner counter, so W3 = wl | J with
//     wl = bswap32(task << 8) (bits 0..23) and J = j << 24 (bits 24..31) in
//     disjoint bits, and sigma0(W3) = sigma0(wl) ^ sigma0(J): a per-task value
//     and one the scalar unit steps (ssig0_salu);
//   * first hash: rounds 3..63 of block 2 (round 3 is two adds on host
//     terms), words 4..15 folded as constants, plus the midstate;
//   * second hash: the digest as words 0..7 of one block from the IV, words
//     8..15 folded as constants.  Only digest word 7 decides the hot path: it
//     is IV[7] + the e that round 60 produces, so 61 rounds run per nonce and
//     rounds 61..63 only on the rare path.
//   * hot-path compare: bswap32(digest word 7), the hash's top 32 bits, against
//     max(best top word, target top word) kept in one register (as hits mode
//     does): every hit and every new minimum takes the rare branch, in
//     whatever order a lane visits its nonces.
//   * rare path: finish the digest; exact 256-bit compare against the target
//     (8 kernarg words) and the range check; a hit records its key, (n << 32) |
//     version index, with one atomicMin on the device's hit word; the running
//     minimum is the lexicographic min of (top 64 bits, key).
//   * early exit: at each dequeue lane 0 reads the hit word (relaxed, agent
//     scope); a wave whose chunk starts above the recorded nonce leaves.
//     Nothing waits on another wave; only nonces above a recorded hit are
//     ever skipped, so the smallest hit is always hashed and recorded.
// bm_header_versions_inst.hip says what M slots over one schedule add to this.
#pragma once
#include "bm_header.hpp"
#include "bm_kernels.hpp"

namespace bm {

constexpr uint32_t csig0(uint32_t x) { return crotr(x, 7) ^ crotr(x, 18) ^ (x >> 3); }
constexpr uint32_t csig1(uint32_t x) { return crotr(x, 17) ^ crotr(x, 19) ^ (x >> 10); }

// Compile-time words of a block: v[k] >= 0 is the value of word k, -1 a
// run-time word.
struct HeaderBlock2 {  // header[64:76], the nonce, 0x80, zeros, 640 bits
    static constexpr int64_t v[16] = {-1, -1, -1, -1, 0x80000000ll, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 640};
};
struct DigestBlock {  // a 32-byte digest, 0x80, zeros, 256 bits
    static constexpr int64_t v[16] = {-1, -1, -1, -1, -1, -1, -1, -1, 0x80000000ll, 0, 0, 0, 0, 0, 0, 256};
};
template <class C>
constexpr int64_t block_const(int k) {
    return (k >= 0 && k < 16) ? C::v[k] : -1;
}

// Schedule word t >= 16 of a block whose constant words are C's: the
// constant terms fold into one literal, only run-time terms cost ops.
// w holds W[k] at w[k & 15] for the run-time words of the last 16.
template <class C, int t>
BM_DEV uint32_t sched_word(const uint32_t (&w)[16]) {
    constexpr int64_t c2 = block_const<C>(t - 2), c7 = block_const<C>(t - 7), c15 = block_const<C>(t - 15),
                      c16 = block_const<C>(t - 16);
    constexpr uint32_t k = (c2 >= 0 ? csig1((uint32_t)c2) : 0u) + (c7 >= 0 ? (uint32_t)c7 : 0u) +
                           (c15 >= 0 ? csig0((uint32_t)c15) : 0u) + (c16 >= 0 ? (uint32_t)c16 : 0u);
    uint32_t r = 0;
    bool any = false;
    auto add = [&](uint32_t x) {
        r = any ? r + x : x;
        any = true;
    };
    if constexpr (c2 < 0) add(ssig1(w[(t - 2) & 15]));
    if constexpr (c7 < 0) add(w[(t - 7) & 15]);
    if constexpr (c15 < 0) add(ssig0(w[(t - 15) & 15]));
    if constexpr (c16 < 0) add(w[t & 15]);
    if constexpr (k != 0) add(k);
    return r;
}

// Round t of a block with constant words C: the word from the window, or
// its literal.
template <class C, int t>
BM_DEV void block_round(uint32_t (&s)[8], uint32_t (&w)[16]) {
    if constexpr (t < 16) {
        if constexpr (block_const<C>(t) >= 0)
            sha_round<t>(s, (uint32_t)block_const<C>(t));
        else
            sha_round<t>(s, w[t]);
    } else {
        w[t & 15] = sched_word<C, t>(w);
        sha_round<t>(s, w[t & 15]);
    }
}

// 256-bit h <= t, both most significant word first.
BM_DEV bool le256(const uint32_t (&h)[8], const uint32_t (&t)[8]) {
    bool le = true;
#pragma unroll
    for (int i = 7; i >= 0; --i) le = h[i] < t[i] || (h[i] == t[i] && le);
    return le;
}

}  // namespace bm
