// bm_header_kernels.hpp -- gfx950 kernels for the Bitcoin block-header search
// (bm_search_header_gpu / bm_search_header_hits_gpu / bm_header_hash_gpu),
// built from the SHA-256 pieces of bm_kernels.hpp.  Two build units:
// bm_header_inst.hip (header_kernel, header_hash_kernel) and
// bm_header_hits_inst.hip (header_hits_kernel: header_kernel's body in hits
// mode; the two share bm_header_body.inc).  A third unit,
// bm_header_versions_inst.hip, takes only the pieces (BM_HEADER_PIECES_ONLY)
// for its own header_versions_kernel<M>.
//
// header_kernel, per nonce n (bm_header.hpp has the per-call host part):
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
//     (8 kernarg words) and the range check; a hit records its nonce with one
//     atomicMin on the device's hit word; the running minimum is the
//     lexicographic min of (top 64 bits, nonce).
//   * early exit: at each dequeue lane 0 reads the hit word (relaxed, agent
//     scope); a wave whose chunk starts above the recorded nonce leaves.
//     Nothing waits on another wave; only nonces above a recorded hit are
//     ever skipped, so the smallest hit is always hashed and recorded.
#pragma once
#include "bm_header.hpp"
#include "bm_kernels.hpp"

namespace bm {

#ifndef BM_WAVES_HEADER  // waves/SIMD asked for header_kernel (DESIGN.md "Block-header search")
#define BM_WAVES_HEADER 8
#endif

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

// Rounds 4..63 of block 2 for W3 = x (s0x = sigma0(x)); s enters as the
// state before round 4 on the rotating file and leaves as the state after
// round 63 (role r in s[r]).
BM_DEV void header_block2(const HeaderArgs& A, uint32_t x, uint32_t s0x, uint32_t (&s)[8]) {
    uint32_t w[16];
    static_for<4, 16>([&](auto I) { block_round<HeaderBlock2, decltype(I)::value>(s, w); });
    static_for<16, 64>([&](auto I) {
        constexpr int t = decltype(I)::value;
        if constexpr (t == 16) {
            w[0] = A.w16;
            sha_round<t>(s, w[0]);
        } else if constexpr (t == 17) {
            w[1] = A.w17;
            sha_round<t>(s, w[1]);
        } else if constexpr (t == 18) {
            w[2] = A.k18 + s0x;
            sha_round<t>(s, w[2]);
        } else if constexpr (t == 19) {
            w[3] = A.k19 + x;
            sha_round<t>(s, w[3]);
        } else if constexpr (t == 31) {
            w[15] = ssig1(w[13]) + w[8] + A.k31;
            sha_round<t>(s, w[15]);
        } else if constexpr (t == 32) {
            w[0] = ssig1(w[14]) + w[9] + A.k32;
            sha_round<t>(s, w[0]);
        } else {
            block_round<HeaderBlock2, t>(s, w);
        }
    });
}

// 256-bit h <= t, both most significant word first.
BM_DEV bool le256(const uint32_t (&h)[8], const uint32_t (&t)[8]) {
    bool le = true;
#pragma unroll
    for (int i = 7; i >= 0; --i) le = h[i] < t[i] || (h[i] == t[i] && le);
    return le;
}

#ifndef BM_HEADER_KATTR
#define BM_HEADER_KATTR __attribute__((amdgpu_waves_per_eu(BM_WAVES_HEADER, 8)))
#endif

// Work distribution as search_body's: each wave dequeues chunks of
// 64 * chunk_m consecutive tasks from the launch's counter (one returning
// atomic per chunk, lane 0), lane l taking tasks base + l, base + 64 + l, ...
// The body is bm_header_body.inc, shared with header_hits_kernel.
#if defined(BM_HEADER_PIECES_ONLY)
// bm_header_versions_inst.hip: the pieces above, none of the kernels below.
#elif defined(BM_HEADER_HITS_UNIT)
// header_kernel in hits mode (bm_search_header_hits_gpu), the one kernel of
// its build unit (bm_header_hits_inst.hip defines BM_HEADER_HITS_UNIT), so the
// unit of the two kernels below holds what it always held.  Occupancy request
// as for header_kernel.  hit_buf holds hit_cap entries of 16 bytes, 16-byte
// aligned.
__global__ __launch_bounds__(kBlock) BM_HEADER_KATTR void header_hits_kernel(
    const HeaderArgs A, Partial* __restrict__ part, unsigned long long* __restrict__ counter,
    unsigned long long* __restrict__ hit_count, Partial* __restrict__ hit_buf, const uint64_t hit_cap) {
#define BM_HEADER_HITS 1
#include "bm_header_body.inc"
#undef BM_HEADER_HITS
}
#else
__global__ __launch_bounds__(kBlock) BM_HEADER_KATTR void header_kernel(
    const HeaderArgs A, Partial* __restrict__ part, unsigned long long* __restrict__ counter,
    unsigned long long* __restrict__ hit) {
#define BM_HEADER_HITS 0
#include "bm_header_body.inc"
#undef BM_HEADER_HITS
}

// One lane per nonce: the full double hash by the plain compression, from
// the midstate; out gets the 8 digest words of each nonce (big-endian words,
// digest byte order).  Shares nothing with header_kernel's shortcuts, so it
// pins the device's sha256d on its own.
constexpr int kHeaderHashThreads = 64;

__global__ __launch_bounds__(kHeaderHashThreads) void header_hash_kernel(const HeaderHashArgs A,
                                                                   const uint32_t* __restrict__ nonces,
                                                                   uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kHeaderHashThreads + threadIdx.x;
    if (i >= A.n) return;
    uint32_t st[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = A.mid[k];
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = 0;
    w[0] = A.w[0];
    w[1] = A.w[1];
    w[2] = A.w[2];
    w[3] = __builtin_bswap32(nonces[i]);
    w[4] = 0x80000000u;
    w[15] = 640u;
    sha_compress(st, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = st[k];
    w[8] = 0x80000000u;
#pragma unroll
    for (int k = 9; k < 15; ++k) w[k] = 0;
    w[15] = 256u;
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = kIV256[k];
    sha_compress(st, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) out[8ull * i + k] = st[k];
}

#endif  // BM_HEADER_HITS_UNIT

}  // namespace bm
