// bm_header.hpp -- Bitcoin block-header search: what the host works out once
// per call, shared by the launcher (bm_search.cpp), the kernels
// (bm_header_versions_body.inc) and a stand-alone CPU check (tools/header_precompute_check.cpp).
// Plain C++: no HIP in here.
//
// H(n) = SHA256(SHA256(header[0:76] || le32(n))), read as a little-endian
// 256-bit integer.  The 80 bytes are two SHA-256 blocks:
//   block 1 = header[0:64]                          -> the midstate, once per call
//   block 2 = header[64:76], le32(n), 0x80, 0.., 640 -> words 0..2 constant, word 3 =
//             bswap32(n), words 4..15 compile-time constants
// and the 32-byte digest is hashed again as one block from the IV (words
// 8..15 = 0x80000000, 0.., 256).
//
// Per call, on the host (header_precompute):
//   * the midstate of block 1;
//   * rounds 0..2 of block 2 (their words are constant), and round 3 up to its
//     one per-nonce term: a3 = a3k + W3, e3 = e3k + W3;
//   * every schedule term of block 2 that does not involve word 3:
//       W16, W17 whole; W18 = k18 + sigma0(W3); W19 = k19 + W3;
//       W31 = sigma1(W29) + W24 + k31;  W32 = sigma1(W30) + W25 + k32.
#pragma once
#include <cstdint>
#include <cstring>

#include "bm_sha256.hpp"

namespace bm {

constexpr int kHeaderBytes = 80;
constexpr int kHeaderTaskBits = 8;  // a task = 2^8 consecutive nonces of one lane (the nonce's low byte,
                                    // W3's top byte, is the wave-uniform inner counter)
constexpr uint32_t kHeaderTaskNonces = 1u << kHeaderTaskBits;

// What header_precompute works out of one header: the per-header terms of the
// kernels' argument block (HeaderVersionsArgs, bm_header_versions.hpp, holds
// them per version slot and the schedule terms once).
struct HeaderArgs {
    uint32_t mid[8];   // state after block 1
    uint32_t a3k, e3k; // round 3 of block 2: a = a3k + W3, e = e3k + W3
    uint32_t r4[6];    // roles b, c, d, f, g, h entering round 4
    uint32_t w16, w17; // schedule words 16 and 17 of block 2
    uint32_t k18, k19; // W18 = k18 + sigma0(W3), W19 = k19 + W3
    uint32_t k31, k32; // W31 = sigma1(W29) + W24 + k31, W32 = sigma1(W30) + W25 + k32
};

// Kernel argument of header_hash_kernel.
struct HeaderHashArgs {
    uint32_t mid[8];  // state after block 1
    uint32_t w[3];    // words 0..2 of block 2
    uint32_t n;       // nonces to hash
};

namespace host {

inline uint32_t sig0(uint32_t x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
inline uint32_t sig1(uint32_t x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }
inline uint32_t bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}

// One round on (a..h) = st[0..7], in place.
inline void round(uint32_t st[8], uint32_t kw) {
    const uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kw;
    const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    st[7] = g; st[6] = f; st[5] = e; st[4] = d + t1; st[3] = c; st[2] = b; st[1] = a; st[0] = t1 + t2;
}

// Everything of HeaderArgs that depends on the header alone.
inline void header_precompute(const uint8_t header[kHeaderBytes], HeaderArgs& A) {
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    compress_bytes(st, header);
    for (int i = 0; i < 8; ++i) A.mid[i] = st[i];
    const uint32_t w0 = load_be32(header + 64), w1 = load_be32(header + 68), w2 = load_be32(header + 72);
    round(st, kK256[0] + w0);
    round(st, kK256[1] + w1);
    round(st, kK256[2] + w2);
    {  // round 3 without its W3
        const uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kK256[3];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        A.a3k = t1 + t2;
        A.e3k = d + t1;
        A.r4[0] = a;  // b
        A.r4[1] = b;  // c
        A.r4[2] = c;  // d
        A.r4[3] = e;  // f
        A.r4[4] = f;  // g
        A.r4[5] = g;  // h
    }
    // block 2: W4 = 0x80000000, W5..W14 = 0, W15 = 640
    A.w16 = sig0(w1) + w0;              // sigma1(W14) = 0, W9 = 0
    A.w17 = sig1(640u) + sig0(w2) + w1; // W10 = 0
    A.k18 = sig1(A.w16) + w2;           // W11 = 0
    A.k19 = sig1(A.w17) + sig0(0x80000000u);  // W12 = 0
    A.k31 = sig0(A.w16) + 640u;
    A.k32 = sig0(A.w17) + A.w16;
}

// SHA256(SHA256(header[0:76] || le32(nonce))): the 32 digest bytes.
inline void sha256d_header(const uint8_t header[kHeaderBytes], uint32_t nonce, uint8_t digest[32]) {
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    compress_bytes(st, header);
    uint8_t blk[64];
    std::memset(blk, 0, sizeof blk);
    std::memcpy(blk, header + 64, 12);
    blk[12] = (uint8_t)nonce;
    blk[13] = (uint8_t)(nonce >> 8);
    blk[14] = (uint8_t)(nonce >> 16);
    blk[15] = (uint8_t)(nonce >> 24);
    blk[16] = 0x80;
    blk[62] = 0x02;  // 640 bits
    blk[63] = 0x80;
    compress_bytes(st, blk);
    uint32_t w[16] = {};
    for (int i = 0; i < 8; ++i) w[i] = st[i];
    w[8] = 0x80000000u;
    w[15] = 256u;
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    compress(st, w);
    for (int i = 0; i < 8; ++i) {
        digest[4 * i] = (uint8_t)(st[i] >> 24);
        digest[4 * i + 1] = (uint8_t)(st[i] >> 16);
        digest[4 * i + 2] = (uint8_t)(st[i] >> 8);
        digest[4 * i + 3] = (uint8_t)st[i];
    }
}

// H(n) as the ABI writes it: most significant byte first (the digest reversed).
inline void header_hash_msb(const uint8_t header[kHeaderBytes], uint32_t nonce, uint8_t hash[32]) {
    uint8_t d[32];
    sha256d_header(header, nonce, d);
    for (int i = 0; i < 32; ++i) hash[i] = d[31 - i];
}

// The top 64 bits of a hash in that order: what a device's partial or hit entry carries of it.
inline uint64_t hash_top64(const uint8_t hash[32]) {
    return ((uint64_t)load_be32(hash) << 32) | load_be32(hash + 4);
}

// The same double hash the way the kernel computes it, from a HeaderArgs:
// rounds 3..63 of block 2 on the precomputed terms, then the second hash.
// Only for checking header_precompute on the CPU.
inline void sha256d_from_args(const HeaderArgs& A, uint32_t nonce, uint8_t digest[32]) {
    const uint32_t x = bswap32(nonce);
    uint32_t W[64] = {};
    W[3] = x;
    W[4] = 0x80000000u;
    W[15] = 640u;
    W[16] = A.w16;
    W[17] = A.w17;
    W[18] = A.k18 + sig0(x);
    W[19] = A.k19 + x;
    for (int t = 20; t < 64; ++t) {
        if (t == 31)
            W[t] = sig1(W[29]) + W[24] + A.k31;
        else if (t == 32)
            W[t] = sig1(W[30]) + W[25] + A.k32;
        else
            W[t] = sig1(W[t - 2]) + W[t - 7] + sig0(W[t - 15]) + W[t - 16];
    }
    uint32_t st[8] = {A.a3k + x, A.r4[0], A.r4[1], A.r4[2], A.e3k + x, A.r4[3], A.r4[4], A.r4[5]};
    for (int t = 4; t < 64; ++t) round(st, kK256[t] + W[t]);
    uint32_t w[16] = {};
    for (int i = 0; i < 8; ++i) w[i] = A.mid[i] + st[i];
    w[8] = 0x80000000u;
    w[15] = 256u;
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    compress(st, w);
    for (int i = 0; i < 8; ++i) {
        digest[4 * i] = (uint8_t)(st[i] >> 24);
        digest[4 * i + 1] = (uint8_t)(st[i] >> 16);
        digest[4 * i + 2] = (uint8_t)(st[i] >> 8);
        digest[4 * i + 3] = (uint8_t)st[i];
    }
}

// Bitcoin's compact target: mantissa = nbits & 0x7fffff, exponent = nbits >> 24,
// target = mantissa << 8 * (exponent - 3) (a right shift below 3), written most
// significant byte first.  false: the sign bit 0x00800000 is set, or the value
// does not fit 256 bits.
inline bool target_from_bits(uint32_t nbits, uint8_t target[32]) {
    const uint32_t mant = nbits & 0x7fffffu;
    const int exp = (int)(nbits >> 24);
    if (nbits & 0x00800000u) return false;
    if (mant != 0 && (exp > 34 || (mant > 0xffu && exp > 33) || (mant > 0xffffu && exp > 32))) return false;
    std::memset(target, 0, 32);
    if (mant == 0) return true;
    if (exp < 3) {
        const uint32_t v = mant >> (8 * (3 - exp));
        target[29] = (uint8_t)(v >> 16);
        target[30] = (uint8_t)(v >> 8);
        target[31] = (uint8_t)v;
        return true;
    }
    // byte k (0 = least significant) of the value is mantissa byte k - (exp - 3)
    for (int k = 0; k < 3; ++k) {
        const int pos = k + exp - 3;
        if (pos < 32) target[31 - pos] = (uint8_t)(mant >> (8 * k));
    }
    return true;
}

}  // namespace host
}  // namespace bm
