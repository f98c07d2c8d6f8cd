// header_precompute_check.cpp -- stand-alone CPU check of the block-header
// search's host part (csrc/bm_header.hpp): the plain sha256d against two
// public block headers, then the double hash rebuilt from header_precompute's
// terms (midstate, rounds 0..3, the schedule terms without word 3) against
// the plain one over many nonces, and the compact-target decoding.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//     -I distributed_bitcoin_minter_amd/csrc tools/header_precompute_check.cpp -o header_check && ./header_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "bm_header.hpp"

namespace {

int fails = 0;

void hex_to_bytes(const char* hex, uint8_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        unsigned v = 0;
        std::sscanf(hex + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}

std::string to_hex(const uint8_t* p, size_t n) {
    std::string s;
    char b[3];
    for (size_t i = 0; i < n; ++i) {
        std::snprintf(b, sizeof b, "%02x", p[i]);
        s += b;
    }
    return s;
}

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        ++fails;
    }
}

struct Golden {
    const char* header;
    uint32_t nonce, bits;
    const char* hash;
};

const Golden kGolden[] = {
    {"0100000000000000000000000000000000000000000000000000000000000000000000003ba3edfd7a7b12b27ac72c3e67768f617f"
     "c81bc3888a51323a9fb8aa4b1e5e4a29ab5f49ffff001d1dac2b7c",
     2083236893u, 0x1d00ffffu, "000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f"},
    {"0100000081cd02ab7e569e8bcd9317e2fe99f2de44d49ab2b8851ba4a308000000000000e320b6c2fffc8d750423db8b1eb942ae71"
     "0e951ed797f7affc8892b0f1fc122bc7f5d74df2b9441a42a14695",
     2504433986u, 0x1a44b9f2u, "00000000000000001e8d6829a8a21adc5d38d0a473b144b6765798e61f98bd1d"},
};

}  // namespace

int main() {
    for (const Golden& g : kGolden) {
        uint8_t header[bm::kHeaderBytes];
        hex_to_bytes(g.header, header, sizeof header);
        uint8_t hash[32], target[32];
        bm::host::header_hash_msb(header, g.nonce, hash);
        expect(to_hex(hash, 32) == g.hash, "sha256d of a golden header");
        expect(bm::host::target_from_bits(g.bits, target), "golden bits decode");
        expect(std::memcmp(hash, target, 32) <= 0, "golden hash <= its target");

        // the nonce field of the caller's header is ignored
        uint8_t other[bm::kHeaderBytes];
        std::memcpy(other, header, sizeof other);
        other[76] ^= 0xFF;
        other[79] ^= 0x55;
        uint8_t hash2[32];
        bm::host::header_hash_msb(other, g.nonce, hash2);
        expect(std::memcmp(hash, hash2, 32) == 0, "bytes 76..79 ignored");

        bm::HeaderArgs A;
        std::memset(&A, 0, sizeof A);
        bm::host::header_precompute(header, A);
        uint32_t x = 0x9E3779B9u;
        for (int i = 0; i < 20000; ++i) {
            const uint32_t n = i == 0 ? 0u : i == 1 ? 0xFFFFFFFFu : i == 2 ? g.nonce : x;
            x = x * 1664525u + 1013904223u;
            uint8_t d1[32], d2[32];
            bm::host::sha256d_header(header, n, d1);
            bm::host::sha256d_from_args(A, n, d2);
            if (std::memcmp(d1, d2, 32) != 0) {
                std::printf("FAIL: precomputed terms differ at nonce %u\n", n);
                ++fails;
                break;
            }
        }
    }

    uint8_t t[32];
    expect(bm::host::target_from_bits(0x1d00ffffu, t) &&
               to_hex(t, 32) == "00000000ffff0000000000000000000000000000000000000000000000000000",
           "bits 0x1d00ffff");
    expect(bm::host::target_from_bits(0x1a44b9f2u, t) &&
               to_hex(t, 32) == "00000000000044b9f20000000000000000000000000000000000000000000000",
           "bits 0x1a44b9f2");
    expect(bm::host::target_from_bits(0x02123456u, t) && t[31] == 0x34 && t[30] == 0x12 && t[29] == 0, "exponent 2");
    expect(bm::host::target_from_bits(0x01123456u, t) && t[31] == 0x12 && t[30] == 0, "exponent 1");
    expect(bm::host::target_from_bits(0x00123456u, t) && t[31] == 0 && t[30] == 0, "exponent 0");
    expect(bm::host::target_from_bits(0x207fffffu, t) && t[0] == 0x7f && t[1] == 0xff && t[2] == 0xff && t[3] == 0,
           "exponent 32");
    expect(bm::host::target_from_bits(0x2200007fu, t) && t[0] == 0x7f && t[1] == 0, "exponent 34, one byte");
    expect(!bm::host::target_from_bits(0x1d80ffffu, t), "sign bit");
    expect(!bm::host::target_from_bits(0x21010000u, t), "overflow, three bytes at exponent 33");
    expect(!bm::host::target_from_bits(0x22000100u, t), "overflow, two bytes at exponent 34");
    expect(!bm::host::target_from_bits(0x23000001u, t), "overflow, exponent 35");
    expect(bm::host::target_from_bits(0xff000000u, t), "zero mantissa never overflows");

    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("header precompute check ok\n");
    return 0;
}
