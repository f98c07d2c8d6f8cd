// sessions_arith.cpp -- test driver for the multiword arithmetic of the session table
// (distributed_bitcoin_minter_amd/csrc/bm_sessions_args.hpp), on the host and without
// HIP: the very header the kernels and the CPU table compile.  It answers one line on
// stdout per line on stdin; every field is hexadecimal, without a prefix.
//
//   mul a b                       -> hi lo                      mul_64x64
//   div hi lo d        (hi < d)   -> quotient remainder         div_128by64
//   tgt d              (d >= 1)   -> q0 q1 q2 q3                target_words_fx
//   var now target window min max burst band up down old since accepted
//                                 -> evaluated new              vardiff_evaluated, vardiff_new
//   args                          -> sizeof(SessionsRetargetArgs) and the offset of each
//                                    of its fields, in the order of declaration
//
// tests/test_sessions_arith.py builds it with the address and undefined-behaviour
// sanitizers and compares every line with Python's big integers.
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "bm_sessions_args.hpp"

int main() {
    char line[1024], op[8];
    while (std::fgets(line, sizeof line, stdin)) {
        uint64_t v[12] = {0};
        int used = 0;
        if (std::sscanf(line, "%7s%n", op, &used) != 1) continue;
        int n = 0;
        for (const char* p = line + used; n < 12; ++n) {
            int step = 0;
            if (std::sscanf(p, "%" SCNx64 "%n", &v[n], &step) != 1) break;
            p += step;
        }
        if (!std::strcmp(op, "mul") && n == 2) {
            const bm::U128 r = bm::mul_64x64(v[0], v[1]);
            std::printf("%" PRIx64 " %" PRIx64 "\n", r.hi, r.lo);
        } else if (!std::strcmp(op, "div") && n == 3 && v[0] < v[2]) {
            uint64_t rem = 0;
            const uint64_t q = bm::div_128by64(v[0], v[1], v[2], &rem);
            std::printf("%" PRIx64 " %" PRIx64 "\n", q, rem);
        } else if (!std::strcmp(op, "tgt") && n == 1 && v[0] >= 1) {
            uint64_t q[4];
            bm::target_words_fx(v[0], q);
            std::printf("%" PRIx64 " %" PRIx64 " %" PRIx64 " %" PRIx64 "\n", q[0], q[1], q[2], q[3]);
        } else if (!std::strcmp(op, "var") && n == 12 && v[8] >= 1 && v[9] >= 1) {  // max_down and old: what the entry checks
            bm::SessionsRetargetArgs A;
            std::memset(&A, 0, sizeof A);
            A.now_ms = v[0], A.target_ms = v[1], A.window_ms = v[2], A.min_fx = v[3], A.max_fx = v[4];
            A.burst = (uint32_t)v[5], A.band_permille = (uint32_t)v[6], A.max_up = (uint32_t)v[7];
            A.max_down = (uint32_t)v[8];
            std::printf("%d %" PRIx64 "\n", bm::vardiff_evaluated(A, v[10], v[11]) ? 1 : 0,
                        bm::vardiff_new(A, v[9], v[10], v[11]));
        } else if (!std::strcmp(op, "args") && n == 0) {
            using S = bm::SessionsRetargetArgs;
            std::printf("%zx %zx %zx %zx %zx %zx %zx %zx %zx %zx %zx %zx %zx %zx\n", sizeof(S), offsetof(S, now_ms),
                        offsetof(S, target_ms), offsetof(S, window_ms), offsetof(S, min_fx), offsetof(S, max_fx),
                        offsetof(S, burst), offsetof(S, band_permille), offsetof(S, max_up), offsetof(S, max_down),
                        offsetof(S, count), offsetof(S, cap), offsetof(S, apply), offsetof(S, pad));
        } else {
            std::printf("error\n");
        }
    }
    return 0;
}
