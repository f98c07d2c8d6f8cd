// bm_header_versions_inst.hip -- header_versions_kernel<M>, M = 1, 2, 4: the
// kernel of bm_search_header_versions_gpu and its build unit, registered with
// the launcher (bm_search.cpp) at load time.  A unit of its own, built from
// header_kernel's pieces (bm_header_kernels.hpp), so the units of header_kernel
// and header_hits_kernel hold what they always held.
//
// A launch scans one nonce range for M versions of one header ("slots";
// bm_header_versions.hpp).  Per nonce n, with header_kernel's task / inner
// counter split of W3:
//   * rounds 4..63 of block 2 for all M slots in lock-step over ONE schedule
//     window: each word (sched_word<HeaderBlock2, t>, and the four special
//     words 18, 19, 31, 32) is computed once and fed to sha_round<t> of every
//     slot's state.  The schedule costs the same whatever M is;
//   * then, slot by slot, the 61-round second hash and the hot-path compare
//     exactly as bm_header_body.inc has them, against one bh for all slots;
//   * rare path: the exact compare and the range check.  A pair is the key
//     (n << 32) | version index: a hit does one atomicMin of its key on the
//     device's hit word, and the running minimum carries the key in the
//     partial's nonce field, so lex_less, block_min and reduce_partials order
//     pairs as (top 64 bits, n, index).  Indices stay below 64, so no pair's
//     key is all-ones.
//   * early exit: at each dequeue lane 0 reads the hit word; a wave leaves
//     when its chunk's first nonce is above hit >> 32.  Only nonces strictly
//     above a recorded hit's nonce are ever skipped, so every pair at the
//     smallest hitting nonce is hashed, whatever the timing.  The hit word is
//     shared by all of a call's launches on the device and set once, before
//     the first, so a later group scans only up to the best hit so far.
#define BM_HEADER_PIECES_ONLY 1
#include "bm_header_kernels.hpp"
#include "bm_header_versions.hpp"

namespace bm {

// Waves/SIMD asked for per M: the highest request whose per-nonce code holds no
// scratch or memory operation (tools/check_inner.py --header-versions; DESIGN.md
// "Version rolling").
#ifndef BM_WAVES_VERSIONS_1
#define BM_WAVES_VERSIONS_1 8
#endif
#ifndef BM_WAVES_VERSIONS_2
#define BM_WAVES_VERSIONS_2 5
#endif
#ifndef BM_WAVES_VERSIONS_4
#define BM_WAVES_VERSIONS_4 5
#endif
constexpr int versions_waves(int m) {
    return m == 1 ? BM_WAVES_VERSIONS_1 : m == 2 ? BM_WAVES_VERSIONS_2 : BM_WAVES_VERSIONS_4;
}

template <int M>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(versions_waves(M), 8))) void
header_versions_kernel(const HeaderVersionsArgs<M> A, Partial* __restrict__ part,
                       unsigned long long* __restrict__ counter, unsigned long long* __restrict__ hit) {
    uint64_t best_h = ~0ull, best_k = ~0ull;
    const uint32_t thi = A.tgt[0];
    uint32_t bh = 0xFFFFFFFFu;  // max(top word of best_h, thi), one for all slots
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t ntask = A.ntask;
    const uint32_t chunk = 64u * A.chunk_m;

    for (;;) {
        uint64_t base = 0, seen = 0;
        if (lane == 0) {
            base = atomicAdd(counter, (unsigned long long)chunk);
            seen = __hip_atomic_load(hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        base = readfirstlane_u64(base);
        if (base >= ntask) break;
        seen = readfirstlane_u64(seen);
        // the chunk's lowest nonce, in 64 bits (tasks stay below 2^24), against the hit's nonce
        if ((seen >> 32) < ((uint64_t)(A.t0 + (uint32_t)base) << kHeaderTaskBits)) break;
        for (uint32_t i = 0; i < A.chunk_m; ++i) {
            const uint64_t tt = base + 64u * i + lane;
            if (tt >= ntask) break;
            const uint32_t nb = (A.t0 + (uint32_t)tt) << kHeaderTaskBits;  // the task's first nonce
            const uint32_t wl = __builtin_bswap32(nb);                     // its part of W3
            const uint32_t s0wl = ssig0(wl);

            uint32_t J = 0;  // the inner counter's part of W3: j << 24
            for (uint32_t j = 0; j < kHeaderTaskNonces; ++j, J += 1u << 24) {
                const uint32_t x = wl | J;
                const uint32_t s0x = s0wl ^ ssig0_salu(J);

                // ---- first hash: block 2 from round 3 on, M states over one window ----
                uint32_t s[M][8];  // entering round 4: role r in s[m][(r - 4) & 7]
                static_for<0, M>([&](auto MI) {
                    constexpr int m = decltype(MI)::value;
                    s[m][4] = A.slot[m].a3k + x;  // a
                    s[m][5] = A.slot[m].r4[0];    // b
                    s[m][6] = A.slot[m].r4[1];    // c
                    s[m][7] = A.slot[m].r4[2];    // d
                    s[m][0] = A.slot[m].e3k + x;  // e
                    s[m][1] = A.slot[m].r4[3];    // f
                    s[m][2] = A.slot[m].r4[4];    // g
                    s[m][3] = A.slot[m].r4[5];    // h
                });
                uint32_t w[16];
                static_for<4, 64>([&](auto I) {
                    constexpr int t = decltype(I)::value;
                    if constexpr (t < 16) {  // compile-time words: nothing to share
                        static_for<0, M>([&](auto MI) {
                            sha_round<t>(s[decltype(MI)::value], (uint32_t)block_const<HeaderBlock2>(t));
                        });
                    } else {
                        if constexpr (t == 16)
                            w[0] = A.w16;
                        else if constexpr (t == 17)
                            w[1] = A.w17;
                        else if constexpr (t == 18)
                            w[2] = A.k18 + s0x;
                        else if constexpr (t == 19)
                            w[3] = A.k19 + x;
                        else if constexpr (t == 31)
                            w[15] = ssig1(w[13]) + w[8] + A.k31;
                        else if constexpr (t == 32)
                            w[0] = ssig1(w[14]) + w[9] + A.k32;
                        else
                            w[t & 15] = sched_word<HeaderBlock2, t>(w);
                        static_for<0, M>([&](auto MI) { sha_round<t>(s[decltype(MI)::value], w[t & 15]); });
                    }
                });

                // ---- per slot: the second hash and the compare of bm_header_body.inc ----
                static_for<0, M>([&](auto MI) {
                    constexpr int m = decltype(MI)::value;
                    uint32_t d[16];
#pragma unroll
                    for (int q = 0; q < 8; ++q) d[q] = A.slot[m].mid[q] + s[m][q];
                    uint32_t z[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) z[q] = kIV256[q];
                    static_for<0, 61>([&](auto I) { block_round<DigestBlock, decltype(I)::value>(z, d); });
                    // entering round 61, role e (the final h) lives in z[(4 - 61) & 7]
                    const uint32_t h0 = __builtin_bswap32(kIV256[7] + z[(4 - 61) & 7]);

                    if (__builtin_expect(h0 <= bh, 0)) {
                        static_for<61, 64>([&](auto I) { block_round<DigestBlock, decltype(I)::value>(z, d); });
                        uint32_t hw[8];  // the hash, most significant word first
#pragma unroll
                        for (int q = 0; q < 8; ++q) hw[q] = __builtin_bswap32(kIV256[7 - q] + z[7 - q]);
                        const uint32_t n = nb + j;
                        if (n >= A.lo && n <= A.hi) {
                            const uint64_t key = ((uint64_t)n << 32) | A.slot[m].vidx;
                            if (le256(hw, A.tgt)) atomicMin(hit, (unsigned long long)key);
                            const uint64_t top = ((uint64_t)hw[0] << 32) | hw[1];
                            if (lex_less(top, key, best_h, best_k)) {
                                best_h = top;
                                best_k = key;
                                bh = hw[0] > thi ? hw[0] : thi;
                            }
                        }
                    }
                });
            }
        }
    }
    if (block_min<kBlock>(best_h, best_k)) part[A.part_off + blockIdx.x] = Partial{best_h, best_k};
}

template __global__ void header_versions_kernel<1>(const HeaderVersionsArgs<1>, Partial*, unsigned long long*,
                                                   unsigned long long*);
template __global__ void header_versions_kernel<2>(const HeaderVersionsArgs<2>, Partial*, unsigned long long*,
                                                   unsigned long long*);
template __global__ void header_versions_kernel<4>(const HeaderVersionsArgs<4>, Partial*, unsigned long long*,
                                                   unsigned long long*);

}  // namespace bm

extern "C" void bm_register_header_versions_kernel(int m, const void* fn);

namespace {
struct Registrar {
    Registrar() {
        bm_register_header_versions_kernel(1, reinterpret_cast<const void*>(&bm::header_versions_kernel<1>));
        bm_register_header_versions_kernel(2, reinterpret_cast<const void*>(&bm::header_versions_kernel<2>));
        bm_register_header_versions_kernel(4, reinterpret_cast<const void*>(&bm::header_versions_kernel<4>));
    }
};
const Registrar registrar;
}  // namespace
