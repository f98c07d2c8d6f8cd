// bm_header_body.inc -- the body of header_kernel and of header_hits_kernel
// (bm_header_kernels.hpp), included inside each with BM_HEADER_HITS 0 / 1.
//
// Text rather than a function template: a kernel that hands its by-value
// argument block on to a function gets the whole block copied at entry, and
// header_kernel's register allocation and code object change with that copy.
// Included here, header_kernel compiles to what it always did, and the rounds
// themselves (header_block2, block_round) are functions both share anyway.
//
// In scope: A (HeaderArgs), part, counter, and
//   BM_HEADER_HITS 0: hit, the device's hit word;
//   BM_HEADER_HITS 1: hit_count, hit_buf, hit_cap, the device's hit counter
//   (zero before the launch) and its buffer of hit_cap 16-byte entries.
// Hits mode is a full scan that appends every nonce of the launch's range with
// H(n) <= target:
//  * no early exit: no wave reads the counter, none leaves before the work
//    counter runs out;
//  * the per-nonce code is header_kernel's: bh is max(best top word, target
//    top word) already, so every hit takes the rare branch;
//  * there, after the range check and the exact le256, a hit takes the next
//    index with one atomicAdd and, below hit_cap, writes its {top 64 bits of
//    the hash, nonce} with one 16-byte store; the slot is that lane's alone.
//    The counter goes on counting past hit_cap, so the count is exact whatever
//    the buffer holds.  The host recomputes every entry's full hash.
#ifndef BM_HEADER_HITS
#error "define BM_HEADER_HITS to 0 or 1 before including bm_header_body.inc"
#endif
    uint64_t best_h = ~0ull, best_n = ~0ull;
    const uint32_t thi = A.tgt[0];
    uint32_t bh = 0xFFFFFFFFu;  // max(top word of best_h, thi)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t ntask = A.ntask;
    const uint32_t chunk = 64u * A.chunk_m;

    for (;;) {
#if BM_HEADER_HITS  // a full scan: no wave reads the hit counter, none leaves early
        uint64_t base = 0;
        if (lane == 0) base = atomicAdd(counter, (unsigned long long)chunk);
        base = readfirstlane_u64(base);
        if (base >= ntask) break;
#else
        uint64_t base = 0, seen = 0;
        if (lane == 0) {
            base = atomicAdd(counter, (unsigned long long)chunk);
            seen = __hip_atomic_load(hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        base = readfirstlane_u64(base);
        if (base >= ntask) break;
        seen = readfirstlane_u64(seen);
        // the chunk's lowest nonce, in 64 bits (tasks stay below 2^24)
        if (seen < ((uint64_t)(A.t0 + (uint32_t)base) << kHeaderTaskBits)) break;
#endif
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

                // ---- first hash: block 2 from round 3 on ----
                uint32_t s[8];  // entering round 4: role r in s[(r - 4) & 7]
                s[4] = A.a3k + x;  // a
                s[5] = A.r4[0];    // b
                s[6] = A.r4[1];    // c
                s[7] = A.r4[2];    // d
                s[0] = A.e3k + x;  // e
                s[1] = A.r4[3];    // f
                s[2] = A.r4[4];    // g
                s[3] = A.r4[5];    // h
                header_block2(A, x, s0x, s);

                // ---- second hash: the digest, one block from the IV ----
                uint32_t w[16];
#pragma unroll
                for (int q = 0; q < 8; ++q) w[q] = A.mid[q] + s[q];
                uint32_t z[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) z[q] = kIV256[q];
                static_for<0, 61>([&](auto I) { block_round<DigestBlock, decltype(I)::value>(z, w); });
                // entering round 61, role e (the final h) lives in z[(4 - 61) & 7]
                const uint32_t h0 = __builtin_bswap32(kIV256[7] + z[(4 - 61) & 7]);

                if (__builtin_expect(h0 <= bh, 0)) {
                    static_for<61, 64>([&](auto I) { block_round<DigestBlock, decltype(I)::value>(z, w); });
                    uint32_t hw[8];  // the hash, most significant word first
#pragma unroll
                    for (int q = 0; q < 8; ++q) hw[q] = __builtin_bswap32(kIV256[7 - q] + z[7 - q]);
                    const uint32_t n = nb + j;
                    if (n >= A.lo && n <= A.hi) {
#if !BM_HEADER_HITS
                        if (le256(hw, A.tgt)) atomicMin(hit, (unsigned long long)n);
#endif
                        const uint64_t top = ((uint64_t)hw[0] << 32) | hw[1];
#if BM_HEADER_HITS
                        if (le256(hw, A.tgt)) {
                            const unsigned long long idx = atomicAdd(hit_count, 1ull);
                            if (idx < hit_cap) {
                                using u64x2 = unsigned long long __attribute__((ext_vector_type(2)));
                                *reinterpret_cast<u64x2*>(hit_buf + idx) = u64x2{top, (unsigned long long)n};
                            }
                        }
#endif
                        if (lex_less(top, n, best_h, best_n)) {
                            best_h = top;
                            best_n = n;
                            bh = hw[0] > thi ? hw[0] : thi;
                        }
                    }
                }
            }
        }
    }
    if (block_min<kBlock>(best_h, best_n)) part[A.part_off + blockIdx.x] = Partial{best_h, best_n};
