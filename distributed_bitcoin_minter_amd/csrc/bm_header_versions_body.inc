// bm_header_versions_body.inc -- the body of header_versions_kernel<M>
// (bm_header_versions_inst.hip) and of header_versions_hits_kernel<M>
// (bm_header_versions_hits_inst.hip), included inside each with
// BM_VERSIONS_HITS 0 / 1.  The one body of the block-header searches: the
// single-header calls run it at M = 1.
//
// Text rather than a function template: a kernel that hands its by-value
// argument block on to a function gets the whole block copied at entry, and
// its register allocation and code object change with that copy.  Included
// here, header_versions_kernel compiles to what it always did, and the rounds
// themselves (sha_round, block_round) are functions both modes share anyway.
//
// Work distribution as search_body's: each wave dequeues chunks of
// 64 * chunk_m consecutive tasks from the launch's counter (one returning
// atomic per chunk, lane 0), lane l taking tasks base + l, base + 64 + l, ...
//
// In scope: M, A (HeaderVersionsArgs<M>), part, counter, and
//   BM_VERSIONS_HITS 0: hit, the device's hit word;
//   BM_VERSIONS_HITS 1: hit_count, hit_buf, hit_cap, the device's hit counter
//   (zero before the device's first launch of the call) and its buffer of
//   hit_cap 16-byte entries, both shared by the call's group launches.
// Hits mode is a full scan that appends every (nonce, version index) pair of
// the launch's range and slots with H(i, n) <= target:
//  * no early exit: lane 0 loads nothing but the work counter at the dequeue,
//    and no wave leaves before the work counter runs out;
//  * the per-nonce code is header_versions_kernel's: bh is max(best top word,
//    target top word) already, so every hit of every slot takes the rare branch;
//  * there, after the range check and the exact le256, a hit takes the next
//    index with one atomicAdd and, below hit_cap, writes its {top 64 bits of
//    the hash, (n << 32) | version index} with one 16-byte store; the slot is
//    that lane's alone, whichever launch of the call the lane belongs to.  The
//    counter goes on counting past hit_cap, so the count is exact whatever the
//    buffer holds.  The host recomputes every entry's full hash.
#ifndef BM_VERSIONS_HITS
#error "define BM_VERSIONS_HITS to 0 or 1 before including bm_header_versions_body.inc"
#endif
    uint64_t best_h = ~0ull, best_k = ~0ull;
    const uint32_t thi = A.tgt[0];
    uint32_t bh = 0xFFFFFFFFu;  // max(top word of best_h, thi), one for all slots
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t ntask = A.ntask;
    const uint32_t chunk = 64u * A.chunk_m;

    for (;;) {
#if BM_VERSIONS_HITS  // a full scan: no wave reads the hit counter, none leaves early
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
        // the chunk's lowest nonce, in 64 bits (tasks stay below 2^24), against the hit's nonce
        if ((seen >> 32) < ((uint64_t)(A.t0 + (uint32_t)base) << kHeaderTaskBits)) break;
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

                // ---- per slot: the second hash (the digest, one block from the IV) and the compare ----
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
#if !BM_VERSIONS_HITS
                            if (le256(hw, A.tgt)) atomicMin(hit, (unsigned long long)key);
#endif
                            const uint64_t top = ((uint64_t)hw[0] << 32) | hw[1];
#if BM_VERSIONS_HITS
                            if (le256(hw, A.tgt)) {
                                const unsigned long long idx = atomicAdd(hit_count, 1ull);
                                if (idx < hit_cap) {
                                    using u64x2 = unsigned long long __attribute__((ext_vector_type(2)));
                                    *reinterpret_cast<u64x2*>(hit_buf + idx) = u64x2{top, (unsigned long long)key};
                                }
                            }
#endif
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
