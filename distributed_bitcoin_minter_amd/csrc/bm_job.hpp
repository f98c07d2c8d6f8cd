// bm_job.hpp -- the host's half of bm_search_job_shares_gpu: a Stratum job
// (coinbase halves, extranonce, merkle branch, prevhash, version, nbits) becomes
// one 80-byte header per extranonce2 value, and the per-header answers of the
// version-rolling share enumeration become one list and one best share
// (JobMerge).  And the host's half of share verification (bm_job_verify_cpu,
// bm_job_verify_gpu): one submission's verdict on the CPU, and what
// job_verify_kernel (bm_job_verify.hpp) takes of a job; the same for one job's
// submissions from many sessions (bm_pool_verify_cpu, bm_pool_verify_gpu,
// pool_verify_kernel in bm_pool_verify.hpp), and for the submissions of several
// jobs (bm_jobs_verify_cpu, bm_jobs_verify_gpu, jobs_verify_kernel in
// bm_jobs_verify.hpp: the grouping by job, the descriptors, the tripwire).  Shared
// by the launcher (bm_search.cpp), bm_aux.hip, the pure-CPU entries (bm_job.cpp)
// and four stand-alone CPU checks (tools/job_check.cpp, tools/verify_check.cpp,
// tools/pool_verify_check.cpp, tools/jobs_verify_check.cpp).  Plain C++: no HIP in
// here (en2_words and field_words alone are marked for both sides).
//
//   coinbase = coinb1 || extranonce1 || BE(extranonce2, extranonce2_size) || coinb2
//   root     = sha256d(coinbase); for each branch entry: root = sha256d(root || entry)
//   header   = le32(version) || prevhash || root || le32(ntime) || le32(nbits) || 00000000
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bm_header.hpp"
#include "btcminer.h"

namespace bm {
namespace host {

// SHA-256 of a byte stream fed in pieces, over compress_bytes.
struct Sha256 {
    uint32_t st[8];
    uint8_t blk[64];
    size_t fill = 0;
    uint64_t total = 0;
    Sha256() {
        for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    }
    void update(const uint8_t* p, size_t n) {
        total += n;
        while (n > 0) {
            const size_t take = n < 64 - fill ? n : 64 - fill;
            std::memcpy(blk + fill, p, take);
            fill += take;
            p += take;
            n -= take;
            if (fill == 64) {
                compress_bytes(st, blk);
                fill = 0;
            }
        }
    }
    void finish(uint8_t digest[32]) {
        const uint64_t bits = total * 8;
        blk[fill++] = 0x80;
        if (fill > 56) {  // no room for the length: it goes into a block of its own
            std::memset(blk + fill, 0, 64 - fill);
            compress_bytes(st, blk);
            fill = 0;
        }
        std::memset(blk + fill, 0, 56 - fill);
        for (int i = 0; i < 8; ++i) blk[56 + i] = (uint8_t)(bits >> (8 * (7 - i)));
        compress_bytes(st, blk);
        for (int i = 0; i < 8; ++i) {
            digest[4 * i] = (uint8_t)(st[i] >> 24);
            digest[4 * i + 1] = (uint8_t)(st[i] >> 16);
            digest[4 * i + 2] = (uint8_t)(st[i] >> 8);
            digest[4 * i + 3] = (uint8_t)st[i];
        }
    }
};

// digest = SHA256(SHA256(first)) of what h has been fed.
inline void sha256d_finish(Sha256& h, uint8_t digest[32]) {
    uint8_t first[32];
    h.finish(first);
    Sha256 second;
    second.update(first, sizeof first);
    second.finish(digest);
}

inline void store_le32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

// extranonce2 fits its field: below 2^(8 * size), size in 1..8.
inline bool extranonce2_fits(uint64_t extranonce2, uint32_t size) {
    return size >= 8 || (extranonce2 >> (8 * size)) == 0;
}

// Everything bm_job_header refuses that does not depend on extranonce2.
inline int job_check(const bm_job_t* job) {
    if (!job) return BM_EINVAL;
    if ((!job->coinb1 && job->coinb1_len) || (!job->extranonce1 && job->extranonce1_len) ||
        (!job->coinb2 && job->coinb2_len) || (!job->branch && job->nbranch))
        return BM_EINVAL;
    if (job->extranonce2_size < 1 || job->extranonce2_size > 8) return BM_EINVAL;
    if (job->nbranch > BM_MAX_JOB_BRANCH) return BM_EINVAL;
    // each length against the limit first, so the sum cannot wrap
    const size_t lim = BM_MAX_JOB_COINBASE;
    if (job->coinb1_len > lim || job->extranonce1_len > lim || job->coinb2_len > lim) return BM_EINVAL;
    if (job->coinb1_len + job->extranonce1_len + job->extranonce2_size + job->coinb2_len > lim) return BM_EINVAL;
    return BM_OK;
}

// The header of a checked job (job_check, extranonce2_fits) with a zero nonce field.
inline void job_header(const bm_job_t* job, uint64_t extranonce2, uint32_t ntime, uint32_t version,
                       uint8_t header[kHeaderBytes]) {
    uint8_t en2[8];
    const uint32_t size = job->extranonce2_size;
    for (uint32_t i = 0; i < size; ++i) en2[i] = (uint8_t)(extranonce2 >> (8 * (size - 1 - i)));
    uint8_t root[32];
    Sha256 h;
    if (job->coinb1_len) h.update(job->coinb1, job->coinb1_len);
    if (job->extranonce1_len) h.update(job->extranonce1, job->extranonce1_len);
    h.update(en2, size);
    if (job->coinb2_len) h.update(job->coinb2, job->coinb2_len);
    sha256d_finish(h, root);
    for (size_t b = 0; b < job->nbranch; ++b) {
        Sha256 node;
        node.update(root, sizeof root);
        node.update(job->branch + 32 * b, 32);
        sha256d_finish(node, root);
    }
    store_le32(header, version);
    std::memcpy(header + 4, job->prevhash, 32);
    std::memcpy(header + 36, root, 32);
    store_le32(header + 68, ntime);
    store_le32(header + 72, job->nbits);
    store_le32(header + 76, 0);
}

}  // namespace host

// ---- share verification (bm_job_verify_cpu / bm_job_verify_gpu) ----
// The coinbase of every submission of a job differs in extranonce2's bytes only,
// and those have a fixed size and position.  So the host hashes the whole 64-byte
// blocks that end before extranonce2's first byte once (mid), and lays the rest
// out as a padded tail of big-endian words with extranonce2's bytes zero; a lane
// ORs its extranonce2 into the up to three consecutive words it can touch (8
// bytes at byte 1..3 of a word span three words, and may span a block edge).

// Kernel argument of job_verify_kernel, by value (SGPRs).
struct JobVerifyArgs {
    uint32_t mid[8];    // state after the whole blocks before extranonce2's block
    uint32_t prev[8];   // prevhash as big-endian words (header words 1..8)
    uint32_t tgt[8];    // the share target, most significant word first
    uint32_t btgt[8];   // the target of nbits, likewise (has_block)
    uint32_t nbits;
    uint32_t has_block; // 1: nbits decodes
    uint32_t nb;        // 64-byte blocks of the tail (1..1025)
    uint32_t j0;        // first tail word extranonce2 touches (0..15)
    uint32_t boff;      // extranonce2's byte offset in that word (0..3)
    uint32_t size;      // extranonce2_size (1..8)
    uint32_t depth;     // branch entries (0..32)
    uint32_t n;         // submissions
};

// A verdict as the kernel stores it: ten 32-bit words in bm_job_verdict_t's layout.
constexpr int kVerdictWords = 10;
static_assert(sizeof(bm_job_verdict_t) == 4 * kVerdictWords, "verdict layout");
static_assert(sizeof(bm_job_submit_t) == 24, "submit layout");

// extranonce2 (size bytes, big-endian) at byte boff of a 12-byte window, as the
// window's three big-endian words.
BM_HD inline void en2_words(uint64_t extranonce2, uint32_t size, uint32_t boff, uint32_t& e0, uint32_t& e1,
                            uint32_t& e2) {
    const uint64_t v = extranonce2 << (8 * (8 - size));  // its first byte on top
    e0 = (uint32_t)(v >> (32 + 8 * boff));
    e1 = (uint32_t)(v >> (8 * boff));
    e2 = boff ? (uint32_t)(v << (32 - 8 * boff)) : 0u;
}

namespace host {

// What job_verify_kernel takes of a checked job (job_check): A but for n, the
// tail's words (16 * A.nb) and the branch's (8 * A.depth), both big-endian.
inline void verify_prepare(const bm_job_t* job, const uint8_t target[32], JobVerifyArgs& A,
                           std::vector<uint32_t>& tail, std::vector<uint32_t>& branch) {
    std::memset(&A, 0, sizeof A);
    const size_t pos = job->coinb1_len + job->extranonce1_len;  // extranonce2's first byte
    const size_t size = job->extranonce2_size;
    const size_t total = pos + size + job->coinb2_len;
    const size_t pre = pos / 64;                                // whole blocks before its block
    const size_t padded = (total + 9 + 63) / 64 * 64;
    std::vector<uint8_t> bytes(padded, 0);
    if (job->coinb1_len) std::memcpy(bytes.data(), job->coinb1, job->coinb1_len);
    if (job->extranonce1_len) std::memcpy(bytes.data() + job->coinb1_len, job->extranonce1, job->extranonce1_len);
    if (job->coinb2_len) std::memcpy(bytes.data() + pos + size, job->coinb2, job->coinb2_len);
    bytes[total] = 0x80;
    const uint64_t bits = (uint64_t)total * 8;
    for (int i = 0; i < 8; ++i) bytes[padded - 8 + i] = (uint8_t)(bits >> (8 * (7 - i)));
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    for (size_t b = 0; b < pre; ++b) compress_bytes(st, bytes.data() + 64 * b);
    for (int i = 0; i < 8; ++i) A.mid[i] = st[i];
    A.nb = (uint32_t)(padded / 64 - pre);
    const size_t off = pos - 64 * pre;
    A.j0 = (uint32_t)(off / 4);
    A.boff = (uint32_t)(off % 4);
    A.size = (uint32_t)size;
    A.depth = (uint32_t)job->nbranch;
    tail.resize(16 * (size_t)A.nb);
    for (size_t k = 0; k < tail.size(); ++k) tail[k] = load_be32(bytes.data() + 64 * pre + 4 * k);
    branch.resize(8 * job->nbranch);
    for (size_t k = 0; k < branch.size(); ++k) branch[k] = load_be32(job->branch + 4 * k);
    for (int k = 0; k < 8; ++k) {
        A.prev[k] = load_be32(job->prevhash + 4 * k);
        A.tgt[k] = load_be32(target + 4 * k);
    }
    A.nbits = job->nbits;
    uint8_t bt[32];
    A.has_block = target_from_bits(job->nbits, bt) ? 1u : 0u;
    if (A.has_block)
        for (int k = 0; k < 8; ++k) A.btgt[k] = load_be32(bt + 4 * k);
}

// The verdict of one submission of a checked job.  block_target: the target of
// the job's nbits, or nullptr when nbits does not decode.
inline void verify_one(const bm_job_t* job, const uint8_t target[32], const uint8_t* block_target,
                       const bm_job_submit_t& s, bm_job_verdict_t& v) {
    std::memset(&v, 0, sizeof v);
    if (!extranonce2_fits(s.extranonce2, job->extranonce2_size)) {
        std::memset(v.hash, 0xFF, sizeof v.hash);
        v.status = BM_SUBMIT_INVALID;
        return;
    }
    uint8_t header[kHeaderBytes];
    job_header(job, s.extranonce2, s.ntime, s.version, header);
    header_hash_msb(header, s.nonce, v.hash);
    if (std::memcmp(v.hash, target, 32) <= 0) v.status |= BM_SUBMIT_SHARE;
    if (block_target && std::memcmp(v.hash, block_target, 32) <= 0) v.status |= BM_SUBMIT_BLOCK;
}

// *out of a call from its verdicts.
inline void verify_count(const bm_job_verdict_t* verdicts, size_t n, bm_job_verify_result_t& out) {
    std::memset(&out, 0, sizeof out);
    out.n = n;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t st = verdicts[i].status;
        out.shares += (st & BM_SUBMIT_SHARE) ? 1 : 0;
        out.blocks += (st & BM_SUBMIT_BLOCK) ? 1 : 0;
        out.invalid += (st & BM_SUBMIT_INVALID) ? 1 : 0;
    }
}

// The arguments both entries refuse, ctx aside.
inline int verify_check(const bm_job_t* job, const uint8_t* target, const bm_job_submit_t* submits, size_t n,
                        const bm_job_verdict_t* verdicts, const bm_job_verify_result_t* out) {
    if (!job || !target || !out || n > BM_MAX_JOB_SUBMITS || (n && (!submits || !verdicts))) return BM_EINVAL;
    return job_check(job);
}

// The per-header answers of one bm_search_job_shares_gpu call, in ascending
// extranonce2 order, become its answer.  All or nothing over the whole call:
// room() is the cap the next header's enumeration gets, what is left of the
// call's cap while the running count fits in it and 0 (a pure count) from then
// on; the list is kept here and reaches the caller's array in finish() only, so
// a failure part-way leaves that array untouched.
class JobMerge {
public:
    // block_target: the target of the job's nbits (most significant byte first),
    // or nullptr when nbits does not decode (is_block stays 0)
    JobMerge(size_t cap, const uint8_t* block_target, uint32_t ntime, uint64_t en2_lo, uint32_t version0)
        : cap_(cap), ntime_(ntime), has_block_(block_target != nullptr) {
        if (has_block_) std::memcpy(block_, block_target, sizeof block_);
        std::memset(&out_, 0, sizeof out_);
        std::memset(out_.hash, 0xFF, sizeof out_.hash);  // the empty answer
        out_.extranonce2 = en2_lo;
        out_.nonce = 0xFFFFFFFFu;
        out_.version = version0;
    }

    size_t room() const { return out_.count <= cap_ ? cap_ - (size_t)out_.count : 0; }

    // One header's answer: r and hits[0 .. r.stored) as header_versions_hits_impl
    // left them for a call with cap room().  BM_EINTERNAL unless stored is what
    // all-or-nothing allows and the entries ascend by (nonce, index).
    int add(uint64_t extranonce2, const bm_header_version_hit_t* hits, const bm_header_versions_hits_result_t& r) {
        const size_t room_now = room();
        if (r.stored != (r.count <= room_now ? r.count : 0)) return BM_EINTERNAL;
        if (r.stored && !hits) return BM_EINTERNAL;
        if (out_.headers > 0 && extranonce2 <= last_en2_) return BM_EINTERNAL;
        for (size_t i = 1; i < r.stored; ++i)
            if (pair_key(hits[i - 1]) >= pair_key(hits[i])) return BM_EINTERNAL;
        out_.count += r.count;
        if (out_.count > cap_) {
            std::vector<bm_job_share_t>().swap(list_);  // over the cap for good: only counts from here
        } else {
            for (size_t i = 0; i < r.stored; ++i) {
                bm_job_share_t s;
                std::memcpy(s.hash, hits[i].hash, sizeof s.hash);
                s.extranonce2 = extranonce2;
                s.nonce = hits[i].nonce;
                s.ntime = ntime_;
                s.version_index = hits[i].version_index;
                s.version = hits[i].version;
                s.is_block = has_block_ && std::memcmp(s.hash, block_, 32) <= 0 ? 1 : 0;
                s.reserved = 0;
                list_.push_back(s);
            }
        }
        // the best share minimises (hash >> 192, extranonce2, nonce, index): headers
        // come in ascending extranonce2 order, so a later one wins on a smaller hash only
        if (out_.headers == 0 || hash_top64(r.hash) < hash_top64(out_.hash)) {
            std::memcpy(out_.hash, r.hash, sizeof out_.hash);
            out_.extranonce2 = extranonce2;
            out_.nonce = r.nonce;
            out_.version_index = r.version_index;
            out_.version = r.version;
        }
        last_en2_ = extranonce2;
        ++out_.headers;
        return BM_OK;
    }

    // The call's answer: shares[0 .. stored) (never more than the cap) and *out.
    void finish(bm_job_share_t* shares, bm_job_shares_result_t* out) {
        out_.stored = out_.count <= cap_ ? list_.size() : 0;
        if (out_.stored) std::memcpy(shares, list_.data(), list_.size() * sizeof(bm_job_share_t));
        *out = out_;
    }

private:
    static uint64_t pair_key(const bm_header_version_hit_t& h) { return ((uint64_t)h.nonce << 32) | h.version_index; }

    size_t cap_;
    uint32_t ntime_;
    bool has_block_;
    uint8_t block_[32];
    uint64_t last_en2_ = 0;
    std::vector<bm_job_share_t> list_;
    bm_job_shares_result_t out_;
};

}  // namespace host

// ---- share verification across sessions (bm_pool_verify_cpu / bm_pool_verify_gpu) ----
// One job, many sessions: extranonce1 and the share target are per-submission
// data, looked up in a session table.  The varying field of the coinbase is now
//   extranonce1 || BE(extranonce2, extranonce2_size),
// 2..16 bytes that start at byte coinb1_len.  The host hashes the whole blocks
// that end before coinb1_len once (mid) and lays the rest out as a padded tail
// with BOTH fields zero; a lane ORs its field into the up to five consecutive
// words it can touch (16 bytes at byte 3 of a word are 19 bytes), which may
// cross a block edge.

// Kernel argument of pool_verify_kernel, by value (SGPRs).
struct PoolVerifyArgs {
    uint32_t mid[8];    // state after the whole blocks before the field's block
    uint32_t prev[8];   // prevhash as big-endian words (header words 1..8)
    uint32_t btgt[8];   // the target of nbits, most significant word first (has_block)
    uint32_t nbits;
    uint32_t has_block; // 1: nbits decodes
    uint32_t nb;        // 64-byte blocks of the tail (1..1025)
    uint32_t j0;        // first tail word the field touches (0..15)
    uint32_t boff;      // the field's byte offset in that word (0..3)
    uint32_t size1;     // extranonce1_len (1..8)
    uint32_t size2;     // extranonce2_size (1..8)
    uint32_t depth;     // branch entries (0..32)
    uint32_t n;         // submissions
    uint32_t nsessions; // entries of the session table a lane may pick (the table on the device has at least one)
    uint32_t ntime_lo, ntime_hi;
};

static_assert(sizeof(bm_pool_session_t) == 40, "session layout");
static_assert(sizeof(bm_pool_submit_t) == 24, "pool submit layout");
constexpr int kSessionWords = 10;  // a session as the kernel loads it: 2 words of extranonce1, 8 of the target
constexpr int kFieldWords = 5;

// The field extranonce1 (its first size1 bytes: en1 holds the session's eight
// bytes as a big-endian integer, byte 0 on top) || extranonce2 (size2 bytes,
// big-endian) at byte boff of a 20-byte window, as the window's five big-endian
// words.
BM_HD inline void field_words(uint64_t en1, uint32_t size1, uint64_t extranonce2, uint32_t size2, uint32_t boff,
                              uint32_t (&e)[kFieldWords]) {
    const uint64_t v1 = en1 & (~0ull << (8 * (8 - size1)));   // the bytes that count, the first on top
    const uint64_t v2 = extranonce2 << (8 * (8 - size2));      // likewise
    // the field as 16 bytes, its first byte on top of hi
    const uint64_t hi = v1 | (size1 < 8 ? v2 >> (8 * size1) : 0ull);
    const uint64_t lo = v2 << (8 * (8 - size1));
    // each window word is 32 bits of the 64-bit pair around it, boff bytes down
    const uint64_t mid = (hi << 32) | (lo >> 32);
    const uint32_t s = 8 * boff;
    e[0] = (uint32_t)((hi >> 32) >> s);
    e[1] = (uint32_t)(hi >> s);
    e[2] = (uint32_t)(mid >> s);
    e[3] = (uint32_t)(lo >> s);
    e[4] = (uint32_t)((lo << 32) >> s);
}

namespace host {

// A session's extranonce1 bytes as field_words takes them.
inline uint64_t session_en1(const bm_pool_session_t& s) {
    return ((uint64_t)load_be32(s.extranonce1) << 32) | load_be32(s.extranonce1 + 4);
}

// What both pool entries refuse, ctx aside.  job->extranonce1 is not looked at.
inline int pool_verify_check(const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                             const bm_pool_submit_t* submits, size_t n, const bm_job_verdict_t* verdicts,
                             const bm_pool_verify_result_t* out) {
    if (!job || !out || n > BM_MAX_JOB_SUBMITS || nsessions > BM_MAX_POOL_SESSIONS) return BM_EINVAL;
    if ((n && (!submits || !verdicts)) || (nsessions && !sessions)) return BM_EINVAL;
    if (job->extranonce1_len < 1 || job->extranonce1_len > 8) return BM_EINVAL;
    bm_job_t j = *job;
    j.extranonce1 = j.prevhash;  // any non-NULL pointer: job_check reads no byte of it
    return job_check(&j);
}

// What pool_verify_kernel takes of a checked job (pool_verify_check): A but for
// n, nsessions and the window, the tail's words (16 * A.nb) and the branch's
// (8 * A.depth), both big-endian.
inline void pool_verify_prepare(const bm_job_t* job, PoolVerifyArgs& A, std::vector<uint32_t>& tail,
                                std::vector<uint32_t>& branch) {
    std::memset(&A, 0, sizeof A);
    const size_t pos = job->coinb1_len;  // the field's first byte
    const size_t size = job->extranonce1_len + job->extranonce2_size;
    const size_t total = pos + size + job->coinb2_len;
    const size_t pre = pos / 64;         // whole blocks before its block
    const size_t padded = (total + 9 + 63) / 64 * 64;
    std::vector<uint8_t> bytes(padded, 0);
    if (job->coinb1_len) std::memcpy(bytes.data(), job->coinb1, job->coinb1_len);
    if (job->coinb2_len) std::memcpy(bytes.data() + pos + size, job->coinb2, job->coinb2_len);
    bytes[total] = 0x80;
    const uint64_t bits = (uint64_t)total * 8;
    for (int i = 0; i < 8; ++i) bytes[padded - 8 + i] = (uint8_t)(bits >> (8 * (7 - i)));
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    for (size_t b = 0; b < pre; ++b) compress_bytes(st, bytes.data() + 64 * b);
    for (int i = 0; i < 8; ++i) A.mid[i] = st[i];
    A.nb = (uint32_t)(padded / 64 - pre);
    const size_t off = pos - 64 * pre;
    A.j0 = (uint32_t)(off / 4);
    A.boff = (uint32_t)(off % 4);
    A.size1 = (uint32_t)job->extranonce1_len;
    A.size2 = job->extranonce2_size;
    A.depth = (uint32_t)job->nbranch;
    tail.resize(16 * (size_t)A.nb);
    for (size_t k = 0; k < tail.size(); ++k) tail[k] = load_be32(bytes.data() + 64 * pre + 4 * k);
    branch.resize(8 * job->nbranch);
    for (size_t k = 0; k < branch.size(); ++k) branch[k] = load_be32(job->branch + 4 * k);
    for (int k = 0; k < 8; ++k) A.prev[k] = load_be32(job->prevhash + 4 * k);
    A.nbits = job->nbits;
    uint8_t bt[32];
    A.has_block = target_from_bits(job->nbits, bt) ? 1u : 0u;
    if (A.has_block)
        for (int k = 0; k < 8; ++k) A.btgt[k] = load_be32(bt + 4 * k);
}

// The verdict of one submission of a checked job: the CPU path.  block_target as
// in verify_one.
inline void pool_verify_one(const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                            const uint8_t* block_target, uint32_t ntime_lo, uint32_t ntime_hi,
                            const bm_pool_submit_t& s, bm_job_verdict_t& v) {
    std::memset(&v, 0, sizeof v);
    if (s.session >= nsessions || !extranonce2_fits(s.extranonce2, job->extranonce2_size)) {
        std::memset(v.hash, 0xFF, sizeof v.hash);
        v.status = BM_SUBMIT_INVALID;
        return;
    }
    const bm_pool_session_t& ses = sessions[s.session];
    bm_job_t j = *job;
    j.extranonce1 = ses.extranonce1;
    uint8_t header[kHeaderBytes];
    job_header(&j, s.extranonce2, s.ntime, s.version, header);
    header_hash_msb(header, s.nonce, v.hash);
    if (std::memcmp(v.hash, ses.target, 32) <= 0) v.status |= BM_SUBMIT_SHARE;
    if (block_target && std::memcmp(v.hash, block_target, 32) <= 0) v.status |= BM_SUBMIT_BLOCK;
    if (s.ntime < ntime_lo || s.ntime > ntime_hi) v.status |= BM_SUBMIT_NTIME;
}

// *out of a pool call from its verdicts.
inline void pool_verify_count(const bm_job_verdict_t* verdicts, size_t n, bm_pool_verify_result_t& out) {
    std::memset(&out, 0, sizeof out);
    out.n = n;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t st = verdicts[i].status;
        out.shares += (st & BM_SUBMIT_SHARE) ? 1 : 0;
        out.blocks += (st & BM_SUBMIT_BLOCK) ? 1 : 0;
        out.invalid += (st & BM_SUBMIT_INVALID) ? 1 : 0;
        out.ntime += (st & BM_SUBMIT_NTIME) ? 1 : 0;
    }
}

}  // namespace host

// ---- share verification over several jobs (bm_jobs_verify_cpu / bm_jobs_verify_gpu) ----
// Several live jobs, one session table: the job is per-submission data too.  What
// pool_verify_kernel takes by value, jobs_verify_kernel (bm_jobs_verify.hpp) reads
// from a descriptor table, and the host groups the batch by job so that a 64-lane
// workgroup holds one job's submissions only: every loop stays wave-uniform.

// One job as jobs_verify_kernel reads it, through scalar loads: PoolVerifyArgs'
// per-job fields, the window, and where the job's tail and branch start in the
// words array (all tails, then all branches), in 32-bit words.
struct JobsVerifyDesc {
    uint32_t mid[8];
    uint32_t prev[8];
    uint32_t btgt[8];
    uint32_t nbits;
    uint32_t has_block;
    uint32_t nb;
    uint32_t j0;
    uint32_t boff;
    uint32_t size1;
    uint32_t size2;
    uint32_t depth;
    uint32_t ntime_lo, ntime_hi;
    uint32_t tail_off;    // first word of the tail (16 * nb words)
    uint32_t branch_off;  // first word of the branch (8 * depth words)
    uint32_t reserved[4]; // 160 bytes: a whole number of 8-byte units, and of 32-byte scalar loads
};
static_assert(sizeof(JobsVerifyDesc) == 160, "descriptor layout");

// One 64-lane workgroup of jobs_verify_kernel: count (1..64) staged records from
// `first` on, all of job `job`, or of no job (kJobsNone: job >= njobs).
struct JobsVerifyBlock {
    uint32_t job;
    uint32_t first;
    uint32_t count;
    uint32_t reserved;
};
static_assert(sizeof(JobsVerifyBlock) == 16, "block table layout");
static_assert(sizeof(bm_jobs_submit_t) == 32, "jobs submit layout");
constexpr uint32_t kJobsNone = 0xFFFFFFFFu;
constexpr uint32_t kJobsVerifyThreads = 64;

namespace host {

// What the three entries over several jobs refuse, ctx and set aside: every job is
// checked, named by a submission or not.
inline int jobs_verify_check(const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions,
                             size_t nsessions, const bm_jobs_submit_t* submits, size_t n,
                             const bm_job_verdict_t* verdicts, const void* out) {
    if (!out || n > BM_MAX_JOB_SUBMITS || nsessions > BM_MAX_POOL_SESSIONS || njobs > BM_MAX_POOL_JOBS) return BM_EINVAL;
    if ((n && (!submits || !verdicts)) || (nsessions && !sessions) || (njobs && !jobs)) return BM_EINVAL;
    static const bm_pool_verify_result_t some = {};  // pool_verify_check only asks that there is one
    for (size_t j = 0; j < njobs; ++j) {
        // the arrays are checked above; a job is checked as for an empty batch
        const int rc = pool_verify_check(&jobs[j].job, sessions, nsessions, nullptr, 0, nullptr, &some);
        if (rc != BM_OK) return rc;
    }
    return BM_OK;
}

// The verdict of one submission over checked jobs (jobs_verify_check): the CPU path.
inline void jobs_verify_one(const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions,
                            size_t nsessions, const bm_jobs_submit_t& s, bm_job_verdict_t& v) {
    if (s.job >= njobs) {
        std::memset(&v, 0, sizeof v);
        std::memset(v.hash, 0xFF, sizeof v.hash);
        v.status = BM_SUBMIT_INVALID;
        return;
    }
    const bm_pool_job_t& pj = jobs[s.job];
    uint8_t bt[32];
    const uint8_t* block_target = target_from_bits(pj.job.nbits, bt) ? bt : nullptr;
    bm_pool_submit_t ps;
    ps.extranonce2 = s.extranonce2;
    ps.ntime = s.ntime;
    ps.nonce = s.nonce;
    ps.version = s.version;
    ps.session = s.session;
    pool_verify_one(&pj.job, sessions, nsessions, block_target, pj.ntime_lo, pj.ntime_hi, ps, v);
}

// The batch grouped by job: group g < njobs holds job g's submissions, group njobs
// those of no job (job >= njobs), each in the caller's order.
struct JobsPlan {
    std::vector<uint32_t> start;            // njobs + 2 entries: group g is staged[start[g] .. start[g + 1])
    std::vector<JobsVerifyBlock> blocks;    // sum over the groups of ceil(size / 64) entries
};

// The counts, by one read of every submission's job field: the groups' offsets and
// the block table, which no entry of ever spans two groups.
inline void jobs_plan(const bm_jobs_submit_t* submits, size_t n, size_t njobs, JobsPlan& P) {
    P.start.assign(njobs + 2, 0);
    for (size_t i = 0; i < n; ++i) {
        const size_t g = submits[i].job < njobs ? submits[i].job : njobs;
        ++P.start[g + 1];
    }
    for (size_t g = 0; g <= njobs; ++g) P.start[g + 1] += P.start[g];
    P.blocks.clear();
    for (size_t g = 0; g <= njobs; ++g)
        for (uint32_t first = P.start[g]; first < P.start[g + 1]; first += kJobsVerifyThreads) {
            const uint32_t left = P.start[g + 1] - first;
            JobsVerifyBlock b;
            b.job = g < njobs ? (uint32_t)g : kJobsNone;
            b.first = first;
            b.count = left < kJobsVerifyThreads ? left : kJobsVerifyThreads;
            b.reserved = 0;
            P.blocks.push_back(b);
        }
}

// The stable scatter of the counting sort, which is the copy into the stage:
// staged[k] is a submission with its original index in `job` (the job is the block
// table's) and `reserved` zero.  staged has room for n records.
inline void jobs_stage(const bm_jobs_submit_t* submits, size_t n, size_t njobs, const JobsPlan& P,
                       bm_jobs_submit_t* staged) {
    uint32_t cursor[BM_MAX_POOL_JOBS + 1];
    for (size_t g = 0; g <= njobs; ++g) cursor[g] = P.start[g];
    for (size_t i = 0; i < n; ++i) {
        const size_t g = submits[i].job < njobs ? submits[i].job : njobs;
        bm_jobs_submit_t& r = staged[cursor[g]++];
        r = submits[i];
        r.job = (uint32_t)i;
        r.reserved = 0;
    }
}

// What jobs_verify_kernel takes of checked jobs: a descriptor per job and the words
// array, all tails and then all branches, big-endian.
inline void jobs_verify_prepare(const bm_pool_job_t* jobs, size_t njobs, std::vector<JobsVerifyDesc>& desc,
                                std::vector<uint32_t>& words) {
    desc.assign(njobs, JobsVerifyDesc());
    words.clear();
    std::vector<std::vector<uint32_t>> branches(njobs);
    std::vector<uint32_t> tail;
    for (size_t j = 0; j < njobs; ++j) {
        PoolVerifyArgs A;
        pool_verify_prepare(&jobs[j].job, A, tail, branches[j]);
        JobsVerifyDesc& D = desc[j];
        std::memset(&D, 0, sizeof D);
        std::memcpy(D.mid, A.mid, sizeof D.mid);
        std::memcpy(D.prev, A.prev, sizeof D.prev);
        std::memcpy(D.btgt, A.btgt, sizeof D.btgt);
        D.nbits = A.nbits, D.has_block = A.has_block, D.nb = A.nb, D.j0 = A.j0, D.boff = A.boff;
        D.size1 = A.size1, D.size2 = A.size2, D.depth = A.depth;
        D.ntime_lo = jobs[j].ntime_lo, D.ntime_hi = jobs[j].ntime_hi;
        D.tail_off = (uint32_t)words.size();
        words.insert(words.end(), tail.begin(), tail.end());
    }
    for (size_t j = 0; j < njobs; ++j) {
        desc[j].branch_off = (uint32_t)words.size();
        words.insert(words.end(), branches[j].begin(), branches[j].end());
    }
}

// The entries the device's answer is checked at by the CPU path: the ends of the
// batch, every claimed block and the lowest-index submission of each job that has
// one (the first staged record of its group: a descriptor or an offset taken from
// another job shows there).  The status bits of `ignore` are not the verifier's.
inline int jobs_verify_tripwire(const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions,
                                size_t nsessions, const bm_jobs_submit_t* submits, size_t n, const JobsPlan& P,
                                const bm_jobs_submit_t* staged, const bm_job_verdict_t* got, uint32_t ignore) {
    auto same = [&](size_t i) {
        bm_job_verdict_t want, have = got[i];
        have.status &= ~ignore;
        jobs_verify_one(jobs, njobs, sessions, nsessions, submits[i], want);
        return std::memcmp(&want, &have, sizeof want) == 0;
    };
    for (size_t i = 0; i < n; ++i) {
        if (i != 0 && i != n - 1 && !(got[i].status & BM_SUBMIT_BLOCK)) continue;
        if (!same(i)) return BM_EINTERNAL;
    }
    for (size_t g = 0; g < njobs; ++g) {
        if (P.start[g] == P.start[g + 1]) continue;
        const size_t i = staged[P.start[g]].job;
        if (i >= n || !same(i)) return BM_EINTERNAL;
    }
    return BM_OK;
}

}  // namespace host
}  // namespace bm
