// btcminer.hpp -- C++17 host side above the C ABI (btcminer.h).
//
// The reference is Go (compiled code) and its toolchain is absent here, so
// the host side of the path is C++ (the Python package mirrors it for tests
// and the system programs).  Two parts:
//
//   btcminer::Context   RAII owner of a bm_ctx (one process over N GPUs, or
//                       one rank of an RCCL group); errors are exceptions.
//   btcminer::Job       a Stratum job that owns its buffers (bm_job_t).
//   bitcoin::           the reference's `bitcoin` package for this path:
//                       Hash (hash.go:11-15), MsgType / Message / NewRequest /
//                       NewResult / NewJoin / String (message.go:5-60), with
//                       Message::Marshal producing the bytes Go's
//                       encoding/json produces for the Go struct, and
//                       Message::Unmarshal accepting what the Python mirror
//                       (distributed_bitcoin_minter_amd/bitcoin.py) accepts.
//
// Header-only; link with -lbtcminer.
#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "bm_json.hpp"
#include "btcminer.h"

namespace btcminer {

class Error : public std::runtime_error {
   public:
    Error(int status, const std::string& what)
        : std::runtime_error(what + ": " + bm_strerror(status) + " (" + std::to_string(status) + ")"),
          status_(status) {}
    int status() const { return status_; }

   private:
    int status_;
};

inline void check(int status, const char* what) {
    if (status != BM_OK) throw Error(status, what);
}

struct Result {
    uint64_t hash = UINT64_MAX;
    uint64_t nonce = UINT64_MAX;
};

// A Stratum job that owns its buffers (bm_job_t borrows them): the coinbase
// halves, the miner's extranonce1, the size of extranonce2, the merkle branch
// (32 bytes per entry, as sent), prevhash in header byte order, and version,
// nbits and ntime as integers.
class Job {
   public:
    std::vector<uint8_t> coinb1, extranonce1, coinb2, branch;
    uint32_t extranonce2_size = 4;
    uint8_t prevhash[32] = {};
    uint32_t version = 0, nbits = 0, ntime = 0;

    // prevhash as mining.notify sends it: each 4-byte word reversed
    void set_prevhash_from_stratum(const uint8_t in[32]) {
        check(bm_job_prevhash_from_stratum(in, prevhash), "bm_job_prevhash_from_stratum");
    }
    // the C view of this job: valid while the job lives and its buffers do not change
    bm_job_t view() const {
        bm_job_t j;
        std::memset(&j, 0, sizeof j);
        j.coinb1 = coinb1.data();
        j.coinb1_len = coinb1.size();
        j.extranonce1 = extranonce1.data();
        j.extranonce1_len = extranonce1.size();
        j.extranonce2_size = extranonce2_size;
        j.coinb2 = coinb2.data();
        j.coinb2_len = coinb2.size();
        j.branch = branch.data();
        j.nbranch = branch.size() / 32;
        std::memcpy(j.prevhash, prevhash, sizeof j.prevhash);
        j.version = version;
        j.nbits = nbits;
        return j;
    }
    // the 80-byte header under extranonce2, with a zero nonce field: bm_job_header
    void header(uint64_t extranonce2, uint32_t ntime_, uint32_t version_, uint8_t out[80]) const {
        if (branch.size() % 32 != 0) throw Error(BM_EINVAL, "Job::header");
        const bm_job_t j = view();
        check(bm_job_header(&j, extranonce2, ntime_, version_, out), "bm_job_header");
    }
    void header(uint64_t extranonce2, uint8_t out[80]) const { header(extranonce2, ntime, version, out); }
};

// floor(diff1 / difficulty) as 32 bytes, most significant first: bm_target_from_difficulty
inline void target_from_difficulty(double difficulty, uint8_t target[32]) {
    check(bm_target_from_difficulty(difficulty, target), "bm_target_from_difficulty");
}

// Context::verify_job_submits without a GPU or a context: bm_job_verify_cpu, the
// specification of the GPU entry (byte-identical verdicts and counts)
inline bm_job_verify_result_t verify_job_submits_cpu(const Job& job, const uint8_t target[32],
                                                     const bm_job_submit_t* submits, size_t n,
                                                     std::vector<bm_job_verdict_t>& verdicts) {
    if (job.branch.size() % 32 != 0) throw Error(BM_EINVAL, "verify_job_submits_cpu");
    const bm_job_t j = job.view();
    bm_job_verify_result_t r;
    std::vector<bm_job_verdict_t> buf(n);
    check(bm_job_verify_cpu(&j, target, submits, n, n ? buf.data() : nullptr, &r), "bm_job_verify_cpu");
    verdicts = std::move(buf);
    return r;
}

// Context::verify_pool_submits without a GPU or a context: bm_pool_verify_cpu, the
// specification of the GPU entry.  job.extranonce1 gives the size of every
// session's extranonce1 (1..8 bytes); its bytes are not used
inline bm_pool_verify_result_t verify_pool_submits_cpu(const Job& job, const std::vector<bm_pool_session_t>& sessions,
                                                       const bm_pool_submit_t* submits, size_t n,
                                                       std::vector<bm_job_verdict_t>& verdicts, uint32_t ntime_lo = 0,
                                                       uint32_t ntime_hi = 0xFFFFFFFFu) {
    if (job.branch.size() % 32 != 0) throw Error(BM_EINVAL, "verify_pool_submits_cpu");
    const bm_job_t j = job.view();
    bm_pool_verify_result_t r;
    std::vector<bm_job_verdict_t> buf(n);
    check(bm_pool_verify_cpu(&j, sessions.empty() ? nullptr : sessions.data(), sessions.size(), submits, n, ntime_lo,
                             ntime_hi, n ? buf.data() : nullptr, &r),
          "bm_pool_verify_cpu");
    verdicts = std::move(buf);
    return r;
}

// One live job of a pool and its own ntime window, inclusive (bm_pool_job_t)
struct PoolJob {
    const Job* job = nullptr;  // borrowed: lives, unchanged, through the call
    uint32_t ntime_lo = 0, ntime_hi = 0xFFFFFFFFu;
};

// The C view of a job table: valid while the jobs live and their buffers do not change
inline std::vector<bm_pool_job_t> pool_job_views(const std::vector<PoolJob>& jobs, const char* what) {
    std::vector<bm_pool_job_t> v(jobs.size());
    for (size_t i = 0; i < jobs.size(); ++i) {
        if (!jobs[i].job || jobs[i].job->branch.size() % 32 != 0) throw Error(BM_EINVAL, what);
        v[i].job = jobs[i].job->view();
        v[i].ntime_lo = jobs[i].ntime_lo;
        v[i].ntime_hi = jobs[i].ntime_hi;
    }
    return v;
}

// Context::verify_jobs without a GPU or a context: bm_jobs_verify_cpu, the
// specification of the GPU entry
inline bm_pool_verify_result_t verify_jobs_cpu(const std::vector<PoolJob>& jobs,
                                               const std::vector<bm_pool_session_t>& sessions,
                                               const bm_jobs_submit_t* submits, size_t n,
                                               std::vector<bm_job_verdict_t>& verdicts) {
    const std::vector<bm_pool_job_t> j = pool_job_views(jobs, "verify_jobs_cpu");
    bm_pool_verify_result_t r;
    std::vector<bm_job_verdict_t> buf(n);
    check(bm_jobs_verify_cpu(j.empty() ? nullptr : j.data(), j.size(), sessions.empty() ? nullptr : sessions.data(),
                             sessions.size(), submits, n, n ? buf.data() : nullptr, &r),
          "bm_jobs_verify_cpu");
    verdicts = std::move(buf);
    return r;
}

// Owns a bm_ctx.  Not thread-safe, like the C context (one per OS thread).
class Context {
   public:
    // num_gpus = 0: every visible GPU
    explicit Context(int num_gpus = 1) { check(bm_ctx_create(num_gpus, &ctx_), "bm_ctx_create"); }
    explicit Context(const std::vector<int>& devices) {
        check(bm_ctx_create_devices(devices.data(), (int)devices.size(), &ctx_), "bm_ctx_create_devices");
    }
    // rank `rank` of an RCCL group of `world` processes (blocks until all join)
    static Context rank(int device, int rank, int world, const uint8_t (&id)[BM_RCCL_ID_BYTES]) {
        Context c{Empty{}};
        check(bm_ctx_create_rank(device, rank, world, id, &c.ctx_), "bm_ctx_create_rank");
        return c;
    }
    // rank `rank` of `world` outside a group: search() returns this rank's
    // partial; join() then makes it a member of the RCCL group
    static Context rank_local(int device, int rank, int world) {
        Context c{Empty{}};
        check(bm_ctx_create_rank_local(device, rank, world, &c.ctx_), "bm_ctx_create_rank_local");
        return c;
    }
    void join(const uint8_t (&id)[BM_RCCL_ID_BYTES], int timeout_ms = 0) {
        check(bm_ctx_join_rank(ctx_, id, timeout_ms), "bm_ctx_join_rank");
    }
    void leave() { check(bm_ctx_leave_rank(ctx_), "bm_ctx_leave_rank"); }
    // a joined rank's wait for its peers, at most (default BM_DEFAULT_PEER_TIMEOUT_MS; 0: no limit)
    void set_peer_timeout(int timeout_ms) {
        check(bm_ctx_set_peer_timeout(ctx_, timeout_ms), "bm_ctx_set_peer_timeout");
    }
    // per-launch HIP event timing, and what the last search reported (bm_stats_t)
    void set_timing(bool on) { check(bm_ctx_set_timing(ctx_, on ? 1 : 0), "bm_ctx_set_timing"); }
    bm_stats_t last_stats() const {
        bm_stats_t s;
        check(bm_ctx_last_stats(ctx_, &s), "bm_ctx_last_stats");
        return s;
    }
    Context(Context&& o) noexcept : ctx_(std::exchange(o.ctx_, nullptr)) {}
    Context& operator=(Context&& o) noexcept {
        if (this != &o) {
            reset();
            ctx_ = std::exchange(o.ctx_, nullptr);
        }
        return *this;
    }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ~Context() { reset(); }

    // min over n in [lower, upper] of (Hash(msg, n), n): miner.go:58-65
    Result search(std::string_view msg, uint64_t lower, uint64_t upper) {
        bm_result_t r;
        check(bm_search_gpu(ctx_, reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), lower, upper, &r),
              "bm_search_gpu");
        return Result{r.hash, r.nonce};
    }
    // the first n in [lower, upper] with Hash(msg, n) <= target (found = 1), or
    // the range's minimum when there is none (found = 0): bm_search_target_gpu
    bm_target_result_t search_target(std::string_view msg, uint64_t lower, uint64_t upper, uint64_t target) {
        bm_target_result_t r;
        check(bm_search_target_gpu(ctx_, reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), lower, upper,
                                   target, &r),
              "bm_search_target_gpu");
        return r;
    }
    // every n in [lower, upper] with Hash(msg, n) <= target, ascending, into
    // `hits` (resized to the result's `stored`: empty when count > cap), plus
    // the exact count and the range's minimum: bm_search_hits_gpu
    bm_hits_result_t search_hits(std::string_view msg, uint64_t lower, uint64_t upper, uint64_t target,
                                 std::vector<bm_result_t>& hits, size_t cap) {
        bm_hits_result_t r;
        std::vector<bm_result_t> buf(cap);
        check(bm_search_hits_gpu(ctx_, reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), lower, upper, target,
                                 cap ? buf.data() : nullptr, cap, &r),
              "bm_search_hits_gpu");
        buf.resize(static_cast<size_t>(r.stored));
        hits = std::move(buf);
        return r;
    }
    bm_target_stats_t last_target_stats() const {
        bm_target_stats_t s;
        check(bm_ctx_last_target_stats(ctx_, &s), "bm_ctx_last_target_stats");
        return s;
    }
    // Bitcoin block header: the first nonce of [nonce_lo, nonce_hi] whose double
    // SHA-256 is <= target (found = 1), or the range's best share (found = 0).
    // header is 80 bytes, target 32 bytes most significant first: bm_search_header_gpu
    bm_header_result_t search_header(const uint8_t header[80], uint32_t nonce_lo, uint32_t nonce_hi,
                                     const uint8_t target[32]) {
        bm_header_result_t r;
        check(bm_search_header_gpu(ctx_, header, nonce_lo, nonce_hi, target, &r), "bm_search_header_gpu");
        return r;
    }
    // the same header under each of `versions` (1..BM_MAX_HEADER_VERSIONS version
    // fields, bytes 0..3): the smallest nonce at which any version's hash is
    // <= target, then the smallest index (found = 1), or the best share over
    // all pairs (found = 0): bm_search_header_versions_gpu
    bm_header_versions_result_t search_header_versions(const uint8_t header[80], const std::vector<uint32_t>& versions,
                                                       uint32_t nonce_lo, uint32_t nonce_hi,
                                                       const uint8_t target[32]) {
        bm_header_versions_result_t r;
        check(bm_search_header_versions_gpu(ctx_, header, versions.data(), versions.size(), nonce_lo, nonce_hi, target,
                                            &r),
              "bm_search_header_versions_gpu");
        return r;
    }
    // every n in [nonce_lo, nonce_hi] whose double SHA-256 is <= target,
    // ascending, into `hits` (resized to the result's `stored`: empty when
    // count > cap), plus the exact count and the range's best share:
    // bm_search_header_hits_gpu
    bm_header_hits_result_t search_header_hits(const uint8_t header[80], uint32_t nonce_lo, uint32_t nonce_hi,
                                               const uint8_t target[32], std::vector<bm_header_hit_t>& hits,
                                               size_t cap) {
        bm_header_hits_result_t r;
        std::vector<bm_header_hit_t> buf(cap);
        check(bm_search_header_hits_gpu(ctx_, header, nonce_lo, nonce_hi, target, cap ? buf.data() : nullptr, cap, &r),
              "bm_search_header_hits_gpu");
        buf.resize(static_cast<size_t>(r.stored));
        hits = std::move(buf);
        return r;
    }
    // every (n, i), n in [nonce_lo, nonce_hi], whose double SHA-256 under
    // versions[i] is <= target, ascending by (n, i), into `hits` (resized to the
    // result's `stored`: empty when count > cap), plus the exact count and the
    // best share over all pairs: bm_search_header_versions_hits_gpu
    bm_header_versions_hits_result_t search_header_versions_hits(const uint8_t header[80],
                                                                 const std::vector<uint32_t>& versions,
                                                                 uint32_t nonce_lo, uint32_t nonce_hi,
                                                                 const uint8_t target[32],
                                                                 std::vector<bm_header_version_hit_t>& hits,
                                                                 size_t cap) {
        bm_header_versions_hits_result_t r;
        std::vector<bm_header_version_hit_t> buf(cap);
        check(bm_search_header_versions_hits_gpu(ctx_, header, versions.data(), versions.size(), nonce_lo, nonce_hi,
                                                 target, cap ? buf.data() : nullptr, cap, &r),
              "bm_search_header_versions_hits_gpu");
        buf.resize(static_cast<size_t>(r.stored));
        hits = std::move(buf);
        return r;
    }
    // a Stratum job under every extranonce2 of [en2_lo, en2_hi] and each of
    // `versions`, at the job's ntime: every share with hash <= target, ascending
    // by (extranonce2, nonce, index), into `shares` (resized to the result's
    // `stored`: empty when count > cap, over the whole call), plus the exact
    // count and the best share: bm_search_job_shares_gpu
    bm_job_shares_result_t search_job_shares(const Job& job, uint64_t en2_lo, uint64_t en2_hi,
                                             const std::vector<uint32_t>& versions, uint32_t nonce_lo,
                                             uint32_t nonce_hi, const uint8_t target[32],
                                             std::vector<bm_job_share_t>& shares, size_t cap) {
        if (job.branch.size() % 32 != 0) throw Error(BM_EINVAL, "search_job_shares");
        const bm_job_t j = job.view();
        bm_job_shares_result_t r;
        std::vector<bm_job_share_t> buf(cap);
        check(bm_search_job_shares_gpu(ctx_, &j, job.ntime, en2_lo, en2_hi, versions.data(), versions.size(), nonce_lo,
                                       nonce_hi, target, cap ? buf.data() : nullptr, cap, &r),
              "bm_search_job_shares_gpu");
        buf.resize(static_cast<size_t>(r.stored));
        shares = std::move(buf);
        return r;
    }
    // a batch of mining.submit tuples of a job against a share target: one verdict
    // per submission, in the caller's order, into `verdicts` (resized to n), plus
    // the count of each flag, on the first device: bm_job_verify_gpu
    bm_job_verify_result_t verify_job_submits(const Job& job, const uint8_t target[32],
                                              const bm_job_submit_t* submits, size_t n,
                                              std::vector<bm_job_verdict_t>& verdicts) {
        if (job.branch.size() % 32 != 0) throw Error(BM_EINVAL, "verify_job_submits");
        const bm_job_t j = job.view();
        bm_job_verify_result_t r;
        std::vector<bm_job_verdict_t> buf(n);
        check(bm_job_verify_gpu(ctx_, &j, target, submits, n, n ? buf.data() : nullptr, &r), "bm_job_verify_gpu");
        verdicts = std::move(buf);
        return r;
    }
    // one job's submissions from many sessions (an extranonce1 and a share target
    // each, picked by submits[i].session), with an ntime window: one verdict per
    // submission into `verdicts` (resized to n) and the count of each flag, on the
    // first device: bm_pool_verify_gpu
    bm_pool_verify_result_t verify_pool_submits(const Job& job, const std::vector<bm_pool_session_t>& sessions,
                                                const bm_pool_submit_t* submits, size_t n,
                                                std::vector<bm_job_verdict_t>& verdicts, uint32_t ntime_lo = 0,
                                                uint32_t ntime_hi = 0xFFFFFFFFu) {
        if (job.branch.size() % 32 != 0) throw Error(BM_EINVAL, "verify_pool_submits");
        const bm_job_t j = job.view();
        bm_pool_verify_result_t r;
        std::vector<bm_job_verdict_t> buf(n);
        check(bm_pool_verify_gpu(ctx_, &j, sessions.empty() ? nullptr : sessions.data(), sessions.size(), submits, n,
                                 ntime_lo, ntime_hi, n ? buf.data() : nullptr, &r),
              "bm_pool_verify_gpu");
        verdicts = std::move(buf);
        return r;
    }
    // the submissions of several live jobs (submits[i].job picks the job and its
    // window; all jobs share the session table) in one call, verdicts in the
    // caller's order, on the first device: bm_jobs_verify_gpu
    bm_pool_verify_result_t verify_jobs(const std::vector<PoolJob>& jobs, const std::vector<bm_pool_session_t>& sessions,
                                        const bm_jobs_submit_t* submits, size_t n,
                                        std::vector<bm_job_verdict_t>& verdicts) {
        const std::vector<bm_pool_job_t> j = pool_job_views(jobs, "verify_jobs");
        bm_pool_verify_result_t r;
        std::vector<bm_job_verdict_t> buf(n);
        check(bm_jobs_verify_gpu(ctx_, j.empty() ? nullptr : j.data(), j.size(),
                                 sessions.empty() ? nullptr : sessions.data(), sessions.size(), submits, n,
                                 n ? buf.data() : nullptr, &r),
              "bm_jobs_verify_gpu");
        verdicts = std::move(buf);
        return r;
    }
    // the double SHA-256 of the header under each nonce, 32 bytes each, most
    // significant byte first, on the first device: bm_header_hash_gpu
    std::vector<uint8_t> header_hash(const uint8_t header[80], const std::vector<uint32_t>& nonces) {
        std::vector<uint8_t> out(32 * nonces.size());
        check(bm_header_hash_gpu(ctx_, header, nonces.data(), nonces.size(), out.data()), "bm_header_hash_gpu");
        return out;
    }
    // bitcoin.Hash for each nonce (hash.go:11-15), on the first device
    std::vector<uint64_t> hash(std::string_view msg, const std::vector<uint64_t>& nonces) {
        std::vector<uint64_t> out(nonces.size());
        check(bm_hash_gpu(ctx_, reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), nonces.data(),
                          nonces.size(), out.data()),
              "bm_hash_gpu");
        return out;
    }
    int num_devices() const {
        int n = 0;
        check(bm_ctx_num_devices(ctx_, &n), "bm_ctx_num_devices");
        return n;
    }
    // the range partitioner: shares per slot (empty: near-equal), or shares
    // that follow each device's measured rate (multi-device contexts)
    void set_split(const std::vector<uint32_t>& shares) {
        check(bm_ctx_set_split(ctx_, shares.data(), (int)shares.size()), "bm_ctx_set_split");
    }
    void set_balance(bool on) { check(bm_ctx_set_balance(ctx_, on ? 1 : 0), "bm_ctx_set_balance"); }
    bm_ctx_t* get() const { return ctx_; }

   private:
    struct Empty {};
    explicit Context(Empty) {}
    void reset() {
        if (ctx_) bm_ctx_destroy(ctx_);
        ctx_ = nullptr;
    }
    bm_ctx_t* ctx_ = nullptr;
};

// A bm_share_set_t: the set of header hashes behind duplicate-share detection,
// cleared by the caller when its jobs retire.  ShareSet(ctx, capacity) lives on the first device of ctx,
// across calls, and is destroyed before ctx; ShareSet::cpu(capacity) lives in host
// memory and needs no GPU: the specification.  Move-only.
class ShareSet {
   public:
    ShareSet(Context& ctx, size_t capacity) { check(bm_share_set_create(ctx.get(), capacity, &set_), "bm_share_set_create"); }
    static ShareSet cpu(size_t capacity) {
        ShareSet s;
        check(bm_share_set_create_cpu(capacity, &s.set_), "bm_share_set_create_cpu");
        return s;
    }
    ShareSet(const ShareSet&) = delete;
    ShareSet& operator=(const ShareSet&) = delete;
    ShareSet(ShareSet&& o) noexcept : set_(o.set_) { o.set_ = nullptr; }
    ShareSet& operator=(ShareSet&& o) noexcept {
        if (this != &o) {
            bm_share_set_destroy(set_);
            set_ = o.set_;
            o.set_ = nullptr;
        }
        return *this;
    }
    ~ShareSet() { bm_share_set_destroy(set_); }

    // Context::verify_pool_submits plus the set: an eligible submission (SHARE or
    // BLOCK, not INVALID) whose hash the set holds carries BM_SUBMIT_DUPLICATE, any
    // other eligible one is recorded.  All or nothing: Error with status BM_EFULL
    // when the batch's new hashes do not fit, `verdicts` and the set as before.
    bm_share_set_result_t verify(const Job& job, const std::vector<bm_pool_session_t>& sessions,
                                 const bm_pool_submit_t* submits, size_t n, std::vector<bm_job_verdict_t>& verdicts,
                                 uint32_t ntime_lo = 0, uint32_t ntime_hi = 0xFFFFFFFFu) {
        if (job.branch.size() % 32 != 0) throw Error(BM_EINVAL, "ShareSet::verify");
        const bm_job_t j = job.view();
        bm_share_set_result_t r;
        std::vector<bm_job_verdict_t> buf(n);
        check(bm_share_set_verify(set_, &j, sessions.empty() ? nullptr : sessions.data(), sessions.size(), submits, n,
                                  ntime_lo, ntime_hi, n ? buf.data() : nullptr, &r),
              "bm_share_set_verify");
        verdicts = std::move(buf);
        return r;
    }
    // Context::verify_jobs plus the set, as verify: bm_share_set_verify_jobs
    bm_share_set_result_t verify_jobs(const std::vector<PoolJob>& jobs, const std::vector<bm_pool_session_t>& sessions,
                                      const bm_jobs_submit_t* submits, size_t n,
                                      std::vector<bm_job_verdict_t>& verdicts) {
        const std::vector<bm_pool_job_t> j = pool_job_views(jobs, "ShareSet::verify_jobs");
        bm_share_set_result_t r;
        std::vector<bm_job_verdict_t> buf(n);
        check(bm_share_set_verify_jobs(set_, j.empty() ? nullptr : j.data(), j.size(),
                                       sessions.empty() ? nullptr : sessions.data(), sessions.size(), submits, n,
                                       n ? buf.data() : nullptr, &r),
              "bm_share_set_verify_jobs");
        verdicts = std::move(buf);
        return r;
    }
    void clear() { check(bm_share_set_clear(set_), "bm_share_set_clear"); }  // the set's jobs have retired
    uint64_t count() const {
        uint64_t n = 0;
        check(bm_share_set_count(set_, &n, nullptr), "bm_share_set_count");
        return n;
    }
    uint64_t capacity() const {
        uint64_t n = 0;
        check(bm_share_set_count(set_, nullptr, &n), "bm_share_set_count");
        return n;
    }
    bm_share_set_t* get() const { return set_; }

   private:
    ShareSet() = default;
    bm_share_set_t* set_ = nullptr;
};

// Owns a bm_ledger_t: the per-account tallies behind share accounting, fed by
// verify_jobs and read or drained at payout or retarget time.  On the first device
// of a context (destroy it before the context), or Ledger::cpu(rows) in host memory
// with no GPU: the specification.  Not thread-safe; a device ledger shares its
// context's buffers, so one call at a time per context.
class Ledger {
   public:
    Ledger(Context& ctx, size_t rows) { check(bm_ledger_create(ctx.get(), rows, &ledger_), "bm_ledger_create"); }
    static Ledger cpu(size_t rows) {
        Ledger l;
        check(bm_ledger_create_cpu(rows, &l.ledger_), "bm_ledger_create_cpu");
        return l;
    }
    Ledger(const Ledger&) = delete;
    Ledger& operator=(const Ledger&) = delete;
    Ledger(Ledger&& o) noexcept : ledger_(o.ledger_) { o.ledger_ = nullptr; }
    Ledger& operator=(Ledger&& o) noexcept {
        if (this != &o) {
            bm_ledger_destroy(ledger_);
            ledger_ = o.ledger_;
            o.ledger_ = nullptr;
        }
        return *this;
    }
    ~Ledger() { bm_ledger_destroy(ledger_); }

    // ShareSet::verify_jobs (set == nullptr: Context::verify_jobs) plus the credit of
    // every submission to the row of its session's account: bm_ledger_verify_jobs.
    // accounts and weights have one entry per session, or are nullptr (session s ->
    // row s; 1 each).  All or nothing, as ShareSet::verify_jobs.
    bm_ledger_result_t verify_jobs(ShareSet* set, const std::vector<PoolJob>& jobs,
                                   const std::vector<bm_pool_session_t>& sessions, const uint32_t* accounts,
                                   const uint64_t* weights, const bm_jobs_submit_t* submits, size_t n,
                                   std::vector<bm_job_verdict_t>& verdicts) {
        const std::vector<bm_pool_job_t> j = pool_job_views(jobs, "Ledger::verify_jobs");
        bm_ledger_result_t r;
        std::vector<bm_job_verdict_t> buf(n);
        check(bm_ledger_verify_jobs(ledger_, set ? set->get() : nullptr, j.empty() ? nullptr : j.data(), j.size(),
                                    sessions.empty() ? nullptr : sessions.data(), sessions.size(), accounts, weights,
                                    submits, n, n ? buf.data() : nullptr, &r),
              "bm_ledger_verify_jobs");
        verdicts = std::move(buf);
        return r;
    }
    std::vector<bm_ledger_row_t> read(size_t first, size_t count) {
        std::vector<bm_ledger_row_t> out(count);
        check(bm_ledger_read(ledger_, first, count, count ? out.data() : nullptr), "bm_ledger_read");
        return out;
    }
    // read, then exactly those rows are empty again
    std::vector<bm_ledger_row_t> drain(size_t first, size_t count) {
        std::vector<bm_ledger_row_t> out(count);
        check(bm_ledger_drain(ledger_, first, count, count ? out.data() : nullptr), "bm_ledger_drain");
        return out;
    }
    void clear() { check(bm_ledger_clear(ledger_), "bm_ledger_clear"); }
    void set_peel(uint32_t rounds) { check(bm_ledger_set_peel(ledger_, rounds), "bm_ledger_set_peel"); }  // 0..64
    uint64_t rows() const {
        uint64_t n = 0;
        check(bm_ledger_rows(ledger_, &n), "bm_ledger_rows");
        return n;
    }
    bm_ledger_t* get() const { return ledger_; }

   private:
    Ledger() = default;
    bm_ledger_t* ledger_ = nullptr;
};

// floor(0xffff * 2^240 / difficulty_fx), the difficulty in units of 2^-32, as 32 bytes,
// most significant first: bm_target_from_difficulty_fx
inline void target_from_difficulty_fx(uint64_t difficulty_fx, uint8_t target[32]) {
    check(bm_target_from_difficulty_fx(difficulty_fx, target), "bm_target_from_difficulty_fx");
}

// Owns a bm_sessions_t: the pool's sessions -- extranonce1, share target, account and
// weight per slot -- and a bm_session_state_t per slot, kept across calls so that a
// verify call copies no session, with the vardiff step on top.  On the first device of a
// context (destroy it before the context), or SessionTable::cpu(capacity) in host memory
// with no GPU: the specification.  Not thread-safe; a device table shares its context's
// buffers, so one call at a time per context.
class SessionTable {
   public:
    SessionTable(Context& ctx, size_t capacity) {
        check(bm_sessions_create(ctx.get(), capacity, &table_), "bm_sessions_create");
    }
    static SessionTable cpu(size_t capacity) {
        SessionTable t;
        check(bm_sessions_create_cpu(capacity, &t.table_), "bm_sessions_create_cpu");
        return t;
    }
    SessionTable(const SessionTable&) = delete;
    SessionTable& operator=(const SessionTable&) = delete;
    SessionTable(SessionTable&& o) noexcept : table_(o.table_) { o.table_ = nullptr; }
    SessionTable& operator=(SessionTable&& o) noexcept {
        if (this != &o) {
            bm_sessions_destroy(table_);
            table_ = o.table_;
            o.table_ = nullptr;
        }
        return *this;
    }
    ~SessionTable() { bm_sessions_destroy(table_); }

    // Slot index[j] (index == nullptr: slot j) becomes init[j] with a fresh state whose
    // window starts at now_ms; difficulty_fx 0 closes the slot; a slot named twice takes
    // its later entry: bm_sessions_set.
    void set(const uint32_t* index, const std::vector<bm_session_init_t>& init, uint64_t now_ms) {
        check(bm_sessions_set(table_, index, init.size(), init.empty() ? nullptr : init.data(), now_ms), "bm_sessions_set");
    }
    // Slots [first, first + count) as the arrays the pool calls take; any output may be nullptr.
    void get(size_t first, size_t count, std::vector<bm_pool_session_t>* sessions, std::vector<uint32_t>* accounts,
             std::vector<uint64_t>* weights, std::vector<bm_session_state_t>* state) {
        std::vector<bm_pool_session_t> s(sessions ? count : 0);
        std::vector<uint32_t> a(accounts ? count : 0);
        std::vector<uint64_t> w(weights ? count : 0);
        std::vector<bm_session_state_t> st(state ? count : 0);
        check(bm_sessions_get(table_, first, count, s.empty() ? nullptr : s.data(), a.empty() ? nullptr : a.data(),
                              w.empty() ? nullptr : w.data(), st.empty() ? nullptr : st.data()),
              "bm_sessions_get");
        if (sessions) *sessions = std::move(s);
        if (accounts) *accounts = std::move(a);
        if (weights) *weights = std::move(w);
        if (state) *state = std::move(st);
    }
    std::vector<bm_session_state_t> state(size_t first, size_t count) {
        std::vector<bm_session_state_t> st;
        get(first, count, nullptr, nullptr, nullptr, &st);
        return st;
    }
    // Ledger::verify_jobs over the table's sessions, accounts and weights (ledger ==
    // nullptr: no row changes), and every accepted submission counts in its slot's
    // state: bm_sessions_verify_jobs.  All or nothing, as Ledger::verify_jobs.
    bm_ledger_result_t verify_jobs(Ledger* ledger, ShareSet* set, const std::vector<PoolJob>& jobs,
                                   const bm_jobs_submit_t* submits, size_t n, std::vector<bm_job_verdict_t>& verdicts) {
        const std::vector<bm_pool_job_t> j = pool_job_views(jobs, "SessionTable::verify_jobs");
        bm_ledger_result_t r;
        std::vector<bm_job_verdict_t> buf(n);
        check(bm_sessions_verify_jobs(table_, ledger ? ledger->get() : nullptr, set ? set->get() : nullptr,
                                      j.empty() ? nullptr : j.data(), j.size(), submits, n, n ? buf.data() : nullptr, &r),
              "bm_sessions_verify_jobs");
        verdicts = std::move(buf);
        return r;
    }
    // One vardiff step at now_ms: bm_sessions_retarget.  `changes` gets the changed slots,
    // ascending; room for `cap` of them (Error with status BM_EFULL, and the table as
    // before, when more change).
    bm_vardiff_result_t retarget(uint64_t now_ms, const bm_vardiff_policy_t& policy, size_t cap,
                                 std::vector<bm_vardiff_change_t>& changes) {
        bm_vardiff_result_t r;
        std::vector<bm_vardiff_change_t> buf(cap);
        check(bm_sessions_retarget(table_, now_ms, &policy, cap ? buf.data() : nullptr, cap, &r), "bm_sessions_retarget");
        buf.resize((size_t)r.changed);
        changes = std::move(buf);
        return r;
    }
    void clear() { check(bm_sessions_clear(table_), "bm_sessions_clear"); }
    uint64_t count() const {
        uint64_t n = 0;
        check(bm_sessions_count(table_, &n, nullptr), "bm_sessions_count");
        return n;
    }
    uint64_t capacity() const {
        uint64_t n = 0;
        check(bm_sessions_count(table_, nullptr, &n), "bm_sessions_count");
        return n;
    }
    bm_sessions_t* get() const { return table_; }

   private:
    SessionTable() = default;
    bm_sessions_t* table_ = nullptr;
};

}  // namespace btcminer

namespace bitcoin {

// message.go:5-11
enum class MsgType : int64_t { Join = 0, Request = 1, Result = 2 };

using DecodeError = bmjson::DecodeError;
namespace detail = ::bmjson;

// message.go:16-21
struct Message {
    MsgType Type = MsgType::Join;
    std::string Data;
    uint64_t Lower = 0, Upper = 0, Hash = 0, Nonce = 0;

    // json.Marshal of the Go struct: fields in declaration order, integers
    // as JSON numbers, Data with encoding/json's escaping.
    std::string Marshal() const {
        return "{\"Type\":" + std::to_string((int64_t)Type) + ",\"Data\":" + detail::go_json_string(Data) +
               ",\"Lower\":" + std::to_string(Lower) + ",\"Upper\":" + std::to_string(Upper) +
               ",\"Hash\":" + std::to_string(Hash) + ",\"Nonce\":" + std::to_string(Nonce) + "}";
    }

    // json.Unmarshal into a Message: absent or null fields keep zero values;
    // a field of the wrong JSON type, a number out of range, a Type outside
    // Join/Request/Result, or anything but one object throws DecodeError.
    static Message Unmarshal(std::string_view raw) {
        detail::Reader rd(raw, "bitcoin message");
        Message m;
        rd.expect('{');
        if (!rd.eat('}')) {
            do {
                const std::string key = rd.string();
                rd.expect(':');
                __int128 v = 0;
                if (key == "Type") {
                    if (rd.integer(INT64_MIN, INT64_MAX, &v)) {
                        if (v < 0 || v > 2) rd.fail("unknown message type");
                        m.Type = (MsgType)(int64_t)v;
                    } else {
                        m.Type = MsgType::Join;
                    }
                } else if (key == "Data") {
                    if (rd.literal("null")) m.Data.clear();
                    else if (rd.peek() == '"') m.Data = rd.string();
                    else rd.fail("Data is not a string");
                } else if (key == "Lower" || key == "Upper" || key == "Hash" || key == "Nonce") {
                    uint64_t& f = key == "Lower" ? m.Lower : key == "Upper" ? m.Upper : key == "Hash" ? m.Hash : m.Nonce;
                    f = rd.integer(0, (__int128)UINT64_MAX, &v) ? (uint64_t)v : 0;
                } else {
                    rd.skip_value();
                }
            } while (rd.eat(','));
            rd.expect('}');
        }
        if (!rd.at_end()) rd.fail("trailing bytes");
        return m;
    }

    // message.go:49-60
    std::string String() const {
        switch (Type) {
            case MsgType::Request:
                return "[Request " + Data + " " + std::to_string(Lower) + " " + std::to_string(Upper) + "]";
            case MsgType::Result: return "[Result " + std::to_string(Hash) + " " + std::to_string(Nonce) + "]";
            case MsgType::Join: return "[Join]";
        }
        return "";
    }
    bool operator==(const Message& o) const {
        return Type == o.Type && Data == o.Data && Lower == o.Lower && Upper == o.Upper && Hash == o.Hash &&
               Nonce == o.Nonce;
    }
};

// message.go:25-47
inline Message NewRequest(std::string data, uint64_t lower, uint64_t upper) {
    Message m;
    m.Type = MsgType::Request;
    m.Data = std::move(data);
    m.Lower = lower;
    m.Upper = upper;
    return m;
}
inline Message NewResult(uint64_t hash, uint64_t nonce) {
    Message m;
    m.Type = MsgType::Result;
    m.Hash = hash;
    m.Nonce = nonce;
    return m;
}
inline Message NewJoin() { return Message{}; }

// hash.go:11-15 -- "Only miners should ever need to call this method"; on
// the context's first GPU.
inline uint64_t Hash(btcminer::Context& ctx, std::string_view msg, uint64_t nonce) {
    return ctx.hash(msg, {nonce})[0];
}

}  // namespace bitcoin
