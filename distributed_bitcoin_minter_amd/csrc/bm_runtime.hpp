// bm_runtime.hpp -- what the units of the host runtime share (internal; the
// public interface is include/btcminer.h):
//   bm_ctx.cpp     contexts and devices: lifetime, buffers, knobs, the rank join
//   bm_combine.cpp the combine of a search's partials (RCCL allgather or host copies)
//   bm_search.cpp  the seven searches: kernel tables, sizing, one call driver, statistics
//   bm_aux.hip     the only unit with device code: the kernels of bm_aux_kernels.hpp,
//                  a host wrapper that launches the reduction, and the entry points
//                  built on them (bm_reduce_gpu, bm_hash_gpu, bm_header_hash_gpu), and
//                  bm_job_verify_gpu over job_verify_kernel (bm_job_verify_inst.hip) and
//                  bm_pool_verify_gpu over pool_verify_kernel (bm_pool_verify_inst.hip), and
//                  the device side of bm_share_set_verify (bm_share_set_inst.hip)
// The first three are plain C++ over the HIP host API.  DESIGN.md section 1.
#pragma once
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "bm_common.h"
#include "bm_header.hpp"
#include "bm_header_versions.hpp"
#include "bm_plan.hpp"
#include "btcminer.h"

// BM_CLOCK_PROBE=1 (make probe): workgroup 0 of every search launch stamps the
// clock counters into its counter strip (bm_kernels.hpp); the host reads them
// back for bm_launch_stat_t.clock_ghz.
#ifndef BM_CLOCK_PROBE
#define BM_CLOCK_PROBE 0
#endif

namespace bm {

constexpr int kMaxInnerDigits = 2;  // S <= 100 nonces per task: small dequeue chunks, short tail
constexpr uint32_t kNoncesPerLaneChunk = 100;  // default nonces per lane per dequeue (BTCMINER_CHUNK)
constexpr int kEventPairs = BM_MAX_LAUNCH_STATS;
// Launch streams per device.  Every search launch is a persistent grid that
// drains a work counter, so its last tasks leave CUs idle (about half a
// 100-nonce task, ~0.5 ms).  With more than one stream the launches of one
// call go out biggest first over the streams, and the next launch's
// workgroups fill the CUs the previous one frees.
constexpr int kMaxStreams = 4;
constexpr uint64_t kMaxTailNonces = 1ull << 40;
constexpr size_t kCtrStride = 32;  // u64 words per launch: counter [0], clock stamps [16..19]
constexpr int kCtrClockSlot = 16;  // = bm_kernels.hpp kClockSlot (bm_aux.hip asserts it)
constexpr size_t kMinCounterStrips = 256, kMinPartials = 4096;  // what a device starts with

// What each device / rank contributes to the combine: its partial and a
// status word (a rank that failed the call before the combine still takes
// part in the allgather, with its status here).  32 bytes = 4 u64.
struct Slot {
    Partial p;
    uint64_t status;
    uint64_t pad;
};
static_assert(sizeof(Slot) == 32, "slot layout");
constexpr size_t kSlotWords = sizeof(Slot) / sizeof(uint64_t);

struct DeviceCtx {
    int id = -1;
    int cus = 0;
    // everything init_device and grow() made (nothing else allocates), for destroy_device
    std::vector<std::pair<void*, bool>> owned;  // (memory, pinned host memory?)
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;
    hipStream_t stream = nullptr;
    Partial* d_part = nullptr;
    size_t part_cap = 0;
    unsigned long long* d_ctr = nullptr;  // per launch a strip of kCtrStride words: [0] dequeue
                                          // counter, [16..19] clock stamps (bm_kernels.hpp)
    unsigned long long* h_ctr = nullptr;  // pinned copy of the strips
    size_t ctr_cap = 0, hctr_cap = 0;
    unsigned long long* d_hit = nullptr;  // target search: the lowest nonce at or below the target seen so
                                          // far (all-ones: none); an allocation, hence a line, of its own
    unsigned long long* h_hit = nullptr;  // pinned copy
    unsigned long long* d_hcount = nullptr;  // hit enumerations: the hits counted so far (an allocation of its own)
    unsigned long long* h_hcount = nullptr;  // pinned copy
    Partial* d_hbuf = nullptr;               // the first hbuf_cap of them, in the order the lanes took their slots
    size_t hbuf_cap = 0;                     // grows to the largest cap asked for
    Slot* d_slot = nullptr;    // this device's slot (reduce_partials writes its partial)
    Slot* d_gather = nullptr;  // nslots slots (allgather target)
    Slot* h_slots = nullptr;   // pinned: nslots slots, + 1 staging slot (a failed rank's status)
    int nslots = 1;
    Partial* d_test = nullptr;    // bm_reduce_gpu's staging buffer
    size_t test_cap = 0;
    uint64_t* d_hash_io = nullptr;  // bm_hash_gpu: n nonces, then n hashes
    size_t hash_cap = 0;
    uint32_t* d_hdr_io = nullptr;  // bm_header_hash_gpu: n nonces, then 8 digest words per nonce
    size_t hdr_cap = 0;
    uint64_t* d_verify = nullptr;  // bm_job_verify_gpu: tail template, branch, n submissions, then n verdicts
                                   // (bm_pool_verify_gpu: the session table between the branch and the submissions;
                                   // bm_share_set_verify: two control words before the verdicts, 8 bytes per lane after)
    uint64_t* h_verify = nullptr;  // pinned copy of the same layout: staged for the copy up, target of the copy back
    size_t verify_cap = 0, hverify_cap = 0;  // in 8-byte units
    hipEvent_t ev[2 * kEventPairs] = {};
    hipStream_t aux[kMaxStreams - 1] = {};  // extra launch streams (ctx->streams > 1)
    hipEvent_t fork = nullptr, join[kMaxStreams - 1] = {};
    hipEvent_t bal[2] = {};     // the device's first op and the end of its reduction (balance, timing)
    hipEvent_t ag[2] = {};      // around the device's allgather (timing): its wait for the peers + transfer
    hipEvent_t own_done = nullptr;  // rank contexts: this rank's reduction done (before the allgather)
    uint64_t piece_nonces = 0;  // nonces of the device's piece in the last call
    std::chrono::steady_clock::time_point submitted{};  // host time of the call's first op on this device
    int test_delay_us = 0;      // test hook: hold back this device's submission (bm_ctx_set_test_start_delay)
    ncclComm_t comm = nullptr;  // multi-device ctx: ncclCommInitAll; joined rank ctx: the process group's
    std::vector<std::pair<const void*, int>> occ;  // kernel -> blocks per CU
    double wall_clock_hz = 100e6;                  // s_memrealtime rate
};

// The seven searches share one plan -> enqueue -> combine -> stats path
// (bm_search.cpp); a Mode says which one a call is, and carries what its
// kernels take beyond a launch's own arguments.  DESIGN.md section 1, "Host
// runtime layout", lists what a mode changes.  Five kinds serve the seven: the
// two single-header searches are HeaderVersions / HeaderVersionsHits over one version.
enum class Kind { Search, Target, Hits, HeaderVersions, HeaderVersionsHits };
struct Mode {
    Kind kind = Kind::Search;
    uint64_t target = 0;  // Target, Hits: the 64-bit bound (the header kinds' 256-bit target is in HeaderVersionsArgs)
    uint64_t cap = 0;     // Hits, HeaderVersionsHits: entries of the hit buffer
    // first hit wins: launches in ascending nonce order, one hit word per device
    // (HeaderVersions: the word holds a (nonce, version index) key, shared by the device's group launches)
    bool first_hit() const { return kind == Kind::Target || kind == Kind::HeaderVersions; }
    // every hit: a counter and a buffer of 16-byte entries per device (d_hcount, d_hbuf)
    // (HeaderVersionsHits: both shared by the device's group launches, the counter zeroed once)
    bool every_hit() const { return kind == Kind::Hits || kind == Kind::HeaderVersionsHits; }
    // the decimal modes whose kernels take the 64-bit target as a parameter
    bool target64() const { return kind == Kind::Target || kind == Kind::Hits; }
};

// One kernel launch of a call, with what the ordering and the accounting of
// dispatched nonces need, so that neither looks inside the argument block.
struct Launch {
    const void* fn;
    union {
        SearchArgs search;  // Search, Target, Hits
        HeaderVersionsArgs<kMaxVersionSlots> versions;  // HeaderVersions, HeaderVersionsHits: a launch of M slots reads the first M
    } args;                 // the kernel's first parameter, by value
    uint64_t first_nonce;  // the lowest nonce it scans
    uint64_t tasks;        // what its work counter runs up to
    uint64_t task_nonces;  // nonces per task
    bm_launch_stat_t stat;  // stat.grid: its workgroups
};

// bm_ctx_join_rank's worker: one communicator set-up, shared with the caller
// (who may give up on it: then the worker aborts what it made).  A join the
// caller gave up on stays on the context as its pending join, so a context
// never has more than one worker inside RCCL.
struct JoinJob {
    std::mutex m;
    std::condition_variable cv;
    bool done = false, abandoned = false;
    ncclComm_t comm = nullptr;
    int rc = BM_ERCCL;
    double init_ms = 0.0;  // the init's host time, until it settled
};

inline int hip_status(hipError_t e) { return e == hipSuccess ? BM_OK : BM_EHIP; }

#define BM_HIP(call)                                     \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) return bm::hip_status(e_); \
    } while (0)
#define BM_TRY(call)  /* the same for a call that returns a BM_* status */ \
    do {                                                                   \
        const int rc_ = (call);                                            \
        if (rc_ != BM_OK) return rc_;                                      \
    } while (0)

// BTCMINER_TRACE=1: one stderr line per step of the group set-up and combine
// (diagnostics of multi-process runs; off by default)
void trace(const char* fmt, ...);

// The submission threads of a multi-device context: created once,
// at the context's first search over several devices, and kept until the
// context is destroyed, so a search does not create and join N - 1 threads
// (about 0.2 ms at N = 8, most of a small job's fixed cost).
// run(n, f) runs f(1) .. f(n - 1) on the pool's threads and f(0) on the
// caller, and returns when all of them have.  f must not throw (the search
// wraps it in guarded()).  A context is not re-entrant, so one run at a time.
class SubmitPool {
   public:
    SubmitPool() = default;
    SubmitPool(const SubmitPool&) = delete;
    SubmitPool& operator=(const SubmitPool&) = delete;
    ~SubmitPool() { stop(); }

    // false when the threads could not be started: the caller submits serially
    bool run(int n, const std::function<void(int)>& f);
    int threads() const { return (int)th_.size(); }

   private:
    bool ensure(int k);
    void loop(int di, uint64_t seen);  // seen: the generation the worker was created in
    void stop();
    std::mutex m_;
    std::condition_variable work_, done_;
    std::vector<std::thread> th_;
    const std::function<void(int)>* job_ = nullptr;
    uint64_t gen_ = 0;
    int pending_ = 0;
    bool quit_ = false;
};

// Restores the caller's current device on scope exit.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// f() as a status: an exception (std::bad_alloc from a plan or order vector,
// anything else a bug) becomes BM_ENOMEM / BM_EINTERNAL instead of leaving
// the C ABI -- or, on a submission thread, calling std::terminate and taking
// the host process down.
template <class F>
int guarded(F&& f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return BM_ENOMEM;
    } catch (...) {
        return BM_EINTERNAL;
    }
}

}  // namespace bm

struct bm_ctx {
    std::vector<bm::DeviceCtx> devs;
    bool timing = false;
    int blocks_per_cu = 0;
    int max_windows = bm::kDefaultMaxWindows;
    int combine = BM_COMBINE_AUTO;
    int task_digits = 0;  // 0: per launch (size_launch); 1 or 2: forced
    uint64_t tail_nonces = 1ull << 24;  // split off the biggest launch's last nonces (BTCMINER_TAIL; 0: off; profiles/r01/ab_tail.log)
    int streams = 2;      // launch streams per device (1..kMaxStreams; BTCMINER_STREAMS; profiles/r01/ab_streams.log)
    bool nccl_ready = false;
    int rccl_status = 0;      // multi-device ctx: the RCCL failure it fell back from (then: host copies)
    int rank = 0, world = 1;  // rank contexts: this process's place in the group
    bool rank_ctx = false;    // made by bm_ctx_create_rank_local (one device, one slot of `world`)
    bool joined = false;      // rank ctx: member of an RCCL group (devs[0].comm)
    int group_status = 0;     // joined rank ctx whose communicator failed (BM_ERCCL / BM_ETIMEDOUT)
    int peer_timeout_ms = BM_DEFAULT_PEER_TIMEOUT_MS;  // joined rank ctx: wait at most this long for
                                                       // the group (0: no limit)
    double rccl_init_ms = 0.0;  // host time the current communicator(s) took to form
    int fault_after = -1;     // test hook: fail after enqueueing this many launches (-1: off)
    int test_rccl_fault = 0;  // test hook: 1 communicator set-up fails, 2 every allgather fails,
                              // 3 the gathered slots report a failed peer (rank groups)
    uint64_t lane_chunk = bm::kNoncesPerLaneChunk;  // nonces per lane per dequeue, at most (BTCMINER_CHUNK)
    std::vector<uint32_t> shares;  // the partitioner's shares per slot (empty: near-equal pieces)
    bool balance = false;          // multi-device: shares follow each device's measured rate
    int header_group = bm::kMaxVersionSlots;  // bm_search_header_versions_gpu: versions per launch, at most (1, 2, 4;
                                          // BTCMINER_HEADER_GROUP; DESIGN.md "Version rolling")
    bool padc = true;              // use search_kernel_padc / _padk where they apply (BTCMINER_PADC=0: never; A/B knob)
    // rank ctx: a join whose caller timed out while its worker was still
    // inside RCCL (the worker aborts the communicator if it ever gets one)
    std::shared_ptr<bm::JoinJob> pending_join;
    std::thread pending_worker;
    bm_stats_t stats;
    bm_target_stats_t tstats;  // the last bm_search_target_gpu / bm_search_header_gpu / bm_search_header_versions_gpu
                               // (zero after a failed one)
    bm::SubmitPool submit;  // multi-device: one submission thread per device but the first (last member:
                            // stopped first, when every device is idle)
};

namespace bm {

// ---- bm_ctx.cpp ----
// Grows the device buffer p (pinned: a pinned host buffer) to at least n
// elements of elem bytes.  The old buffer goes only once the new one exists,
// so a failed growth leaves the context as it was: BM_EHIP, or oom_status
// when the device is out of memory.  The caller has made d's device current.
int grow_bytes(DeviceCtx& d, void** p, size_t* cap, size_t n, size_t elem, bool pinned, int oom_status);
template <class T>
int grow(DeviceCtx& d, T*& p, size_t& cap, size_t n, size_t elem = sizeof(T), bool pinned = false,
         int oom_status = BM_EHIP) {
    return grow_bytes(d, reinterpret_cast<void**>(&p), &cap, n, elem, pinned, oom_status);
}
int ensure_counters(DeviceCtx& d, size_t strips);  // d_ctr and its pinned copy h_ctr

// ---- bm_combine.cpp ----
// The RCCL figures of the last combine, into the stats (used = false: none).
void record_rccl(bm_ctx* ctx, bool used);
int combine_local(bm_ctx* ctx, Partial* best_out, bool host_only);
int combine_group(bm_ctx* ctx, int own_rc, Partial* best_out);
int rccl_version();

// ---- bm_search.cpp ----
extern const void* g_header_hash;  // header_hash_kernel, registered by bm_header_inst.hip

// ---- bm_aux.hip: launches of the kernels of bm_aux_kernels.hpp ----
// lexicographic min of n partials (n = 0: (2^64-1, 2^64-1)) into *out
int launch_reduce_partials(const Partial* part, uint32_t n, Partial* out, hipStream_t s);

}  // namespace bm
