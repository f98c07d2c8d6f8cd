// bm_ctx.cpp -- contexts and their devices (include/btcminer.h): creation and
// teardown, the device buffers, environment knobs, setters and getters, and a
// rank context's join / leave of its RCCL group.  Plain C++ over the HIP host
// API; see bm_runtime.hpp for the layout of the host runtime.
#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <system_error>

#include "bm_runtime.hpp"

namespace bm {

void trace(const char* fmt, ...) {
    static const bool on = std::getenv("BTCMINER_TRACE") != nullptr;
    if (!on) return;
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "[btcminer] ");
    std::vfprintf(stderr, fmt, ap);
    std::fprintf(stderr, "\n");
    va_end(ap);
}

bool SubmitPool::run(int n, const std::function<void(int)>& f) {
    if (!ensure(n - 1)) return false;
    {
        std::lock_guard<std::mutex> g(m_);
        job_ = &f;
        pending_ = n - 1;
        ++gen_;
    }
    work_.notify_all();
    f(0);
    std::unique_lock<std::mutex> l(m_);
    done_.wait(l, [&] { return pending_ == 0; });
    job_ = nullptr;
    return true;
}

bool SubmitPool::ensure(int k) {
    if ((int)th_.size() == k) return true;
    stop();  // (a context's device count never changes; this is only the first call)
    // A worker starts from the generation of its creation, so a pool re-created
    // after a run cannot wake on a stale job.  Read here, by the only thread that
    // bumps gen_, not by the worker when it starts: run() bumps it right after
    // this returns, and a worker that started later would take that job for seen.
    const uint64_t gen = gen_;
    try {
        for (int i = 0; i < k; ++i) th_.emplace_back([this, i, gen] { loop(i + 1, gen); });
    } catch (const std::system_error&) {
        stop();
        return false;
    }
    return true;
}

void SubmitPool::loop(int di, uint64_t seen) {
    for (;;) {
        const std::function<void(int)>* job;
        {
            std::unique_lock<std::mutex> l(m_);
            work_.wait(l, [&] { return quit_ || gen_ != seen; });
            if (quit_) return;
            seen = gen_;
            job = job_;
        }
        (*job)(di);
        std::lock_guard<std::mutex> g(m_);
        if (--pending_ == 0) done_.notify_one();
    }
}

void SubmitPool::stop() {
    {
        std::lock_guard<std::mutex> g(m_);
        quit_ = true;
    }
    work_.notify_all();
    for (auto& t : th_) t.join();
    th_.clear();
    quit_ = false;
}

int grow_bytes(DeviceCtx& d, void** p, size_t* cap, size_t n, size_t elem, bool pinned, int oom_status) {
    if (n <= *cap) return BM_OK;
    if (!*p) d.owned.reserve(d.owned.size() + 1);  // (so that registering the buffer cannot throw)
    void* nb = nullptr;
    const hipError_t e = pinned ? hipHostMalloc(&nb, n * elem, hipHostMallocDefault) : hipMalloc(&nb, n * elem);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? oom_status : BM_EHIP;
    }
    if (*p) {  // the new buffer takes the old one's place in the list
        (void)(pinned ? hipHostFree(*p) : hipFree(*p));
        std::find(d.owned.begin(), d.owned.end(), std::make_pair(*p, pinned))->first = nb;
    } else {
        d.owned.emplace_back(nb, pinned);
    }
    *p = nb;
    *cap = n;
    return BM_OK;
}

int ensure_counters(DeviceCtx& d, size_t strips) {
    const size_t n = std::max(strips, kMinCounterStrips), elem = kCtrStride * sizeof(unsigned long long);
    BM_TRY(grow(d, d.h_ctr, d.hctr_cap, n, elem, true));
    return grow(d, d.d_ctr, d.ctr_cap, n, elem);
}

namespace {

// A buffer of fixed size, an event, a stream of d: registered for destroy_device.
template <class T>
int alloc(DeviceCtx& d, T*& p, size_t bytes, bool pinned = false) {
    size_t cap = 0;
    return grow(d, p, cap, bytes, 1, pinned);
}

int new_event(DeviceCtx& d, hipEvent_t& e, unsigned flags = hipEventDefault) {
    BM_HIP(hipEventCreateWithFlags(&e, flags));
    d.events.push_back(e);
    return BM_OK;
}

int new_stream(DeviceCtx& d, hipStream_t& s) {
    BM_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    d.streams.push_back(s);
    return BM_OK;
}

// nslots: partials the combine gathers (devices of the ctx, or ranks of its
// process group).
int init_device(DeviceCtx& d, int id, int nslots) {
    d.id = id;
    BM_HIP(hipSetDevice(id));
    hipDeviceProp_t prop;
    BM_HIP(hipGetDeviceProperties(&prop, id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return BM_ENODEV;  // kernels are gfx950 code objects
    d.cus = prop.multiProcessorCount;
    int wall_khz = 0;
    if (hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, id) == hipSuccess && wall_khz > 0)
        d.wall_clock_hz = 1e3 * wall_khz;
    BM_TRY(new_stream(d, d.stream));
    d.nslots = nslots;
    BM_TRY(alloc(d, d.d_slot, sizeof(Slot)));
    BM_TRY(alloc(d, d.d_hit, 128));
    BM_TRY(alloc(d, d.h_hit, sizeof(unsigned long long), true));
    BM_TRY(alloc(d, d.d_hcount, 128));
    BM_TRY(alloc(d, d.h_hcount, sizeof(unsigned long long), true));
    BM_TRY(alloc(d, d.d_gather, sizeof(Slot) * (size_t)nslots));
    BM_TRY(alloc(d, d.h_slots, sizeof(Slot) * (size_t)(nslots + 1), true));
    for (auto& e : d.ev) BM_TRY(new_event(d, e));
    for (auto& s : d.aux) BM_TRY(new_stream(d, s));
    BM_TRY(new_event(d, d.fork, hipEventDisableTiming));
    for (auto& e : d.join) BM_TRY(new_event(d, e, hipEventDisableTiming));
    for (auto& e : d.bal) BM_TRY(new_event(d, e));
    for (auto& e : d.ag) BM_TRY(new_event(d, e));
    BM_TRY(new_event(d, d.own_done, hipEventDisableTiming));
    BM_TRY(ensure_counters(d, kMinCounterStrips));
    return grow(d, d.d_part, d.part_cap, kMinPartials);
}

void destroy_device(DeviceCtx& d) {
    if (d.id < 0) return;
    (void)hipSetDevice(d.id);
    for (hipStream_t s : d.streams) (void)hipStreamSynchronize(s);
    // abort, not destroy: the streams are drained, so nothing of ours is in
    // flight, and an abort never waits on a peer (a joined rank whose group
    // lost a member would otherwise block in teardown)
    if (d.comm) (void)ncclCommAbort(d.comm);
    d.comm = nullptr;
    for (hipEvent_t e : d.events) (void)hipEventDestroy(e);
    for (const auto& m : d.owned) (void)(m.second ? hipHostFree(m.first) : hipFree(m.first));
    for (hipStream_t s : d.streams) (void)hipStreamDestroy(s);
}

// Environment knobs read at context creation.  Malformed or out-of-range
// values keep the default (results never depend on them).
void read_env(bm_ctx* ctx) {
    if (const char* e = std::getenv("BTCMINER_STREAMS")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= kMaxStreams) ctx->streams = v;
    }
    if (const char* e = std::getenv("BTCMINER_TAIL")) {
        char* end = nullptr;
        errno = 0;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end != e && *end == '\0' && errno == 0 && v <= kMaxTailNonces) ctx->tail_nonces = v;
    }
    if (const char* e = std::getenv("BTCMINER_PADC")) ctx->padc = std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("BTCMINER_HEADER_GROUP")) {
        const int v = std::atoi(e);
        if (v == 1 || v == 2 || v == 4) ctx->header_group = v;
    }
    if (const char* e = std::getenv("BTCMINER_CHUNK")) {
        char* end = nullptr;
        errno = 0;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end != e && *end == '\0' && errno == 0 && v >= 10 && v <= 100000) ctx->lane_chunk = v;
    }
}

int create_ctx(const int* devices, int n, int nslots, bm_ctx** out) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return BM_ENODEV;
    for (int i = 0; i < n; ++i)
        if (devices[i] < 0 || devices[i] >= count) return BM_ENODEV;
    bm_ctx* ctx = new (std::nothrow) bm_ctx();
    if (!ctx) return BM_ENOMEM;
    std::memset(&ctx->stats, 0, sizeof ctx->stats);
    std::memset(&ctx->tstats, 0, sizeof ctx->tstats);
    record_rccl(ctx, false);
    read_env(ctx);
    DeviceGuard guard;
    ctx->devs.resize(n);
    for (int i = 0; i < n; ++i) {
        int rc = init_device(ctx->devs[i], devices[i], nslots);
        if (rc != BM_OK) {
            for (auto& d : ctx->devs) destroy_device(d);
            delete ctx;
            return rc;
        }
    }
    *out = ctx;
    return BM_OK;
}

void join_worker(std::shared_ptr<JoinJob> job, int dev, int world, int rank, ncclUniqueId u) {
    ncclComm_t comm = nullptr;
    int rc = BM_ERCCL;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipSetDevice(dev) == hipSuccess) {
        ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
        cfg.blocking = 0;
        ncclResult_t r = ncclCommInitRankConfig(&comm, world, u, rank, &cfg);
        trace("rank %d: init returned %d", rank, (int)r);
        while (r == ncclInProgress) {
            {
                std::lock_guard<std::mutex> g(job->m);
                if (job->abandoned) break;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
            if (ncclCommGetAsyncError(comm, &r) != ncclSuccess) r = ncclInternalError;
        }
        rc = r == ncclSuccess ? BM_OK : BM_ERCCL;
    }
    // publish; a communicator nobody will use (a failed set-up, or a caller
    // that gave up) is aborted first, outside the lock: an abort may block,
    // and the caller's timed wait must still be able to take the lock
    for (;;) {
        {
            std::lock_guard<std::mutex> g(job->m);
            if (!comm || (rc == BM_OK && !job->abandoned)) {
                job->comm = comm;
                job->rc = rc;
                job->init_ms =
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                job->done = true;
                job->cv.notify_all();
                return;
            }
        }
        (void)ncclCommAbort(comm);
        comm = nullptr;
        trace("rank %d: communicator aborted", rank);
    }
}

}  // namespace
}  // namespace bm

extern "C" {

int bm_abi_version(void) { return BM_ABI_VERSION; }

const char* bm_strerror(int status) {
    switch (status) {
        case BM_OK: return "ok";
        case BM_EINVAL: return "invalid argument";
        case BM_ENODEV: return "no usable gfx950 device";
        case BM_EHIP: return "HIP runtime error";
        case BM_ERCCL: return "RCCL error";
        case BM_ENOMEM: return "out of memory";
        case BM_EINTERNAL: return "internal error";
        case BM_EPEER: return "another rank of the group failed";
        case BM_ETIMEDOUT: return "the group did not answer within the peer timeout";
        case BM_EFULL: return "the share set is full";
        default: return "unknown status";
    }
}

int bm_device_count(int* out) {
    if (!out) return BM_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return BM_OK;
}

int bm_device_pci_bus_id(int device, char* buf, int len) {
    if (!buf || len < 13) return BM_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return BM_ENODEV;
    return hipDeviceGetPCIBusId(buf, len, device) == hipSuccess ? BM_OK : BM_EHIP;
}

int bm_ctx_create_devices(const int* devices, int n, bm_ctx_t** out) {
    if (!out || !devices || n < 1) return BM_EINVAL;
    return bm::create_ctx(devices, n, n, out);
}

int bm_rccl_unique_id(uint8_t* id) {
    if (!id) return BM_EINVAL;
    static_assert(sizeof(ncclUniqueId) == BM_RCCL_ID_BYTES, "RCCL unique id size");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return BM_ERCCL;
    std::memcpy(id, &u, sizeof u);
    return BM_OK;
}

int bm_ctx_create_rank_local(int device, int rank, int world, bm_ctx_t** out) {
    if (!out || world < 1 || world > BM_MAX_SLOTS || rank < 0 || rank >= world) return BM_EINVAL;
    bm_ctx* ctx = nullptr;
    int rc = bm::create_ctx(&device, 1, world, &ctx);
    if (rc != BM_OK) return rc;
    ctx->rank = rank;
    ctx->world = world;
    ctx->rank_ctx = true;
    *out = ctx;
    return BM_OK;
}

int bm_ctx_join_rank(bm_ctx_t* ctx, const uint8_t* id, int timeout_ms) {
    if (!ctx || !id || !ctx->rank_ctx || ctx->joined || timeout_ms < 0) return BM_EINVAL;
    if (ctx->test_rccl_fault == 1) return BM_ERCCL;  // test hook
    bm::DeviceGuard guard;
    bm::DeviceCtx& d = ctx->devs[0];
    if (hipSetDevice(d.id) != hipSuccess) return BM_EHIP;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    const int dev = d.id, world = ctx->world, rank = ctx->rank;
    // one deadline for the whole call: the wait for a pending join and the
    // new join share timeout_ms
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms);
    // An earlier join this context gave up on may still be inside RCCL: wait
    // for it (within this call's timeout) rather than put a second worker
    // there; it has abandoned = true, so it aborts whatever it ends with.
    if (ctx->pending_join) {
        auto& pj = ctx->pending_join;
        std::unique_lock<std::mutex> lk(pj->m);
        const bool ended = timeout_ms == 0 ? (pj->cv.wait(lk, [&] { return pj->done; }), true)
                                           : pj->cv.wait_until(lk, deadline, [&] { return pj->done; });
        lk.unlock();
        if (!ended) {
            bm::trace("rank %d: the previous join is still inside RCCL; not starting another", rank);
            return BM_ETIMEDOUT;
        }
        ctx->pending_worker.join();
        ctx->pending_join.reset();
        if (timeout_ms > 0 && std::chrono::steady_clock::now() >= deadline) {
            bm::trace("rank %d: the previous join ended, but no time is left for a new one", rank);
            return BM_ETIMEDOUT;
        }
    }
    // The join runs on a worker thread: a non-blocking ncclCommInitRankConfig
    // polled until it settles.  With a timeout the caller waits at most that
    // long; past it the worker becomes the context's pending join (neither
    // the init of a group whose peer never comes nor its abort is guaranteed
    // to return promptly), and the call returns BM_ETIMEDOUT.
    auto job = std::make_shared<bm::JoinJob>();
    bm::trace("rank %d/%d: joining (timeout %d ms)", rank, world, timeout_ms);
    std::thread worker([job, dev, world, rank, u]() { bm::join_worker(job, dev, world, rank, u); });
    std::unique_lock<std::mutex> lk(job->m);
    if (timeout_ms == 0) {
        job->cv.wait(lk, [&] { return job->done; });
    } else if (!job->cv.wait_until(lk, deadline, [&] { return job->done; })) {
        job->abandoned = true;
        lk.unlock();
        ctx->pending_join = job;
        ctx->pending_worker = std::move(worker);
        bm::trace("rank %d: join timed out; the worker aborts the communicator if it ever gets one", rank);
        return BM_ETIMEDOUT;
    }
    lk.unlock();
    worker.join();
    bm::trace("rank %d: join status %d", rank, job->rc);
    if (job->rc != BM_OK) return job->rc;
    d.comm = job->comm;
    ctx->rccl_init_ms = job->init_ms;
    ctx->joined = true;
    ctx->group_status = BM_OK;
    return BM_OK;
}

int bm_ctx_leave_rank(bm_ctx_t* ctx) {
    if (!ctx || !ctx->rank_ctx) return BM_EINVAL;
    bm::DeviceGuard guard;
    bm::DeviceCtx& d = ctx->devs[0];
    if (d.comm) {
        // leaving is what a rank does when the group cannot be trusted (a
        // peer failed to join, or the caller falls back): abort, which frees
        // this rank's side without waiting for any peer
        (void)hipSetDevice(d.id);
        (void)hipStreamSynchronize(d.stream);
        (void)ncclCommAbort(d.comm);
        d.comm = nullptr;
    }
    ctx->joined = false;
    ctx->group_status = BM_OK;
    return BM_OK;
}

int bm_ctx_rank_joined(const bm_ctx_t* ctx, int* joined) {
    if (!ctx || !joined) return BM_EINVAL;
    *joined = ctx->joined ? 1 : 0;
    return BM_OK;
}

int bm_ctx_set_peer_timeout(bm_ctx_t* ctx, int timeout_ms) {
    if (!ctx || timeout_ms < 0) return BM_EINVAL;
    ctx->peer_timeout_ms = timeout_ms;
    return BM_OK;
}

int bm_ctx_create_rank(int device, int rank, int world, const uint8_t* id, bm_ctx_t** out) {
    if (!out || !id) return BM_EINVAL;
    bm_ctx* ctx = nullptr;
    int rc = bm_ctx_create_rank_local(device, rank, world, &ctx);
    if (rc != BM_OK) return rc;
    rc = bm_ctx_join_rank(ctx, id, 0);  // blocks until every rank of the group has joined
    if (rc != BM_OK) {
        bm_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return BM_OK;
}

int bm_ctx_rank(const bm_ctx_t* ctx, int* rank, int* world) {
    if (!ctx || !rank || !world) return BM_EINVAL;
    *rank = ctx->rank;
    *world = ctx->world;
    return BM_OK;
}

int bm_ctx_create(int num_gpus, bm_ctx_t** out) {
    if (!out || num_gpus < 0) return BM_EINVAL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return BM_ENODEV;
    if (num_gpus == 0) num_gpus = count;
    if (num_gpus > count) return BM_ENODEV;
    std::vector<int> ids(num_gpus);
    for (int i = 0; i < num_gpus; ++i) ids[i] = i;
    return bm_ctx_create_devices(ids.data(), num_gpus, out);
}

int bm_ctx_destroy(bm_ctx_t* ctx) {
    if (!ctx) return BM_EINVAL;
    if (ctx->pending_join) {
        // a join worker that has ended is joined; one still blocked inside
        // RCCL holds only its JoinJob, so it is left to end with the process
        bool ended;
        {
            std::lock_guard<std::mutex> g(ctx->pending_join->m);
            ended = ctx->pending_join->done;
        }
        if (ended)
            ctx->pending_worker.join();
        else
            ctx->pending_worker.detach();
    }
    bm::DeviceGuard guard;
    for (auto& d : ctx->devs) bm::destroy_device(d);
    delete ctx;
    return BM_OK;
}

int bm_ctx_num_devices(const bm_ctx_t* ctx, int* out) {
    if (!ctx || !out) return BM_EINVAL;
    *out = (int)ctx->devs.size();
    return BM_OK;
}

int bm_ctx_last_stats(const bm_ctx_t* ctx, bm_stats_t* out) {
    if (!ctx || !out) return BM_EINVAL;
    *out = ctx->stats;
    return BM_OK;
}

int bm_ctx_last_target_stats(const bm_ctx_t* ctx, bm_target_stats_t* out) {
    if (!ctx || !out) return BM_EINVAL;
    *out = ctx->tstats;
    return BM_OK;
}

int bm_ctx_set_test_fault(bm_ctx_t* ctx, int launches) {
    if (!ctx || launches < -1) return BM_EINVAL;
    ctx->fault_after = launches;
    return BM_OK;
}

int bm_ctx_set_test_start_delay(bm_ctx_t* ctx, int device, int delay_us) {
    if (!ctx || device < 0 || device >= (int)ctx->devs.size() || delay_us < 0) return BM_EINVAL;
    ctx->devs[(size_t)device].test_delay_us = delay_us;
    return BM_OK;
}

int bm_ctx_set_test_rccl_fault(bm_ctx_t* ctx, int where) {
    if (!ctx || where < 0 || where > 3) return BM_EINVAL;
    ctx->test_rccl_fault = where;
    return BM_OK;
}

int bm_ctx_set_timing(bm_ctx_t* ctx, int enable) {
    if (!ctx) return BM_EINVAL;
    ctx->timing = enable != 0;
    return BM_OK;
}

int bm_ctx_set_blocks_per_cu(bm_ctx_t* ctx, int blocks_per_cu) {
    if (!ctx || blocks_per_cu < 0 || blocks_per_cu > 32) return BM_EINVAL;
    ctx->blocks_per_cu = blocks_per_cu;
    return BM_OK;
}

int bm_ctx_set_combine(bm_ctx_t* ctx, int mode) {
    if (!ctx || mode < BM_COMBINE_AUTO || mode > BM_COMBINE_HOST) return BM_EINVAL;
    if (ctx->rank_ctx && mode != BM_COMBINE_AUTO) return BM_EINVAL;  // a rank combines through its group
    ctx->combine = mode;
    return BM_OK;
}

int bm_ctx_set_task_digits(bm_ctx_t* ctx, int digits) {
    if (!ctx || digits < 0 || digits > bm::kMaxInnerDigits) return BM_EINVAL;
    ctx->task_digits = digits;
    return BM_OK;
}

int bm_ctx_set_max_windows(bm_ctx_t* ctx, int max_windows) {
    if (!ctx || max_windows < 0) return BM_EINVAL;
    ctx->max_windows = max_windows;
    return BM_OK;
}

int bm_ctx_set_split(bm_ctx_t* ctx, const uint32_t* shares, int n) {
    if (!ctx || n < 0 || (n > 0 && !shares)) return BM_EINVAL;
    if (n == 0) {
        ctx->shares.clear();
        return BM_OK;
    }
    const int slots = ctx->rank_ctx ? ctx->world : (int)ctx->devs.size();
    if (n != slots) return BM_EINVAL;
    for (int i = 0; i < n; ++i)
        if (shares[i] == 0) return BM_EINVAL;
    ctx->shares.assign(shares, shares + n);
    return BM_OK;
}

int bm_ctx_get_split(const bm_ctx_t* ctx, uint32_t* shares, int cap, int* n) {
    if (!ctx || !n || cap < 0 || (cap > 0 && !shares)) return BM_EINVAL;
    *n = (int)ctx->shares.size();
    for (int i = 0; i < cap && i < *n; ++i) shares[i] = ctx->shares[(size_t)i];
    return BM_OK;
}

int bm_ctx_set_balance(bm_ctx_t* ctx, int enable) {
    // a rank sees only its own device: a group's shares need an exchange,
    // which is the caller's (the same bm_ctx_set_split on every rank)
    if (!ctx || (ctx->rank_ctx && ctx->world > 1 && enable)) return BM_EINVAL;
    ctx->balance = enable != 0;
    return BM_OK;
}

int bm_split_range(uint64_t lower, uint64_t upper, const uint32_t* shares, int n, uint64_t* lo, uint64_t* hi) {
    if (n < 1 || n > BM_MAX_SLOTS || !lo || !hi) return BM_EINVAL;
    std::vector<uint32_t> sh;
    if (shares) {
        for (int i = 0; i < n; ++i)
            if (shares[i] == 0) return BM_EINVAL;
        sh.assign(shares, shares + n);
    }
    const std::vector<bm::Piece> p = bm::slot_pieces(lower, upper, n, sh);
    for (int i = 0; i < n; ++i) {
        lo[i] = p[(size_t)i].lo;
        hi[i] = p[(size_t)i].hi;
    }
    return BM_OK;
}

int bm_plan_segments(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, bm_segment_t* segs, int cap,
                     int* nseg) {
    return bm_plan_segments_ex(msg, len, lower, upper, bm::kDefaultMaxWindows, segs, cap, nseg);
}

int bm_plan_segments_ex(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, int max_windows,
                        bm_segment_t* segs, int cap, int* nseg) {
    if (!nseg || cap < 0 || (cap > 0 && !segs)) return BM_EINVAL;
    std::vector<bm_segment_t> v;
    int rc = bm::plan_segments(msg, len, lower, upper, v, max_windows);
    if (rc != BM_OK) return rc;
    *nseg = (int)v.size();
    for (int i = 0; i < cap && i < (int)v.size(); ++i) segs[i] = v[i];
    return BM_OK;
}

}  // extern "C"
