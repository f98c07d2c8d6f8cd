// bm_combine.cpp -- stage 3 of a search: the devices' (or ranks') 16-byte
// partials become one result, through one RCCL allgather or by host copies,
// and what RCCL reports about it goes into the stats.  Plain C++ over the HIP
// host API; see bm_runtime.hpp for the layout of the host runtime.
#include <algorithm>

#include "bm_runtime.hpp"

namespace bm {
namespace {

bool distinct_devices(const bm_ctx* ctx) {
    for (size_t i = 0; i < ctx->devs.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (ctx->devs[i].id == ctx->devs[j].id) return false;
    return true;
}

int ensure_nccl(bm_ctx* ctx) {
    if (ctx->nccl_ready) return BM_OK;
    // an RCCL communicator holds one rank per GPU: a device listed twice
    // (a one-GPU rehearsal of the N-device split) combines on the host
    if (!distinct_devices(ctx)) return BM_EINVAL;
    if (ctx->test_rccl_fault == 1) return BM_ERCCL;  // test hook
    const int n = (int)ctx->devs.size();
    std::vector<ncclComm_t> comms(n);
    std::vector<int> ids(n);
    for (int i = 0; i < n; ++i) ids[i] = ctx->devs[i].id;
    const auto t0 = std::chrono::steady_clock::now();
    if (ncclCommInitAll(comms.data(), n, ids.data()) != ncclSuccess) return BM_ERCCL;
    ctx->rccl_init_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < n; ++i) ctx->devs[i].comm = comms[i];
    ctx->nccl_ready = true;
    return BM_OK;
}

// Drops every communicator of the context after a failure (ncclCommAbort:
// also ends any collective of it still queued on a stream).
void abort_nccl(bm_ctx* ctx) {
    for (auto& d : ctx->devs) {
        if (!d.comm) continue;
        (void)hipSetDevice(d.id);
        (void)ncclCommAbort(d.comm);
        d.comm = nullptr;
    }
    ctx->nccl_ready = false;
    ctx->rccl_init_ms = 0.0;
}

// A non-blocking communicator's last operation: wait until it leaves
// ncclInProgress (or the deadline passes: BM_ETIMEDOUT).
int comm_settle(ncclComm_t comm, ncclResult_t r, std::chrono::steady_clock::time_point deadline, bool limited) {
    while (r == ncclInProgress) {
        if (limited && std::chrono::steady_clock::now() > deadline) return BM_ETIMEDOUT;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (ncclCommGetAsyncError(comm, &r) != ncclSuccess) return BM_ERCCL;
    }
    return r == ncclSuccess ? BM_OK : BM_ERCCL;
}

// The allgather's event pair on each device (timing on; the streams have
// been synchronised): bm_stats_t.dev_allgather_ms and their max.
void record_allgather(bm_ctx* ctx) {
    bm_stats_t& st = ctx->stats;
    for (size_t di = 0; di < ctx->devs.size() && di < (size_t)BM_MAX_STAT_DEVICES; ++di) {
        DeviceCtx& d = ctx->devs[di];
        float ms = 0.f;
        if (hipSetDevice(d.id) != hipSuccess || hipEventElapsedTime(&ms, d.ag[0], d.ag[1]) != hipSuccess) continue;
        st.dev_allgather_ms[di] = ms;
        st.rccl_allgather_ms = std::max(st.rccl_allgather_ms, (double)ms);
    }
}

Partial lex_min_slots(const Slot* s, int n) {
    Partial best{UINT64_MAX, UINT64_MAX};
    for (int i = 0; i < n; ++i) {
        const Partial& p = s[i].p;
        if (p.hash < best.hash || (p.hash == best.hash && p.nonce < best.nonce)) best = p;
    }
    return best;
}

}  // namespace

// The library's RCCL version.
int rccl_version() {
    static const int v = [] {
        int x = 0;
        return ncclGetVersion(&x) == ncclSuccess ? x : 0;
    }();
    return v;
}

// What RCCL reports about the communicator(s) a combine just ran over, into
// the stats: its rank count, and each device's rank and the HIP device RCCL
// placed it on (bm_stats_t.rccl_*).  used = false (no RCCL combine), or a
// device without a communicator: 0 ranks, -1 elsewhere.
void record_rccl(bm_ctx* ctx, bool used) {
    bm_stats_t& st = ctx->stats;
    for (int i = 0; i < BM_MAX_STAT_DEVICES; ++i) st.dev_rccl_rank[i] = st.dev_rccl_device[i] = -1;
    st.rccl_nranks = 0;
    st.rccl_rank = -1;
    for (size_t di = 0; used && di < ctx->devs.size(); ++di) {
        ncclComm_t c = ctx->devs[di].comm;
        int n = 0, r = -1, dev = -1;
        if (!c || ncclCommCount(c, &n) != ncclSuccess) continue;
        if (ncclCommUserRank(c, &r) != ncclSuccess) r = -1;
        if (ncclCommCuDevice(c, &dev) != ncclSuccess) dev = -1;
        if (di == 0) {
            st.rccl_nranks = n;
            st.rccl_rank = r;
        }
        if (di < (size_t)BM_MAX_STAT_DEVICES) {
            st.dev_rccl_rank[di] = r;
            st.dev_rccl_device[di] = dev;
        }
    }
}

// Stage 3 of a search, one process: combine the devices' partials with one
// RCCL allgather, or by host copies (BM_COMBINE_HOST, a device listed twice,
// or RCCL failing at run time: the context then aborts its communicators and
// stays on host copies, reported in the stats).  A rank context outside a
// group copies its own partial.  host_only (a target, hits or header search):
// host copies, whatever the context's combine mode.
int combine_local(bm_ctx* ctx, Partial* best_out, bool host_only) {
    bm_stats_t& st = ctx->stats;
    const int ndev = (int)ctx->devs.size();
    int nslots = ndev;
    bool via_rccl = false;
    if (!ctx->rank_ctx && !host_only) {
        const bool distinct = distinct_devices(ctx);
        if (ctx->combine == BM_COMBINE_RCCL && !distinct) return BM_EINVAL;
        const bool want = ctx->combine == BM_COMBINE_RCCL || (ctx->combine == BM_COMBINE_AUTO && ndev > 1 && distinct);
        if (want && ctx->rccl_status == 0) {
            int rc = ensure_nccl(ctx);
            if (rc == BM_OK) {
                for (int di = 0; di < ndev && rc == BM_OK; ++di) {
                    DeviceCtx& d = ctx->devs[di];
                    if (hipSetDevice(d.id) != hipSuccess ||
                        hipMemsetAsync(&d.d_slot->status, 0, 2 * sizeof(uint64_t), d.stream) != hipSuccess ||
                        (ctx->timing && hipEventRecord(d.ag[0], d.stream) != hipSuccess))
                        return BM_EHIP;
                }
                if (ctx->test_rccl_fault == 2) {
                    rc = BM_ERCCL;  // test hook: as if the grouped allgather failed
                } else if (ncclGroupStart() != ncclSuccess) {
                    rc = BM_ERCCL;
                } else {
                    for (int di = 0; di < ndev && rc == BM_OK; ++di) {
                        DeviceCtx& d = ctx->devs[di];
                        if (ncclAllGather(d.d_slot, d.d_gather, kSlotWords, ncclUint64, d.comm, d.stream) !=
                            ncclSuccess)
                            rc = BM_ERCCL;
                    }
                    if (ncclGroupEnd() != ncclSuccess) rc = BM_ERCCL;
                }
                // the allgather's span on each device: from the end of its own
                // reduction (recorded before the collective was enqueued) to the
                // collective's end, so it includes the wait for the slowest device
                for (int di = 0; di < ndev && rc == BM_OK && ctx->timing; ++di) {
                    DeviceCtx& d = ctx->devs[di];
                    if (hipSetDevice(d.id) != hipSuccess || hipEventRecord(d.ag[1], d.stream) != hipSuccess)
                        return BM_EHIP;
                }
            }
            if (rc == BM_OK) {
                DeviceCtx& d0 = ctx->devs[0];
                BM_HIP(hipSetDevice(d0.id));
                BM_HIP(hipMemcpyAsync(d0.h_slots, d0.d_gather, sizeof(Slot) * ndev, hipMemcpyDeviceToHost,
                                      d0.stream));
                via_rccl = true;
            } else if (rc == BM_ERCCL) {
                ctx->rccl_status = rc;  // fall back to host copies, now and for every later call
                abort_nccl(ctx);
            } else {
                return rc;
            }
        }
    } else if (ctx->rank_ctx) {
        nslots = 1;  // a rank outside a group: its own partial
    }
    if (!via_rccl) {
        for (int di = 0; di < ndev; ++di) {
            DeviceCtx& d = ctx->devs[di];
            BM_HIP(hipSetDevice(d.id));
            BM_HIP(hipMemcpyAsync(ctx->devs[0].h_slots + di, d.d_slot, sizeof(Partial), hipMemcpyDeviceToHost,
                                  d.stream));
        }
    }
    // the end of every device's own work (its reduction, bal[1]) seen on the
    // host: from there on the wait is the combine's (bm_stats_t.combine_ms)
    if (ctx->balance || ctx->timing)
        for (int di = 0; di < ndev; ++di) {
            BM_HIP(hipSetDevice(ctx->devs[di].id));
            BM_HIP(hipEventSynchronize(ctx->devs[di].bal[1]));
        }
    const auto t_own = std::chrono::steady_clock::now();
    for (int di = 0; di < ndev; ++di) {
        BM_HIP(hipSetDevice(ctx->devs[di].id));
        BM_HIP(hipStreamSynchronize(ctx->devs[di].stream));
    }
    st.combine_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_own).count();
    st.combine_used = ctx->rank_ctx ? BM_COMBINED_LOCAL : via_rccl ? BM_COMBINED_RCCL : BM_COMBINED_HOST;
    st.rccl_status = ctx->rccl_status;
    record_rccl(ctx, via_rccl);
    if (via_rccl && ctx->timing) record_allgather(ctx);
    *best_out = lex_min_slots(ctx->devs[0].h_slots, nslots);
    return BM_OK;
}

// Stage 3 of a search, a rank of a group: one allgather of every rank's
// slot.  A rank whose call failed before this point (own_rc) still takes
// part, with its status in the slot, so the group fails the call together
// instead of waiting for it.  The wait for the group after this rank's own
// work is bounded by peer_timeout_ms (then the communicator is aborted).
int combine_group(bm_ctx* ctx, int own_rc, Partial* best_out) {
    bm_stats_t& st = ctx->stats;
    DeviceCtx& d = ctx->devs[0];
    const int world = ctx->world;
    // Post this rank's slot.  A HIP failure while staging it becomes this
    // rank's status (it still takes part, so the group fails the call
    // together instead of waiting for it); only a slot that cannot be posted
    // at all leaves the group (abort below).
    bool posted = hipSetDevice(d.id) == hipSuccess;
    if (posted && own_rc == BM_OK &&
        hipMemsetAsync(&d.d_slot->status, 0, 2 * sizeof(uint64_t), d.stream) != hipSuccess)
        own_rc = BM_EHIP;
    if (posted && own_rc != BM_OK) {
        Slot& out = d.h_slots[d.nslots];  // pinned staging slot
        out = Slot{Partial{UINT64_MAX, UINT64_MAX}, (uint64_t)(int64_t)own_rc, 0};
        posted = hipMemcpyAsync(d.d_slot, &out, sizeof(Slot), hipMemcpyHostToDevice, d.stream) == hipSuccess;
    }
    // the end of this rank's own work, from which the peer timeout counts
    // (without the event: from the moment the allgather is enqueued)
    const bool own_mark = posted && hipEventRecord(d.own_done, d.stream) == hipSuccess;
    auto t_own = std::chrono::steady_clock::now();
    const bool limited = ctx->peer_timeout_ms > 0;
    int rc = BM_OK;
    bool copied = false;
    if (!posted) {
        rc = own_rc != BM_OK ? own_rc : BM_EHIP;
    } else if (ctx->test_rccl_fault == 2) {
        rc = BM_ERCCL;  // test hook: as if the allgather failed (world 1 only: no peer is left waiting)
    } else {
        // the allgather goes on the stream behind this rank's own work (a
        // non-blocking communicator may first report ncclInProgress: then it
        // is enqueued once the communicator settles)
        const auto timeout = std::chrono::milliseconds(ctx->peer_timeout_ms);
        const bool ag_timed = ctx->timing && hipEventRecord(d.ag[0], d.stream) == hipSuccess;
        rc = comm_settle(d.comm, ncclAllGather(d.d_slot, d.d_gather, kSlotWords, ncclUint64, d.comm, d.stream),
                         std::chrono::steady_clock::now() + timeout, limited);
        // the allgather's span on this rank's stream: from the end of its own
        // work to the end of the collective (the wait for the slowest rank included)
        if (rc == BM_OK && ag_timed) (void)hipEventRecord(d.ag[1], d.stream);
        // a failed copy of the gathered slots is this rank's own error: the
        // collective itself still runs, so the communicator stays good
        copied = rc == BM_OK && hipMemcpyAsync(d.h_slots, d.d_gather, sizeof(Slot) * world,
                                               hipMemcpyDeviceToHost, d.stream) == hipSuccess;
        // only the wait for the other ranks is bounded
        if (own_mark) (void)hipEventSynchronize(d.own_done);
        t_own = std::chrono::steady_clock::now();  // this rank's own work is done: the rest is the group's
        const auto deadline = t_own + timeout;
        if (rc == BM_OK && !limited && hipStreamSynchronize(d.stream) != hipSuccess) rc = BM_EHIP;
        for (auto pause = std::chrono::microseconds(10); rc == BM_OK && limited;) {
            const hipError_t q = hipStreamQuery(d.stream);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) {
                rc = BM_EHIP;  // the stream itself failed: the allgather's fate is unknown
                break;
            }
            if (std::chrono::steady_clock::now() > deadline) {
                rc = BM_ETIMEDOUT;
                break;
            }
            std::this_thread::sleep_for(pause);
            pause = std::min(pause * 2, std::chrono::microseconds(100));
        }
    }
    if (rc != BM_OK) {
        // the communicator cannot be trusted any more: abort it (this also
        // ends an allgather still waiting on the stream); later searches
        // return the same status until bm_ctx_leave_rank
        if (d.comm) (void)ncclCommAbort(d.comm);
        d.comm = nullptr;
        ctx->group_status = rc;
        (void)hipStreamSynchronize(d.stream);
        (void)hipGetLastError();
        st.rccl_status = rc;
        return own_rc != BM_OK ? own_rc : rc;  // this rank's own failure stays the one it reports
    }
    st.combine_used = BM_COMBINED_RCCL;
    st.combine_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_own).count();
    record_rccl(ctx, true);
    if (ctx->timing) record_allgather(ctx);
    if (!copied) return own_rc != BM_OK ? own_rc : BM_EHIP;
    // test hook: the last slot arrives carrying a peer's failure status, as
    // a real peer's would (at world 1 that slot is this rank's own)
    if (ctx->test_rccl_fault == 3) d.h_slots[world - 1].status = (uint64_t)(int64_t)BM_EHIP;
    for (int r = 0; r < world; ++r)
        if (d.h_slots[r].status != 0) return own_rc != BM_OK ? own_rc : BM_EPEER;
    if (own_rc != BM_OK) return own_rc;
    *best_out = lex_min_slots(d.h_slots, world);
    return BM_OK;
}

}  // namespace bm
