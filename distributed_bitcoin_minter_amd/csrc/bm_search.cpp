// bm_search.cpp -- the seven searches of include/btcminer.h (bm_search_gpu,
// bm_search_target_gpu, bm_search_hits_gpu, bm_search_header_gpu,
// bm_search_header_hits_gpu, bm_search_header_versions_gpu,
// bm_search_header_versions_hits_gpu) over one path, and bm_search_job_shares_gpu,
// a host loop over the last of them (job_shares_impl).  The path: plan and size every
// launch, enqueue each device's launches and its second-pass reduction,
// combine the devices' partials, read back what an enumeration appended,
// record the stats.  run_call drives that path for the six searches outside a
// rank group; what differs between them is a Mode (bm_runtime.hpp), the
// planner each *_impl passes in (plan_decimal, plan_versions, both over
// plan_devices) and what it alone does with the outcome.  bm_search_header_gpu
// and bm_search_header_hits_gpu are the one-version case of the two
// version-rolling searches: the same impl over the header's own version field,
// its answer narrowed.  search_impl runs the same stages around its group
// combine and the balance step.  Plain C++ over the HIP host API.
//
// bm_search_gpu is a drop-in for the reference miner's job loop body
// (miner.go:58-65): the same (hash, nonce) for the same (msg, range).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bm_header_versions_hits.hpp"
#include "bm_job.hpp"
#include "bm_runtime.hpp"

namespace bm {

const void* g_header_hash = nullptr;

namespace {

// search kernel table [nbv-1][P], filled by bm_inst.hip at load time; rows
// 2 + K hold the padding-block layouts (P >= 55) with their constants folded
// after K whole prefix blocks: search_kernel_padc<P> (K = 0, a one-block
// message) and search_kernel_padk<P, K> (K = 1..kMaxPadPrefixBlocks = 15)
constexpr int kSearchRows = 3 + kMaxPadPrefixBlocks;
const void* g_search[kSearchRows][64];
// target_kernel<P, NBV> and hits_kernel<P, NBV> tables [nbv-1][P]: the generic
// kernel in target / hits mode, every layout
const void* g_target[2][64];
const void* g_hits[2][64];
// header_versions_kernel<M> at [M], M = 1, 2, 4, filled by bm_header_versions_inst.hip at load time
const void* g_header_versions[kMaxVersionSlots + 1];
// header_versions_hits_kernel<M> at [M], filled by bm_header_versions_hits_inst.hip at load time
const void* g_header_versions_hits[kMaxVersionSlots + 1];

// Balance (bm_ctx_set_balance): a device's rate is measured only when its
// piece held at least this many nonces (about 20 ms of one MI355X), and the
// shares are the rates scaled so the fastest device gets kShareScale.
constexpr uint64_t kBalanceMinNonces = 1ull << 30;
constexpr double kShareScale = 65536.0;
// A device's start offset (bm_stats_t.dev_start_ms) enters its rate only
// above host jitter: at least 1 ms and 1% of its span.
constexpr double kBalanceStartMinMs = 1.0;
constexpr double kBalanceStartMinFrac = 0.01;

}  // namespace
}  // namespace bm

extern "C" void bm_register_search_kernel(int p, int nbv, const void* fn) {
    if (p >= 0 && p < 64 && nbv >= 1 && nbv <= bm::kSearchRows) bm::g_search[nbv - 1][p] = fn;
}

extern "C" void bm_register_target_kernel(int p, int nbv, const void* fn) {
    if (p >= 0 && p < 64 && nbv >= 1 && nbv <= 2) bm::g_target[nbv - 1][p] = fn;
}

extern "C" void bm_register_hits_kernel(int p, int nbv, const void* fn) {
    if (p >= 0 && p < 64 && nbv >= 1 && nbv <= 2) bm::g_hits[nbv - 1][p] = fn;
}

extern "C" void bm_register_header_hash_kernel(const void* fn) { bm::g_header_hash = fn; }

extern "C" void bm_register_header_versions_kernel(int m, const void* fn) {
    if (m >= 1 && m <= bm::kMaxVersionSlots) bm::g_header_versions[m] = fn;
}

extern "C" void bm_register_header_versions_hits_kernel(int m, const void* fn) {
    if (m >= 1 && m <= bm::kMaxVersionSlots) bm::g_header_versions_hits[m] = fn;
}

namespace bm {
namespace {

// Workgroups of fn one device holds at a time.
uint64_t resident_blocks(bm_ctx* ctx, DeviceCtx& d, const void* fn) {
    int nb = ctx->blocks_per_cu;
    for (size_t i = 0; nb <= 0 && i < d.occ.size(); ++i)
        if (d.occ[i].first == fn) nb = d.occ[i].second;
    if (nb <= 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, kBlock, 0) != hipSuccess || nb < 1) nb = 1;
        d.occ.emplace_back(fn, nb);
    }
    return (uint64_t)nb * (uint64_t)d.cus;
}

// A folded padding-block kernel applies when the segment's padding block is
// the one of a message of K whole blocks plus the varying block ending at
// byte P (bm_sha256.hpp pad_kw_const(P, K), K <= kMaxPadPrefixBlocks), and for
// K = 0 its entering state is the IV: the constants the kernel folds.
// Returns K, or -1 when the generic kernel must run.
int pad_fold_k(const bm_segment_t& s) {
    if (!s.pad_block || s.nbv != 1 || s.p < 55) return -1;
    // the only K this padding block can be: its bit length 8 * (64K + P + 1)
    const uint32_t bits = s.pad_w[15];
    if (bits % 8 != 0 || bits / 8 < (uint32_t)s.p + 1 || (bits / 8 - s.p - 1) % 64 != 0) return -1;
    const uint32_t k = (bits / 8 - s.p - 1) / 64;
    if (k > (uint32_t)kMaxPadPrefixBlocks) return -1;
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = s.pad_w[i];
    host::expand(w);
    const KW64 kw = pad_kw_const(s.p, (int)k);
    for (int t = 0; t < 64; ++t)
        if (kK256[t] + w[t] != kw.v[t]) return -1;
    if (k == 0)
        for (int q = 0; q < 8; ++q)
            if (s.mid[q] != kIV256[q]) return -1;
    return (int)k;
}

// One device's launches as its planner sizes them (size_launch,
// size_header_launch): each starts at the partial slot the one before it ended at.
struct DevicePlan {
    DeviceCtx& d;
    const int di;
    const Piece piece;  // never empty
    std::vector<Launch>& list;
    uint32_t off = 0;  // the next launch's first partial slot
    void push(Launch& L) {
        L.stat.device = di;
        off += L.stat.grid;
        list.push_back(L);
    }
};

// The launch of one segment of a decimal search (Search, Target, Hits): tasks
// of S = 10^ms nonces (ms <= digits of word LW), its grid by launch_geometry.
int size_launch(bm_ctx* ctx, DevicePlan& dp, Kind kind, const bm_segment_t& s) {
    // the folded kernel where it applies and this build registered it (an
    // A/B build may instantiate only some layouts): else the generic one,
    // which gives the same answer.  A target search and a hit enumeration
    // have generic kernels only.
    const int fk = (ctx->padc && kind == Kind::Search) ? pad_fold_k(s) : -1;
    const void* fn = fk >= 0 ? g_search[2 + fk][s.p] : nullptr;
    const bool padc = fn != nullptr;
    if (!fn) fn = (kind == Kind::Target ? g_target : kind == Kind::Hits ? g_hits : g_search)[s.nbv - 1][s.p];
    if (!fn) return BM_EINTERNAL;
    int ms = std::max(1, std::min(s.max_inner, kMaxInnerDigits));
    // word LW holds one digit: the kernel steps the next one in word LW-1
    // (bm_kernels.hpp TWOW), so a task can still be 100 nonces
    if (s.p % 4 == 0 && s.p / 4 >= 1 && s.nd >= 2) ms = 2;
    const uint64_t resident = resident_blocks(ctx, dp.d, fn);
    if (ctx->task_digits > 0) {
        ms = std::min(ms, ctx->task_digits);
    } else if (ms > 1) {
        // A launch with fewer 100-nonce tasks than twice its resident lanes
        // (the 1..8-digit segments of a search from 0) leaves SIMDs half
        // empty while each lane runs its one 100-nonce task: use 10-nonce
        // tasks instead, so every lane has work and the launch ends sooner.
        const uint64_t lanes = resident * (uint64_t)kBlock;
        const uint64_t tasks100 = (s.vhi - s.vlo) / 100 + 1;
        if (tasks100 < 2 * lanes) ms = 1;
    }
    const uint64_t S = kPow10[ms];
    const uint64_t t0 = s.vlo / S, t_end = s.vhi / S + 1;
    const LaunchGeometry g = launch_geometry(t_end - t0, S, ctx->lane_chunk, resident, kBlock);

    Launch L;
    std::memset(&L, 0, sizeof L);
    SearchArgs& A = L.args.search;
    std::memcpy(A.mid, s.mid, sizeof A.mid);
    std::memcpy(A.tmpl, s.tmpl, sizeof A.tmpl);
    if (s.pad_block) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i) w[i] = s.pad_w[i];
        host::expand(w);
        for (int i = 0; i < 64; ++i) A.padkw[i] = kK256[i] + w[i];
    }
    A.vlo = s.vlo;
    A.vhi = s.vhi;
    A.nonce_base = s.nonce_base;
    A.t0 = t0;
    A.t_end = t_end;
    A.chunk_m = g.chunk_m;
    A.S = (uint32_t)S;
    A.ms = (uint32_t)ms;
    A.nd = (uint32_t)s.nd;
    A.part_off = dp.off;
    L.fn = fn;
    L.first_nonce = s.nonce_base + s.vlo;
    L.tasks = t_end - t0;
    L.task_nonces = S;
    L.stat.p = s.p;
    L.stat.nbv = s.nbv;
    L.stat.pad_block = padc ? 2 + fk : s.pad_block;
    L.stat.digits = s.digits;
    L.stat.inner_digits = ms;
    L.stat.nonces = s.vhi - s.vlo + 1;
    L.stat.grid = g.grid;
    L.stat.tasks_per_thread = (uint32_t)g.tasks_per_thread;
    dp.push(L);
    return BM_OK;
}

// One device's launch of a block-header kernel: its piece of the nonce range in
// tasks of 256 nonces, of m hashes each (base: the terms of one group of m
// versions, which the kernel runs in lock-step).
int size_header_launch(bm_ctx* ctx, DevicePlan& dp, Kind kind, const HeaderVersionsArgs<kMaxVersionSlots>& base,
                       int m) {
    const void* fn = (kind == Kind::HeaderVersionsHits ? g_header_versions_hits : g_header_versions)[m];
    if (!fn) return BM_EINTERNAL;
    const uint32_t lo = (uint32_t)dp.piece.lo, hi = (uint32_t)dp.piece.hi;
    Launch L;
    std::memset(&L, 0, sizeof L);
    HeaderVersionsArgs<kMaxVersionSlots>& A = L.args.versions;
    A = base;
    A.lo = lo;
    A.hi = hi;
    A.t0 = lo >> kHeaderTaskBits;
    A.ntask = (hi >> kHeaderTaskBits) - A.t0 + 1;
    const LaunchGeometry g = launch_geometry(A.ntask, kHeaderTaskNonces, ctx->lane_chunk,
                                             resident_blocks(ctx, dp.d, fn), kBlock);
    A.chunk_m = g.chunk_m;
    A.part_off = dp.off;
    L.fn = fn;
    L.first_nonce = lo;
    L.tasks = A.ntask;
    L.task_nonces = (uint64_t)kHeaderTaskNonces * (uint64_t)m;  // (nonce, version) pairs
    L.stat.nbv = m;
    L.stat.nonces = ((uint64_t)hi - lo + 1) * (uint64_t)m;
    L.stat.grid = g.grid;
    L.stat.tasks_per_thread = (uint32_t)g.tasks_per_thread;
    dp.push(L);
    return BM_OK;
}

// This process's piece of [lower, upper] (rank contexts: every rank passes the
// same range and scans its contiguous share of it), split over the devices
// (the partitioner: slot_pieces over ctx->shares; an empty piece has lo > hi).
std::vector<Piece> plan_pieces(bm_ctx* ctx, uint64_t lower, uint64_t upper) {
    const int ndev = (int)ctx->devs.size();
    uint64_t lo = lower, hi = upper;
    bool have = true;
    if (ctx->rank_ctx) {
        const Piece mine = slot_pieces(lower, upper, ctx->world, ctx->shares)[(size_t)ctx->rank];
        lo = mine.lo;
        hi = mine.hi;
        have = lo <= hi;  // else a range shorter than the group (or a tiny share): nothing here
    }
    if (have) ctx->stats.nonces = hi - lo + 1;  // wraps to 0 only for the full 2^64 range
    std::vector<Piece> pieces =
        slot_pieces(have ? lo : 1, have ? hi : 0, ndev, ctx->rank_ctx ? std::vector<uint32_t>() : ctx->shares);
    for (int di = 0; di < ndev; ++di)
        ctx->devs[di].piece_nonces = pieces[di].lo <= pieces[di].hi ? pieces[di].hi - pieces[di].lo + 1 : 0;
    return pieces;
}

// Room on the (current) device for what its launches write.
int ensure_buffers(DeviceCtx& d, const Mode& mode, const std::vector<Launch>& launches) {
    size_t parts = 0;
    for (const Launch& L : launches) parts += L.stat.grid;
    BM_TRY(grow(d, d.d_part, d.part_cap, std::max(parts, kMinPartials)));
    BM_TRY(ensure_counters(d, launches.size()));
    if (!mode.every_hit()) return BM_OK;
    return grow(d, d.d_hbuf, d.hbuf_cap, std::max<size_t>(mode.cap, 1), sizeof(Partial), false, BM_ENOMEM);
}

// Stage 1 of every search: the range cut into the devices' pieces, and for each
// device with a piece, with that device current, its launches as
// per_device(DevicePlan&) sizes them and the room for what they write.
template <class PerDevice>
int plan_devices(bm_ctx* ctx, const Mode& mode, uint64_t lower, uint64_t upper,
                 std::vector<std::vector<Launch>>& launches, PerDevice&& per_device) {
    const std::vector<Piece> pieces = plan_pieces(ctx, lower, upper);
    for (size_t di = 0; di < pieces.size(); ++di) {
        if (pieces[di].lo > pieces[di].hi) continue;
        DevicePlan dp{ctx->devs[di], (int)di, pieces[di], launches[di]};
        BM_HIP(hipSetDevice(dp.d.id));
        BM_TRY(per_device(dp));
        BM_TRY(ensure_buffers(dp.d, mode, launches[di]));
    }
    return BM_OK;
}

// A decimal search (Search, Target, Hits): one launch per segment of the
// device's piece.
int plan_decimal(bm_ctx* ctx, const Mode& mode, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                 std::vector<std::vector<Launch>>& launches) {
    return plan_devices(ctx, mode, lower, upper, launches, [&](DevicePlan& dp) -> int {
        std::vector<bm_segment_t> segs;
        BM_TRY(plan_segments(msg, len, dp.piece.lo, dp.piece.hi, segs, ctx->max_windows));
        // With streams to overlap on, the biggest segment's last tail_nonces
        // become a launch of their own: it is small enough for 10-nonce tasks
        // (size_launch), so the call ends on a short drain instead of half a
        // 100-nonce task.
        if (ctx->streams > 1 && ctx->tail_nonces > 0 && !segs.empty()) {
            size_t big = 0;
            for (size_t i = 1; i < segs.size(); ++i)
                if (segs[i].vhi - segs[i].vlo > segs[big].vhi - segs[big].vlo) big = i;
            bm_segment_t& b = segs[big];
            if ((b.vhi - b.vlo) / 8 >= ctx->tail_nonces) {
                bm_segment_t t = b;
                t.vlo = b.vhi - ctx->tail_nonces + 1;
                b.vhi = t.vlo - 1;
                segs.push_back(t);
            }
        }
        for (const bm_segment_t& seg : segs) BM_TRY(size_launch(ctx, dp, mode.kind, seg));
        return BM_OK;
    });
}

// A block-header search or enumeration (HeaderVersions, HeaderVersionsHits):
// every device gets one launch per group of versions over its piece of the
// nonce range, in group order (they all start at the piece's first nonce, so
// enqueue_device keeps that order).
int plan_versions(bm_ctx* ctx, const Mode& mode, const uint8_t* header, const uint32_t* versions, size_t nver,
                  const uint8_t* target, uint32_t lo, uint32_t hi, std::vector<std::vector<Launch>>& launches) {
    uint8_t sizes[BM_MAX_HEADER_VERSIONS];
    const int ngroups = host::versions_groups(nver, ctx->header_group, sizes);
    std::vector<HeaderVersionsArgs<kMaxVersionSlots>> groups((size_t)ngroups);
    size_t at = 0;
    for (int g = 0; g < ngroups; ++g) {
        std::memset(&groups[g], 0, sizeof groups[g]);
        // the shared schedule terms do not depend on the version: a kernel may share them
        if (!host::header_versions_precompute(header, versions, at, sizes[g], groups[g])) return BM_EINTERNAL;
        for (int i = 0; i < 8; ++i) groups[g].tgt[i] = host::load_be32(target + 4 * i);
        at += sizes[g];
    }
    BM_TRY(plan_devices(ctx, mode, lo, hi, launches, [&](DevicePlan& dp) -> int {
        for (int g = 0; g < ngroups; ++g) BM_TRY(size_header_launch(ctx, dp, mode.kind, groups[g], sizes[g]));
        return BM_OK;
    }));
    ctx->stats.nonces *= nver;  // pairs
    return BM_OK;
}

// Waits for everything a call may have queued on any stream of the context.
// Used when a call fails part-way: launches already on the aux streams keep
// running against d_ctr / d_part, so the next call (whose counter memset is
// ordered only on the main stream) must not start before they end.
void drain(bm_ctx* ctx) {
    for (auto& d : ctx->devs) {
        if (hipSetDevice(d.id) != hipSuccess) continue;
        for (hipStream_t s : d.streams) (void)hipStreamSynchronize(s);
    }
    (void)hipGetLastError();
}

// Stage 2, one device: its launches, its second-pass reduction (its partial
// lands in d_slot) and the copies of what the mode reads back.  `enqueued`
// counts launches over every device (the test fault).  On failure the caller drains.
int enqueue_device(bm_ctx* ctx, int di, const Mode& mode, std::vector<Launch>& launches, uint32_t& first,
                   std::atomic<int>& enqueued) {
    DeviceCtx& d = ctx->devs[di];
    const bool mark = ctx->balance || ctx->timing;  // per-device span events
    const size_t strip_bytes = launches.size() * kCtrStride * sizeof(unsigned long long);
    BM_HIP(hipSetDevice(d.id));
    if (d.test_delay_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(d.test_delay_us));
    // the call's first op on this device: its stream is idle, so it starts
    // about when it is submitted (the common start of bm_stats_t.dev_start_ms)
    if (mark) BM_HIP(hipEventRecord(d.bal[0], d.stream));
    d.submitted = std::chrono::steady_clock::now();
    if (!launches.empty()) BM_HIP(hipMemsetAsync(d.d_ctr, 0, strip_bytes, d.stream));
    if (mode.first_hit()) {
        *d.h_hit = ~0ull;
        BM_HIP(hipMemsetAsync(d.d_hit, 0xFF, sizeof(unsigned long long), d.stream));
    }
    if (mode.every_hit()) {
        *d.h_hcount = 0;
        BM_HIP(hipMemsetAsync(d.d_hcount, 0, sizeof(unsigned long long), d.stream));
    }
    // The order of the launches, round-robin over the streams.  First hit
    // wins: lowest nonces first, so that a hit cancels what lies above it.
    // Else, with streams to overlap on: biggest first.
    const int ns = std::max(1, std::min<int>(ctx->streams, (int)launches.size()));
    std::vector<uint32_t> order(launches.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    if (mode.first_hit())
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t x, uint32_t y) { return launches[x].first_nonce < launches[y].first_nonce; });
    else if (ns > 1)
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t x, uint32_t y) { return launches[x].stat.nonces > launches[y].stat.nonces; });
    if (ns > 1) {
        BM_HIP(hipEventRecord(d.fork, d.stream));
        for (int k = 0; k + 1 < ns; ++k) BM_HIP(hipStreamWaitEvent(d.aux[k], d.fork, 0));
    }
    if (!order.empty()) first = order[0];
    uint32_t nparts = 0;
    for (uint32_t r = 0; r < order.size(); ++r) {
        const uint32_t li = order[r];
        Launch& L = launches[li];
        hipStream_t s = (r % ns) == 0 ? d.stream : d.aux[r % ns - 1];
        if (ctx->fault_after >= 0 && enqueued.fetch_add(1) >= ctx->fault_after) return BM_EINTERNAL;  // test hook
        const bool timed = ctx->timing && li < (uint32_t)kEventPairs;
        if (timed) BM_HIP(hipEventRecord(d.ev[2 * li], s));
        unsigned long long* ctr = d.d_ctr + kCtrStride * li;
        uint64_t target = mode.target, cap = mode.cap;
        // the kernel's parameters: the launch's own, then what the mode adds
        void* params[7] = {&L.args, &d.d_part, &ctr};
        int np = 3;
        if (mode.target64()) params[np++] = &target;
        if (mode.first_hit()) params[np++] = &d.d_hit;
        if (mode.every_hit()) {
            params[np++] = &d.d_hcount;
            params[np++] = &d.d_hbuf;
            params[np++] = &cap;
        }
        BM_HIP(hipLaunchKernel(L.fn, dim3(L.stat.grid), dim3(kBlock), params, 0, s));
        if (timed) BM_HIP(hipEventRecord(d.ev[2 * li + 1], s));
        nparts += L.stat.grid;
    }
    for (int k = 0; k + 1 < ns; ++k) {
        BM_HIP(hipEventRecord(d.join[k], d.aux[k]));
        BM_HIP(hipStreamWaitEvent(d.stream, d.join[k], 0));
    }
    // nparts = 0 (a device or rank with nothing to scan) writes (2^64-1, 2^64-1)
    BM_TRY(launch_reduce_partials(d.d_part, nparts, &d.d_slot->p, d.stream));
    if (mark) BM_HIP(hipEventRecord(d.bal[1], d.stream));
    if (mode.first_hit())
        BM_HIP(hipMemcpyAsync(d.h_hit, d.d_hit, sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    if (mode.every_hit())
        BM_HIP(hipMemcpyAsync(d.h_hcount, d.d_hcount, sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    // the strips: clock stamps, for the launch stats; first hit wins: the dequeue counters
    if (((BM_CLOCK_PROBE && ctx->timing) || mode.first_hit()) && !launches.empty())
        BM_HIP(hipMemcpyAsync(d.h_ctr, d.d_ctr, strip_bytes, hipMemcpyDeviceToHost, d.stream));
    return BM_OK;
}

// Stage 2 of a search: every device's work.  A context of several devices
// submits each device's work from a host thread of its own (the context's
// SubmitPool, kept across searches since round 6), so device N-1 does not
// wait for the other devices' ~15 API calls each before it starts (the start
// skew of a serial submission; bm_stats_t.dev_start_ms reports what is left
// of it).  Each thread touches its own DeviceCtx only, and `enqueued`.
int enqueue(bm_ctx* ctx, const Mode& mode, std::vector<std::vector<Launch>>& launches,
            std::vector<uint32_t>& first) {
    const int ndev = (int)ctx->devs.size();
    if (ctx->fault_after == 0) return BM_EINTERNAL;  // test hook (also for a rank with nothing to scan)
    std::atomic<int> enqueued{0};
    ctx->stats.start_threads = 1;
    auto one = [&](int di) {
        return guarded([&] { return enqueue_device(ctx, di, mode, launches[di], first[di], enqueued); });
    };
    if (ndev == 1) return one(0);
    std::vector<int> rc(ndev, BM_OK);
    const std::function<void(int)> job = [&](int di) { rc[di] = one(di); };
    bool pooled = false;
    try {
        pooled = ctx->submit.run(ndev, job);
    } catch (...) {  // std::function or the pool's own bookkeeping: submit serially
        pooled = false;
    }
    if (!pooled)  // no threads: this one submits every device's work itself
        for (int di = 0; di < ndev; ++di) rc[di] = one(di);
    ctx->stats.start_threads = pooled ? 1 + ctx->submit.threads() : 1;
    for (int r : rc)
        if (r != BM_OK) return r;
    return BM_OK;
}

// The RCCL figures every call reports, whatever its outcome: the library's
// RCCL version and, while the context holds a communicator, the time it took
// to form.
void stamp_common(bm_ctx* ctx) {
    bm_stats_t& st = ctx->stats;
    st.rccl_version = rccl_version();
    const bool have = ctx->rank_ctx ? ctx->joined && ctx->devs[0].comm != nullptr : ctx->nccl_ready;
    st.rccl_init_ms = have ? ctx->rccl_init_ms : 0.0;
    if (st.start_threads == 0) st.start_threads = 1;
}

// Every search starts here: the last call's stats go, and a first-hit search
// (and only that) also resets the target stats.
void begin_call(bm_ctx* ctx, const Mode& mode) {
    std::memset(&ctx->stats, 0, sizeof ctx->stats);
    if (mode.first_hit()) std::memset(&ctx->tstats, 0, sizeof ctx->tstats);
    record_rccl(ctx, false);
    stamp_common(ctx);  // (what a call that ends at once, on an empty range, reports)
}

// ... and a search that fails ends here: what it queued is waited for, and the
// stats keep the common figures only (and a joined rank's failed communicator).
int fail_call(bm_ctx* ctx, int rc, int rccl_status = 0) {
    drain(ctx);
    std::memset(&ctx->stats, 0, sizeof ctx->stats);
    record_rccl(ctx, false);
    ctx->stats.rccl_status = rccl_status;
    stamp_common(ctx);
    return rc;
}

// Each device's start against the earliest device's (host submission times).
std::vector<double> start_offsets(bm_ctx* ctx) {
    const int ndev = (int)ctx->devs.size();
    std::vector<double> start_ms(ndev, 0.0);
    auto t0 = ctx->devs[0].submitted;
    for (const auto& d : ctx->devs) t0 = std::min(t0, d.submitted);
    for (int di = 0; di < ndev; ++di)
        start_ms[di] = std::chrono::duration<double, std::milli>(ctx->devs[di].submitted - t0).count();
    return start_ms;
}

// The statistics of a finished call: devices, launch list, event timings,
// wall time.
int record_stats(bm_ctx* ctx, std::vector<std::vector<Launch>>& launches, const std::vector<uint32_t>& first,
                 const std::vector<double>& start_ms, std::chrono::steady_clock::time_point t_start) {
    bm_stats_t& st = ctx->stats;
    const int ndev = (int)ctx->devs.size();
    st.devices = (uint32_t)std::min(ndev, BM_MAX_STAT_DEVICES);
    for (int di = 0; di < ndev; ++di) {
        DeviceCtx& d = ctx->devs[di];
        if (di < BM_MAX_STAT_DEVICES) {
            st.dev_nonces[di] = d.piece_nonces;
            if (ctx->timing || ctx->balance) st.dev_start_ms[di] = start_ms[di];
            float ms = 0.f;
            if ((ctx->timing || ctx->balance) && hipSetDevice(d.id) == hipSuccess &&
                hipEventElapsedTime(&ms, d.bal[0], d.bal[1]) == hipSuccess)
                st.dev_span_ms[di] = ms;
        }
        uint32_t li = 0;
        const bool span_ok = ctx->timing && !launches[di].empty() && first[di] < (uint32_t)kEventPairs;
        for (Launch& L : launches[di]) {
            ++st.launches;
            if (ctx->timing && li < (uint32_t)kEventPairs) {
                float ms = 0.f;
                BM_HIP(hipEventElapsedTime(&ms, d.ev[2 * li], d.ev[2 * li + 1]));
                L.stat.ms = ms;
                st.kernel_ms += ms;
                const unsigned long long* c = d.h_ctr + kCtrStride * li + kCtrClockSlot - 1;
                if (BM_CLOCK_PROBE && c[4] > c[2] && c[3] > c[1])  // shader cycles over constant-rate ticks
                    L.stat.clock_ghz = (double)(c[3] - c[1]) / ((double)(c[4] - c[2]) / d.wall_clock_hz) / 1e9;
                if (span_ok) {  // the first launch's start to this launch's end
                    float sp = 0.f;
                    BM_HIP(hipEventElapsedTime(&sp, d.ev[2 * first[di]], d.ev[2 * li + 1]));
                    st.span_ms = std::max(st.span_ms, (double)sp);
                }
            }
            if (st.recorded < BM_MAX_LAUNCH_STATS) st.launch[st.recorded++] = L.stat;
            ++li;
        }
    }
    stamp_common(ctx);
    st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return BM_OK;
}

// After a first-hit search: the hit of the lowest device that has one (pieces
// ascend with the device index; UINT64_MAX: none), and into the target stats
// the nonces each device's launches took off their work counters.
uint64_t scan_hit_words(bm_ctx* ctx, const std::vector<std::vector<Launch>>& launches) {
    bm_target_stats_t& ts = ctx->tstats;
    const int ndev = (int)ctx->devs.size();
    uint64_t hit = UINT64_MAX;
    ts.devices = (uint32_t)std::min(ndev, BM_MAX_STAT_DEVICES);
    for (int di = 0; di < ndev; ++di) {
        const DeviceCtx& d = ctx->devs[di];
        if (launches[di].empty()) continue;
        if (hit == UINT64_MAX) hit = *d.h_hit;
        uint64_t disp = 0;
        for (size_t li = 0; li < launches[di].size(); ++li) {
            const Launch& L = launches[di][li];
            const uint64_t tasks = std::min<uint64_t>(d.h_ctr[kCtrStride * li], L.tasks);
            disp += std::min<uint64_t>(tasks * L.task_nonces, L.stat.nonces);
        }
        if (di < BM_MAX_STAT_DEVICES) ts.dev_dispatched[di] = disp;
        ts.nonces_dispatched += disp;
    }
    return hit;
}

// What the shared path of a call hands back to its *_impl.
struct Call {
    bool empty = false;                         // the range was: nothing ran, the impl's empty-range answer stands
    std::vector<std::vector<Launch>> launches;  // per device
    std::vector<uint32_t> first;                // per device: the launch that went out first
    Partial best{UINT64_MAX, UINT64_MAX};       // the minimum of the devices' partials
    // an every_hit mode: what the devices counted, and their entries (device 0's
    // counts[0], then device 1's counts[1], ...) when there are any and they fit in cap
    uint64_t count = 0;
    std::vector<size_t> counts;
    std::vector<Partial> entries;
};

// Stage 4 of an enumeration, after the combine has waited for every device's
// copies: the counters, and the entries only when their sum fits in cap.
// max_per_nonce: what one nonce of a device's piece can add to its counter at
// most (an entry counts once); 0: no such bound.
int read_back_hits(bm_ctx* ctx, const Mode& mode, uint64_t max_per_nonce, Call& c) {
    const int ndev = (int)ctx->devs.size();
    c.counts.assign(ndev, 0);
    for (int di = 0; di < ndev; ++di) {
        if (c.launches[di].empty()) continue;
        const uint64_t n = *ctx->devs[di].h_hcount;
        if (max_per_nonce && n > ctx->devs[di].piece_nonces * max_per_nonce) return BM_EINTERNAL;
        c.counts[di] = (size_t)n;
        c.count += n;
    }
    if (c.count > mode.cap || c.count == 0) return BM_OK;
    c.entries.resize((size_t)c.count);
    size_t at = 0;
    for (int di = 0; di < ndev; ++di) {
        DeviceCtx& d = ctx->devs[di];
        if (c.counts[di] == 0) continue;
        BM_HIP(hipSetDevice(d.id));
        BM_HIP(hipMemcpyAsync(c.entries.data() + at, d.d_hbuf, c.counts[di] * sizeof(Partial), hipMemcpyDeviceToHost,
                              d.stream));
        BM_HIP(hipStreamSynchronize(d.stream));
        at += c.counts[di];
    }
    return BM_OK;
}

// A call outside a rank group, start to end: the last call's stats go
// (begin_call), plan(launches) plans and sizes every launch, enqueue, the host
// combine (which also waits for every device's copies), an enumeration's
// read-back and settle(), the stats.  settle is what an enumeration does with
// its entries (sort, rehash, check): bm_stats_t.wall_ms has always covered
// that, while a first-hit call's one rehash comes after the stats, in its
// *_impl.  Any failure ends in fail_call.
template <class Plan, class Settle>
int run_call(bm_ctx* ctx, const Mode& mode, bool empty, Call& c, Plan&& plan, uint64_t max_per_nonce,
             Settle&& settle) {
    const auto t_start = std::chrono::steady_clock::now();
    begin_call(ctx, mode);
    c.empty = empty;
    if (empty) return BM_OK;
    const int ndev = (int)ctx->devs.size();
    c.launches.resize(ndev);
    c.first.assign(ndev, 0);
    int rc = guarded([&] { return plan(c.launches); });
    if (rc == BM_OK) rc = enqueue(ctx, mode, c.launches, c.first);
    if (rc == BM_OK) rc = combine_local(ctx, &c.best, true);
    if (rc == BM_OK && mode.every_hit()) rc = guarded([&] { return read_back_hits(ctx, mode, max_per_nonce, c); });
    if (rc == BM_OK) rc = guarded([&] { return settle(); });
    if (rc == BM_OK) rc = record_stats(ctx, c.launches, c.first, start_offsets(ctx), t_start);
    return rc == BM_OK ? BM_OK : fail_call(ctx, rc);
}
template <class Plan>
int run_call(bm_ctx* ctx, const Mode& mode, bool empty, Call& c, Plan&& plan) {  // a first-hit call
    return run_call(ctx, mode, empty, c, plan, 0, [] { return BM_OK; });
}

int search_impl(bm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, bm_result_t* out) {
    const auto t_start = std::chrono::steady_clock::now();
    const Mode mode{Kind::Search};
    begin_call(ctx, mode);
    const int ndev = (int)ctx->devs.size();
    const bool group = ctx->rank_ctx && ctx->joined;
    // the communicator failed earlier: leave the group first
    if (group && ctx->group_status != BM_OK) return fail_call(ctx, ctx->group_status, ctx->group_status);
    if (lower > upper) {  // miner.go:45-46 with zero iterations (every rank sees the same range)
        out->hash = UINT64_MAX;
        out->nonce = UINT64_MAX;
        return BM_OK;
    }

    // 1-2. plan and size every launch; enqueue them and each device's
    // second-pass reduction.  A failure part-way drains every stream first,
    // so the context stays usable.
    std::vector<std::vector<Launch>> launches(ndev);
    std::vector<uint32_t> first(ndev, 0);
    int rc = guarded([&] { return plan_decimal(ctx, mode, msg, len, lower, upper, launches); });
    if (rc == BM_OK) rc = enqueue(ctx, mode, launches, first);
    if (rc != BM_OK) drain(ctx);

    // 3. combine (a rank of a group takes part even after a failure, and its
    // failed communicator's status survives in the stats)
    Partial best{UINT64_MAX, UINT64_MAX};
    if (group)
        rc = combine_group(ctx, rc, &best);
    else if (rc == BM_OK)
        rc = combine_local(ctx, &best, false);
    if (rc != BM_OK) return fail_call(ctx, rc, group ? ctx->stats.rccl_status : 0);

    const std::vector<double> start_ms = start_offsets(ctx);

    // 4. balance: the next call's shares follow each device's measured rate,
    // its nonces over the time from the call's common start to its reduction,
    // so a device that starts late gets a smaller piece
    if (ctx->balance && ndev > 1) {
        std::vector<double> rate(ndev, 0.0);
        bool ok = true;
        for (int di = 0; di < ndev && ok; ++di) {
            DeviceCtx& d = ctx->devs[di];
            float ms = 0.f;
            ok = d.piece_nonces >= kBalanceMinNonces && hipSetDevice(d.id) == hipSuccess &&
                 hipEventElapsedTime(&ms, d.bal[0], d.bal[1]) == hipSuccess && ms > 0.f;
            // a start offset counts only when it is more than host jitter
            // (thread scheduling: sub-ms to ms on a loaded host), so shares
            // move only for a persistent late start
            const double late = start_ms[di] >= std::max(kBalanceStartMinMs, kBalanceStartMinFrac * ms) ? start_ms[di]
                                                                                                          : 0.0;
            if (ok) rate[di] = (double)d.piece_nonces / (late + ms);
        }
        if (ok) {
            const double top = *std::max_element(rate.begin(), rate.end());
            ctx->shares.assign(ndev, 1);
            for (int di = 0; di < ndev; ++di)
                ctx->shares[di] = (uint32_t)std::max(1.0, std::floor(rate[di] / top * kShareScale + 0.5));
        }
    }

    // 5. statistics
    rc = record_stats(ctx, launches, first, start_ms, t_start);
    if (rc != BM_OK) return rc;
    out->hash = best.hash;
    out->nonce = best.nonce;
    return BM_OK;
}

// bitcoin.Hash(msg, nonce) on the host (hash.go:11-15: the first 8 bytes,
// big-endian, of SHA-256("msg nonce")), with the compression the planner
// uses for midstates: once per found target, never per nonce.
uint64_t host_hash(const uint8_t* msg, size_t len, uint64_t nonce) {
    char dec[24];
    const int nd = std::snprintf(dec, sizeof dec, "%llu", (unsigned long long)nonce);
    const uint64_t total = (uint64_t)len + 1 + (uint64_t)nd;
    auto byte_at = [&](uint64_t pos) -> uint8_t {
        if (pos < len) return msg[pos];
        if (pos == len) return (uint8_t)' ';
        if (pos < total) return (uint8_t)dec[pos - len - 1];
        return pos == total ? 0x80 : 0;
    };
    const uint64_t blocks = (total + 1 + 8 + 63) / 64;  // data, the 0x80 byte, the 64-bit length
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = kIV256[i];
    uint8_t blk[64];
    for (uint64_t b = 0; b < blocks; ++b) {
        for (int i = 0; i < 64; ++i) blk[i] = byte_at(b * 64 + (uint64_t)i);
        if (b + 1 == blocks)
            for (int i = 0; i < 8; ++i) blk[56 + i] = (uint8_t)((total * 8) >> (8 * (7 - i)));
        host::compress_bytes(st, blk);
    }
    return ((uint64_t)st[0] << 32) | st[1];
}

// bm_search_target_gpu: each device scans its piece in ascending launch order
// with a hit word of its own; the host takes the lowest-nonce hit, or the
// lexicographic min of the partials when there is none.
int target_impl(bm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                bm_target_result_t* out) {
    const Mode mode{Kind::Target, target};
    *out = bm_target_result_t{UINT64_MAX, UINT64_MAX, 0, 0};
    Call c;
    const int rc = run_call(ctx, mode, lower > upper, c, [&](auto& launches) {
        return plan_decimal(ctx, mode, msg, len, lower, upper, launches);
    });
    if (rc != BM_OK || c.empty) return rc;

    uint64_t hit = scan_hit_words(ctx, c.launches);
    bool found = hit != UINT64_MAX;
    // the nonce 2^64-1 cannot be told from "none" in the hit word: it is the
    // answer exactly when nothing below it hit and its own hash meets the target
    if (!found && upper == UINT64_MAX && host_hash(msg, len, UINT64_MAX) <= target) found = true;
    if (found)
        *out = bm_target_result_t{host_hash(msg, len, hit), hit, 1, 0};
    else
        *out = bm_target_result_t{c.best.hash, c.best.nonce, 0, 0};
    return BM_OK;
}

// bm_search_hits_gpu: a full scan in a search's launch order.  Each device
// appends its hits to a buffer of its own in whatever order its lanes took
// their slots; the host reads every counter back, and only when their sum
// fits in cap the entries, sorted by nonce per device and concatenated in
// device order (pieces ascend with the device index).  hits and out are
// written last, on success only.
int hits_impl(bm_ctx* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
              bm_result_t* hits, size_t cap, bm_hits_result_t* out) {
    const Mode mode{Kind::Hits, target, (uint64_t)cap};
    *out = bm_hits_result_t{UINT64_MAX, UINT64_MAX, 0, 0};
    Call c;
    const int rc = run_call(ctx, mode, lower > upper, c, [&](auto& launches) {
        return plan_decimal(ctx, mode, msg, len, lower, upper, launches);
    }, 0 /* no bound on a device's count */, [&] {
        auto at = c.entries.begin();
        for (size_t n : c.counts) {
            if (c.entries.empty()) break;  // none, or more than cap
            std::sort(at, at + n, [](const Partial& a, const Partial& b) { return a.nonce < b.nonce; });
            at += n;
        }
        return BM_OK;
    });
    if (rc != BM_OK || c.empty) return rc;

    static_assert(sizeof(bm_result_t) == sizeof(Partial), "hit entry layout");
    if (!c.entries.empty()) std::memcpy(hits, c.entries.data(), c.entries.size() * sizeof(Partial));
    *out = bm_hits_result_t{c.best.hash, c.best.nonce, c.count, c.entries.size()};
    return BM_OK;
}

// bm_search_header_versions_gpu, and bm_search_header_gpu with the header's own
// version as the whole list: the nonce range cut over the devices by the
// partitioner.  Every device scans its piece once per group of versions; its
// hit word holds the smallest (nonce, version index) key of all its launches.
// The host takes the lowest device's hit (pieces ascend with the device
// index), or else the minimum of the (top 64 bits, key) partials, recomputes
// the full 256-bit hash of the one pair it returns and checks the device's
// claim against it (header_versions_select).
int header_versions_impl(bm_ctx* ctx, const uint8_t* header, const uint32_t* versions, size_t nver, uint32_t lo,
                         uint32_t hi, const uint8_t* target, bm_header_versions_result_t* out) {
    const Mode mode{Kind::HeaderVersions};
    std::memset(out, 0, sizeof *out);
    std::memset(out->hash, 0xFF, sizeof out->hash);
    out->nonce = 0xFFFFFFFFu;
    out->version = versions[0];
    Call c;
    int rc = run_call(ctx, mode, lo > hi, c, [&](auto& launches) {
        return plan_versions(ctx, mode, header, versions, nver, target, lo, hi, launches);
    });
    if (rc != BM_OK || c.empty) return rc;

    const uint64_t hit = scan_hit_words(ctx, c.launches);
    bm_header_versions_result_t r;
    rc = host::header_versions_select(header, versions, nver, target, hit, c.best, &r);
    if (rc != BM_OK) return fail_call(ctx, rc);
    *out = r;
    return BM_OK;
}

// bm_search_header_versions_hits_gpu, and bm_search_header_hits_gpu with the
// header's own version as the whole list (Hit: the caller's entry type,
// bm_header_version_hit_t or bm_header_hit_t): a full scan over
// header_versions_impl's launches (one per device and group of versions, over
// the partitioner's pieces) in hits mode.  All of a device's launches append
// {top 64 bits, (nonce << 32) | version index} to d_hbuf through d_hcount (what
// bm_search_hits_gpu uses, with the same 16-byte entries), zeroed once before
// the device's first launch; the host reads every counter back and, only when
// their sum fits in cap, the entries, which header_versions_hits_collect sorts
// by (nonce, index), rehashes in full and checks.  The best share is
// header_versions_impl's found = 0 answer.  hits and out are written last, on
// success only.
template <class Hit>
int header_versions_hits_impl(bm_ctx* ctx, const uint8_t* header, const uint32_t* versions, size_t nver,
                              uint32_t lo, uint32_t hi, const uint8_t* target, Hit* hits, size_t cap,
                              bm_header_versions_hits_result_t* out) {
    const Mode mode{Kind::HeaderVersionsHits, 0, (uint64_t)cap};
    bm_header_versions_hits_result_t r;
    std::memset(&r, 0, sizeof r);
    std::memset(r.hash, 0xFF, sizeof r.hash);
    r.nonce = 0xFFFFFFFFu;
    r.version = versions[0];
    *out = r;
    std::vector<Hit> list;
    Call c;
    const int rc = run_call(ctx, mode, lo > hi, c, [&](auto& launches) {
        return plan_versions(ctx, mode, header, versions, nver, target, lo, hi, launches);
    }, nver /* a pair counts once */, [&]() -> int {
        list.resize(c.entries.size());
        if (!list.empty())
            BM_TRY(host::header_versions_hits_collect(header, versions, nver, target, lo, hi, c.entries.data(),
                                                      c.counts.data(), (int)c.counts.size(), list.data()));
        // the best share: the device's claim against the host's hash of that pair, and against the count
        return host::header_versions_hits_best(header, versions, nver, target, c.best, c.count, &r);
    });
    if (rc != BM_OK || c.empty) return rc;

    r.count = c.count;
    r.stored = list.size();
    if (r.stored) std::memcpy(hits, list.data(), list.size() * sizeof(Hit));
    *out = r;
    return BM_OK;
}

// bm_search_job_shares_gpu: no kernel of its own.  One header per extranonce2
// value of [en2_lo, en2_hi], ascending (host::job_header), each scanned by
// header_versions_hits_impl with what is left of the call's cap (0, a pure
// count, once the running count has passed it); host::JobMerge keeps the list
// and the best share until the last header has succeeded, so a failure
// part-way leaves shares and out untouched.  An empty range runs one empty
// inner call, so the stats are those of the last inner call either way.
int job_shares_impl(bm_ctx* ctx, const bm_job_t* job, uint32_t ntime, uint64_t en2_lo, uint64_t en2_hi,
                    const uint32_t* versions, size_t nver, uint32_t lo, uint32_t hi, const uint8_t* target,
                    bm_job_share_t* shares, size_t cap, bm_job_shares_result_t* out) {
    uint8_t block[32];
    const bool has_block = host::target_from_bits(job->nbits, block);
    host::JobMerge merge(cap, has_block ? block : nullptr, ntime, en2_lo, versions[0]);
    bm_header_versions_hits_result_t r;
    uint8_t header[kHeaderBytes] = {};
    std::unique_ptr<bm_header_version_hit_t[]> hits;  // one header's list: at most cap entries
    if (en2_lo > en2_hi || lo > hi) {
        BM_TRY(header_versions_hits_impl(ctx, header, versions, nver, 1, 0, target, hits.get(), 0, &r));
        merge.finish(shares, out);
        return BM_OK;
    }
    if (cap > 0) hits.reset(new bm_header_version_hit_t[cap]);
    for (uint64_t e = en2_lo;; ++e) {  // ends on e == en2_hi: en2_hi + 1 may wrap
        host::job_header(job, e, ntime, versions[0], header);
        BM_TRY(header_versions_hits_impl(ctx, header, versions, nver, lo, hi, target, hits.get(), merge.room(), &r));
        const int rc = merge.add(e, hits.get(), r);
        if (rc != BM_OK) return fail_call(ctx, rc);
        if (e == en2_hi) break;
    }
    merge.finish(shares, out);
    return BM_OK;
}

// The tail of every bm_search_*_gpu once it has checked its arguments:
// impl(&r) with the caller's current device kept and no exception leaving the
// C ABI; *out is written on success only.
template <class R, class Impl>
int call_into(R* out, Impl&& impl) {
    DeviceGuard guard;
    R r;
    const int rc = guarded([&] { return impl(&r); });
    if (rc == BM_OK) *out = r;
    return rc;
}

}  // namespace
}  // namespace bm

extern "C" {

int bm_search_gpu(bm_ctx_t* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, bm_result_t* out) {
    if (!ctx || !out || (len && !msg) || len > BM_MAX_MSG_LEN) return BM_EINVAL;
    return bm::call_into(out, [&](bm_result_t* r) { return bm::search_impl(ctx, msg, len, lower, upper, r); });
}

int bm_search_target_gpu(bm_ctx_t* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                         uint64_t target, bm_target_result_t* out) {
    if (!ctx || !out || (len && !msg) || len > BM_MAX_MSG_LEN) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // the group's allgather slot carries no hit
    return bm::call_into(out, [&](bm_target_result_t* r) {
        return bm::target_impl(ctx, msg, len, lower, upper, target, r);
    });
}

int bm_search_hits_gpu(bm_ctx_t* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                       uint64_t target, bm_result_t* hits, size_t cap, bm_hits_result_t* out) {
    if (!ctx || !out || (len && !msg) || len > BM_MAX_MSG_LEN) return BM_EINVAL;
    if (cap > BM_MAX_HITS || (!hits && cap > 0)) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // the group's allgather slot carries no hits
    return bm::call_into(out, [&](bm_hits_result_t* r) {
        return bm::hits_impl(ctx, msg, len, lower, upper, target, hits, cap, r);
    });
}

int bm_search_header_gpu(bm_ctx_t* ctx, const uint8_t* header, uint32_t nonce_lo, uint32_t nonce_hi,
                         const uint8_t* target, bm_header_result_t* out) {
    if (!ctx || !header || !target || !out) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    const uint32_t version = bm::host::header_version(header);  // the one-version case: the header as it stands
    return bm::call_into(out, [&](bm_header_result_t* r) {
        bm_header_versions_result_t v;
        BM_TRY(bm::header_versions_impl(ctx, header, &version, 1, nonce_lo, nonce_hi, target, &v));
        std::memcpy(r->hash, v.hash, sizeof r->hash);
        r->nonce = v.nonce;
        r->found = v.found;
        return BM_OK;
    });
}

int bm_search_header_hits_gpu(bm_ctx_t* ctx, const uint8_t* header, uint32_t nonce_lo, uint32_t nonce_hi,
                              const uint8_t* target, bm_header_hit_t* hits, size_t cap,
                              bm_header_hits_result_t* out) {
    if (!ctx || !header || !target || !out) return BM_EINVAL;
    if (cap > BM_MAX_HEADER_HITS || (!hits && cap > 0)) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    const uint32_t version = bm::host::header_version(header);  // the one-version case: the header as it stands
    return bm::call_into(out, [&](bm_header_hits_result_t* r) {
        bm_header_versions_hits_result_t v;
        BM_TRY(bm::header_versions_hits_impl(ctx, header, &version, 1, nonce_lo, nonce_hi, target, hits, cap, &v));
        std::memcpy(r->hash, v.hash, sizeof r->hash);
        r->nonce = v.nonce;
        r->reserved = 0;
        r->count = v.count;
        r->stored = v.stored;
        return BM_OK;
    });
}

int bm_search_header_versions_gpu(bm_ctx_t* ctx, const uint8_t* header, const uint32_t* versions, size_t nver,
                                  uint32_t nonce_lo, uint32_t nonce_hi, const uint8_t* target,
                                  bm_header_versions_result_t* out) {
    if (!ctx || !header || !versions || !target || !out) return BM_EINVAL;
    if (nver == 0 || nver > BM_MAX_HEADER_VERSIONS) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    return bm::call_into(out, [&](bm_header_versions_result_t* r) {
        return bm::header_versions_impl(ctx, header, versions, nver, nonce_lo, nonce_hi, target, r);
    });
}

int bm_search_header_versions_hits_gpu(bm_ctx_t* ctx, const uint8_t* header, const uint32_t* versions, size_t nver,
                                       uint32_t nonce_lo, uint32_t nonce_hi, const uint8_t* target,
                                       bm_header_version_hit_t* hits, size_t cap,
                                       bm_header_versions_hits_result_t* out) {
    if (!ctx || !header || !versions || !target || !out) return BM_EINVAL;
    if (nver == 0 || nver > BM_MAX_HEADER_VERSIONS) return BM_EINVAL;
    if (cap > BM_MAX_HEADER_HITS || (!hits && cap > 0)) return BM_EINVAL;
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    return bm::call_into(out, [&](bm_header_versions_hits_result_t* r) {
        return bm::header_versions_hits_impl(ctx, header, versions, nver, nonce_lo, nonce_hi, target, hits, cap, r);
    });
}

int bm_search_job_shares_gpu(bm_ctx_t* ctx, const bm_job_t* job, uint32_t ntime, uint64_t en2_lo, uint64_t en2_hi,
                             const uint32_t* versions, size_t nver, uint32_t nonce_lo, uint32_t nonce_hi,
                             const uint8_t* target, bm_job_share_t* shares, size_t cap,
                             bm_job_shares_result_t* out) {
    if (!ctx || !job || !versions || !target || !out) return BM_EINVAL;
    if (nver == 0 || nver > BM_MAX_HEADER_VERSIONS) return BM_EINVAL;
    if (cap > BM_MAX_HEADER_HITS || (!shares && cap > 0)) return BM_EINVAL;
    if (bm::host::job_check(job) != BM_OK) return BM_EINVAL;
    if (en2_lo <= en2_hi) {
        if (en2_hi - en2_lo >= BM_MAX_JOB_HEADERS) return BM_EINVAL;
        if (!bm::host::extranonce2_fits(en2_hi, job->extranonce2_size)) return BM_EINVAL;
    }
    if (ctx->rank_ctx && ctx->world > 1) return BM_EINVAL;  // rank groups are out of scope
    return bm::call_into(out, [&](bm_job_shares_result_t* r) {
        return bm::job_shares_impl(ctx, job, ntime, en2_lo, en2_hi, versions, nver, nonce_lo, nonce_hi, target, shares,
                                   cap, r);
    });
}

int bm_header_target_from_bits(uint32_t nbits, uint8_t* target) {
    if (!target) return BM_EINVAL;
    uint8_t t[32];
    if (!bm::host::target_from_bits(nbits, t)) return BM_EINVAL;
    std::memcpy(target, t, sizeof t);
    return BM_OK;
}

}  // extern "C"
