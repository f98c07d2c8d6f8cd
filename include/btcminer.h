/*
 * btcminer.h -- C ABI of libbtcminer.so, the MI355X (gfx950) nonce-search
 * backend for the distributed bitcoin miner.
 *
 * What it replaces in the reference (/root/reference/project2):
 *   bitcoin.Hash(msg string, nonce uint64) uint64          bitcoin/hash.go:11-15
 *   the miner's min-scan over a job's nonce range          bitcoin/miner/miner.go:43-74
 *                                                           (init :45-46, hot loop :58-65)
 * The Go miner would bind these with cgo; everything
 * else in the reference (LSP transport, JSON Join/Request/Result messages,
 * the server's scheduler) is unchanged by this library.
 *
 * Conventions
 *   - Every function returns an int status: BM_OK (0) or a negative BM_E*
 *     code; bm_strerror() names it.  Nothing aborts.  On failure the output
 *     arguments are left untouched.
 *   - msg is a raw byte string (Go's "%s" of a string: no escaping, may hold
 *     any byte).  The library copies what it needs before returning and keeps
 *     no caller pointer.
 *   - Ranges are INCLUSIVE [lower, upper] (project2/README.md:329,
 *     "0 <= n <= N").  upper = 2^64-1 is legal.  lower > upper is an empty
 *     range and yields {2^64-1, 2^64-1}, which is what miner.go:45-46 returns
 *     when its loop runs zero times.  (miner.go:59 itself loops i < Upper; a
 *     caller that wants that literal behaviour passes upper-1.)
 *   - Results are bit-exact with the reference scan: the minimum hash, and on
 *     ties the smallest nonce (strict '<' over ascending nonces, miner.go:61).
 *   - A context is not re-entrant: use one per OS thread or serialise calls.
 *     Calls are synchronous.  The caller's current HIP device is restored
 *     before each call returns.
 *   - The compute path is the gfx950 HIP kernels only.  There is no CPU
 *     fallback: without a usable GPU, bm_ctx_create() fails with BM_ENODEV.
 */
#ifndef BTCMINER_H
#define BTCMINER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BM_ABI_VERSION 7

/* status codes */
#define BM_OK 0
#define BM_EINVAL (-1)   /* bad argument (NULL pointer, msg too long, ...) */
#define BM_ENODEV (-2)   /* no usable gfx950 device / device id out of range */
#define BM_EHIP (-3)     /* a HIP runtime call failed */
#define BM_ERCCL (-4)    /* an RCCL call failed (multi-GPU contexts) */
#define BM_ENOMEM (-5)   /* host or device allocation failed */
#define BM_EINTERNAL (-6)/* planner invariant violated (a bug) */
#define BM_EPEER (-7)    /* rank contexts: another rank of the group failed this call */
#define BM_ETIMEDOUT (-8)/* rank contexts: the group did not answer within the peer timeout */
#define BM_EFULL (-9)    /* bm_share_set_verify: the batch's new hashes do not fit the set */

#define BM_MAX_MSG_LEN (1u << 20) /* bytes; LSP payloads are ~1 KB (README:61) */

/* The 16-byte result of a search: {Hash, Nonce} of bitcoin.NewResult
 * (bitcoin/message.go:36-42).  Ordered lexicographically (hash, nonce). */
typedef struct bm_result {
    uint64_t hash;
    uint64_t nonce;
} bm_result_t;

typedef struct bm_ctx bm_ctx_t;

int bm_abi_version(void);
const char* bm_strerror(int status);

/* Number of visible HIP devices (0 when there is none). */
int bm_device_count(int* out);
/* PCI bus id of a visible device ("0000:05:00.0"; len >= 13), e.g. to find
 * its driver clock in sysfs (bench.py samples it while it times). */
int bm_device_pci_bus_id(int device, char* buf, int len);

/* Context over devices 0..num_gpus-1 (num_gpus = 0: all visible devices).
 * A context with several devices splits every search across them and
 * combines the per-device partials with one RCCL allgather (host copies if
 * RCCL fails at run time; see bm_ctx_set_combine).
 * Launch-overlap tuning is read from the environment at creation (results
 * never depend on it): BTCMINER_STREAMS = launch streams per device (1..4,
 * default 2); BTCMINER_TAIL = nonces split off the biggest launch into a
 * short-task launch of their own (default 16777216, 0 = off); BTCMINER_CHUNK =
 * nonces per lane per work-counter dequeue, at most (10..100000, default 100);
 * BTCMINER_PADC=0 = never use the padding-block kernels with folded constants
 * (search_kernel_padc / search_kernel_padk; default: wherever they apply). */
int bm_ctx_create(int num_gpus, bm_ctx_t** out);
/* Context over an explicit device list (e.g. {LOCAL_RANK} for one process
 * per GPU).  A device listed twice is allowed (a one-GPU rehearsal of the
 * N-device split); such a context combines on the host. */
int bm_ctx_create_devices(const int* devices, int n, bm_ctx_t** out);

/* ---- one process per GPU: a context that is one rank of an RCCL group ----
 * Every rank calls bm_search_gpu() with the SAME (msg, lower, upper): rank r
 * scans the r-th of `world` contiguous pieces of the range (near-equal, or
 * per bm_ctx_set_split).  The reference's equivalent is the server handing
 * each miner a piece of the request (bitcoin/server/server.go:153-169).
 *
 * Two steps, so that no rank waits in RCCL for a peer that failed earlier:
 *   1. bm_ctx_create_rank_local() on the rank's own device: every resource,
 *      no communicator.  Such a context is usable on its own: a search
 *      returns THIS rank's partial (its piece's min), which the caller
 *      combines over any side channel (bench.py's rendezvous gather).
 *   2. once every rank has created its context (exchange the statuses over
 *      the side channel), rank 0 calls bm_rccl_unique_id() and hands the
 *      bytes to every rank, and each calls bm_ctx_join_rank(): a
 *      non-blocking ncclCommInitRankConfig on a worker thread; the call
 *      waits for it at most timeout_ms (0: no limit) and then returns
 *      BM_ETIMEDOUT.  RCCL's bootstrap can block inside that init until
 *      every rank has connected (RCCL 2.27 does), so the worker may stay
 *      there: the context keeps it as its pending join, aborts whatever
 *      communicator it ends up with, and starts no second one -- a later
 *      bm_ctx_join_rank() first waits up to its own timeout_ms for the
 *      pending one to end and returns BM_ETIMEDOUT if it has not.
 *      bm_ctx_destroy() leaves a still-blocked worker detached (it holds no
 *      reference to the context); it ends with the process.  The context
 *      itself stays usable for searches of its own piece throughout.
 *      From then on a search ends with
 *      one RCCL allgather of 32-byte slots {hash, nonce, status, 0}, so
 *      every rank returns the whole range's answer -- or, when any rank
 *      failed the call before the combine (it still takes part, with its
 *      status in the slot -- a HIP error while staging that slot included),
 *      every rank fails it together: the failing rank with its own status,
 *      the others with BM_EPEER.  Only a rank that cannot post its slot at
 *      all aborts its communicator instead; its peers then see that as a
 *      communicator error or wait for their peer timeout.
 * bm_ctx_create_rank() is both steps in one call (blocking join).
 * bm_ctx_set_peer_timeout(): a joined rank waits at most this long for the
 *   group's allgather after its own work ends (default BM_DEFAULT_PEER_TIMEOUT_MS,
 *   10 minutes, so a peer that never posts its slot is a bounded failure;
 *   0: no limit); past it the communicator is aborted and the call returns
 *   BM_ETIMEDOUT, as does every later search until bm_ctx_leave_rank().
 *   Callers whose pieces take longer than that per call raise it.
 * bm_ctx_join_rank(): timeout_ms bounds the WHOLE call, including the wait
 *   for a pending join; 0 waits without limit.
 * bm_ctx_leave_rank(): drop the communicator; searches return the rank's
 *   own partial again.  bm_ctx_rank_joined(): 1 inside a group, else 0.
 * bm_ctx_destroy() (any context) waits for its own streams, then drops every
 *   communicator it holds with ncclCommAbort: teardown never waits on a peer,
 *   even one that has died. */
#define BM_RCCL_ID_BYTES 128
#define BM_DEFAULT_PEER_TIMEOUT_MS 600000
int bm_rccl_unique_id(uint8_t* id /* BM_RCCL_ID_BYTES */);
int bm_ctx_create_rank_local(int device, int rank, int world, bm_ctx_t** out);
int bm_ctx_join_rank(bm_ctx_t* ctx, const uint8_t* id, int timeout_ms);
int bm_ctx_leave_rank(bm_ctx_t* ctx);
int bm_ctx_rank_joined(const bm_ctx_t* ctx, int* joined);
int bm_ctx_set_peer_timeout(bm_ctx_t* ctx, int timeout_ms);
int bm_ctx_create_rank(int device, int rank, int world, const uint8_t* id, bm_ctx_t** out);
int bm_ctx_rank(const bm_ctx_t* ctx, int* rank, int* world);
int bm_ctx_destroy(bm_ctx_t* ctx);
int bm_ctx_num_devices(const bm_ctx_t* ctx, int* out);

/* The hot path: min over n in [lower, upper] of (Hash(msg, n), n).
 * Replaces miner.go:58-65 (+ hash.go:11-15 per nonce). */
int bm_search_gpu(bm_ctx_t* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                  bm_result_t* out);

/* ---- target search: the first nonce whose hash meets a target ------------
 * bm_search_target_gpu scans [lower, upper] for Hash(msg, n) <= target (full
 * 64-bit unsigned compare) and stops scanning above a hit once one is known.
 *   found = 1: nonce is the SMALLEST n in [lower, upper] with Hash(msg, n) <=
 *     target and hash = Hash(msg, nonce): what a sequential ascending scan
 *     that stops at its first hit returns.
 *   found = 0: no nonce meets the target; (hash, nonce) is exactly
 *     bm_search_gpu's answer for the range (all of it was scanned).
 *   lower > upper: found = 0, {2^64-1, 2^64-1}.  target = 2^64-1 always finds
 *     lower.  upper = 2^64-1 is legal.
 * The result never depends on timing, residency, streams, task digits,
 * max_windows or the split.  On failure `out` is untouched and the context
 * stays usable; the next bm_search_gpu on the context is unaffected.
 * Contexts: one device, or one process over several devices (a device listed
 * N times included): each device scans its piece with a hit word of its own
 * and the host takes the lowest-nonce hit, or the lexicographic min of the
 * partials when no device found one -- always by host copies, whatever
 * bm_ctx_set_combine says.  A hit on one device does NOT cancel another
 * device's work in flight (out of scope: every device still ends within its
 * own piece).  A rank context with world > 1 returns BM_EINVAL, joined or
 * not: the group's 32-byte allgather slot carries no hit.
 * bm_ctx_set_balance does not learn from target calls (their spans say
 * nothing about a device's rate); bm_ctx_set_test_fault applies as for a
 * search.  bm_ctx_last_stats is filled as for a search (the launch list). */
typedef struct bm_target_result {
    uint64_t hash;     /* found: Hash(msg, nonce); else the range's minimum hash */
    uint64_t nonce;    /* found: the first nonce at or below target; else the minimum's nonce */
    int32_t found;     /* 1: some nonce of the range has Hash <= target */
    int32_t reserved;  /* 0 */
} bm_target_result_t;

int bm_search_target_gpu(bm_ctx_t* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                         uint64_t target, bm_target_result_t* out);

/* ---- hit enumeration: every nonce whose hash meets a target --------------
 * bm_search_hits_gpu scans all of [lower, upper] (no early exit) and returns
 * every n with Hash(msg, n) <= target (full 64-bit unsigned compare), plus
 * the range's minimum.
 *   hits[0 .. stored) holds {Hash(msg, n), n} for every hit in ascending nonce
 *     order, each exactly once.  count is exact, always.
 *   All or nothing: count > cap writes NOTHING to hits, stored = 0, and the
 *     call still succeeds with the exact count; ask again with a larger buffer
 *     or a smaller range.  No subset is ever returned, so the result never
 *     depends on timing, residency, streams, task digits, max_windows or the
 *     split.
 *   hits == NULL with cap == 0 is a pure count.  cap > BM_MAX_HITS, or
 *     hits == NULL with cap > 0: BM_EINVAL.
 *   lower > upper: {2^64-1, 2^64-1, 0, 0}.  upper = 2^64-1 is legal and the
 *     nonce 2^64-1 is reported like any other.
 * On failure `out` and `hits` are untouched and the context stays usable (a
 * device buffer that cannot grow to cap: BM_ENOMEM).
 * Contexts: one device, or one process over several devices (a device listed
 * N times included): each device appends to a buffer and a counter of its
 * own, and the host concatenates them in device order (pieces ascend) --
 * always by host copies.  A rank context with world > 1 returns BM_EINVAL.
 * bm_ctx_set_balance does not learn from these calls (their time depends on
 * the hit density); bm_ctx_set_test_fault applies as for a search;
 * bm_ctx_last_stats is filled as for a search (nonces = the range size).
 * Cost: that of bm_search_gpu while hits are rare.  Every hit is one atomic
 * on one word per device, so targets of about 8 leading zero bits or fewer
 * are bound by that atomic, not by hashing; the result stays exact at any
 * density, target = 2^64-1 included. */
#define BM_MAX_HITS (1u << 22) /* entries; 64 MiB of device buffer per device at most */
typedef struct bm_hits_result {
    uint64_t hash, nonce; /* the range's minimum: exactly bm_search_gpu's answer */
    uint64_t count;       /* nonces n in [lower, upper] with Hash(msg, n) <= target: exact, always */
    uint64_t stored;      /* entries written to hits[]: count when count <= cap, else 0 */
} bm_hits_result_t;

int bm_search_hits_gpu(bm_ctx_t* ctx, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                       uint64_t target, bm_result_t* hits, size_t cap, bm_hits_result_t* out);

/* ---- Bitcoin block headers: double SHA-256 over a nonce range ------------
 * The hash of a nonce is H(n) = SHA256(SHA256(header[0:76] || le32(n))) read as
 * a little-endian 256-bit integer (what block explorers print).  Bytes 76..79
 * of the caller's header are ignored.  `hash` and `target` are 256-bit numbers
 * written MOST significant byte first (= the sha256d digest bytes reversed).
 *
 * bm_search_header_gpu scans [nonce_lo, nonce_hi] for H(n) <= target, compared
 * over the full 256 bits, and stops handing out work above a hit once one is
 * known (as bm_search_target_gpu does).
 *   found = 1: nonce is the SMALLEST n of the range with H(n) <= target and
 *     hash = H(nonce).
 *   found = 0: the whole range was scanned; nonce minimises the pair
 *     (H(n) >> 192, n) lexicographically -- the top 64 bits of the hash, the
 *     smallest nonce on equal top bits: the range's "best share" -- and
 *     hash = H(nonce) in full (recomputed on the host).
 *   nonce_lo > nonce_hi: found = 0, hash all 0xFF, nonce = 0xFFFFFFFF.
 *     nonce_hi = 2^32-1 is legal.  An all-ones target always finds nonce_lo.
 * The result never depends on timing, residency, streams, BTCMINER_CHUNK,
 * blocks per CU or the split.  On failure `out` is untouched and the context
 * stays usable; the next bm_search_gpu on it is unaffected.
 * Contexts: one device, or one process over several devices (a device listed
 * N times included): the nonce range is cut by the partitioner, each device
 * has a hit word of its own, and the host takes the lowest-nonce hit, or else
 * the lexicographic minimum of the partials -- always by host copies.  A rank
 * context with world > 1 returns BM_EINVAL.
 * bm_ctx_set_balance does not learn from these calls; bm_ctx_set_test_fault
 * applies as for a search; bm_ctx_last_stats is filled, one launch per device
 * (p = digits = inner_digits = 0: a launch of the header kernel);
 * bm_ctx_last_target_stats is filled with the nonces dispatched, as for a
 * target search.
 *
 * bm_header_hash_gpu: out[32*i .. 32*i+31] = H(nonces[i]), most significant
 * byte first, on the first device of ctx, by a kernel that shares none of the
 * search's shortcuts (the twin of bm_hash_gpu).  n <= BM_MAX_HEADER_HASHES.
 *
 * bm_header_target_from_bits (pure CPU): Bitcoin's compact target.
 * mantissa = nbits & 0x7fffff, exponent = nbits >> 24, target = mantissa <<
 * 8 * (exponent - 3), a right shift for exponents below 3.  BM_EINVAL when the
 * sign bit 0x00800000 is set or the value overflows 256 bits.
 *
 * Rolling extranonce2 past 2^32 nonces is bm_search_job_shares_gpu, below.
 * Out of scope: rolling ntime (the caller changes the header and calls again; a
 * call is a fraction of a second); cancelling one device's work on another device's hit; rank groups; the LSP
 * server protocol. */
#define BM_MAX_HEADER_HASHES (1u << 24)
typedef struct bm_header_result {
    uint8_t hash[32]; /* found: H(nonce); else H of the best share's nonce */
    uint32_t nonce;
    int32_t found;    /* 1: some nonce of the range has H <= target */
} bm_header_result_t; /* 40 bytes */

int bm_search_header_gpu(bm_ctx_t* ctx, const uint8_t header[80], uint32_t nonce_lo, uint32_t nonce_hi,
                         const uint8_t target[32], bm_header_result_t* out);
int bm_header_hash_gpu(bm_ctx_t* ctx, const uint8_t header[80], const uint32_t* nonces, size_t n,
                       uint8_t* out /* 32 * n */);
int bm_header_target_from_bits(uint32_t nbits, uint8_t target[32]);

/* ---- block-header shares: every nonce whose hash meets a target -----------
 * bm_search_header_hits_gpu scans all of [nonce_lo, nonce_hi] (no early exit)
 * and returns every n with H(n) <= target, plus the range's best share: what a
 * pool miner submits for one header.  H, `hash` and `target` are as above: 256-bit
 * numbers written MOST significant byte first, compared over the full 256 bits.
 *   hits[0 .. stored) holds {H(n), n, 0} for every hit in ascending nonce order,
 *     each nonce exactly once (every hash recomputed on the host).  count is
 *     exact, always.
 *   All or nothing: count > cap writes NOTHING to hits, stored = 0, and the
 *     call still succeeds with the exact count; ask again with a larger buffer
 *     or a smaller range.  No subset is ever returned.
 *   hits == NULL with cap == 0 is a pure count.  cap > BM_MAX_HEADER_HITS, or
 *     hits == NULL with cap > 0: BM_EINVAL.  A NULL ctx, header, target or out:
 *     BM_EINVAL, before anything is dereferenced.
 *   out->hash / out->nonce: the range's best share in full, exactly the answer
 *     of bm_search_header_gpu with found = 0 (target 0): the minimum of
 *     (H(n) >> 192, n).
 *   nonce_lo > nonce_hi: hash all 0xFF, nonce = 0xFFFFFFFF, count = stored = 0,
 *     hits untouched.  nonce_hi = 2^32-1 is legal.
 * The result never depends on timing, residency, streams, BTCMINER_CHUNK,
 * blocks per CU or the split.  On failure `out` and `hits` are untouched and
 * the context stays usable (a device buffer that cannot grow to cap:
 * BM_ENOMEM, and the context is as it was).
 * Contexts: one device, or one process over several devices (a device listed
 * N times included): the nonce range is cut by the partitioner, each device
 * appends 16-byte entries {H(n) >> 192, n} to the buffer and counter that
 * bm_search_hits_gpu uses, and the host sorts them by nonce, recomputes each
 * full hash and checks the device's claim (BM_EINTERNAL if one fails) -- always
 * by host copies.  A rank context with world > 1 returns BM_EINVAL.
 * bm_ctx_set_balance does not learn from these calls; bm_ctx_set_test_fault
 * applies as for a header search; bm_ctx_last_stats is filled, one launch per
 * device (a launch of the header kernel in hits mode; nonces = the range size);
 * bm_ctx_last_target_stats is not touched.
 * Cost: that of a full bm_search_header_gpu scan while hits are rare.  Every
 * hit is one atomic on one word per device and, when stored, one sha256d on
 * the host.
 *
 * Several headers in one call, with extranonce2 and merkle rolling, is
 * bm_search_job_shares_gpu, below.
 * Out of scope: cancelling across devices; rank groups; the LSP server protocol. */
#define BM_MAX_HEADER_HITS (1u << 20) /* entries; each stored hit costs one host sha256d */
typedef struct bm_header_hit {
    uint8_t hash[32]; /* H(nonce) */
    uint32_t nonce;
    uint32_t reserved; /* 0 */
} bm_header_hit_t;     /* 40 bytes */
typedef struct bm_header_hits_result {
    uint8_t hash[32];  /* the range's best share, in full: bm_search_header_gpu's found = 0 answer */
    uint32_t nonce;    /* its nonce */
    uint32_t reserved; /* 0 */
    uint64_t count;    /* nonces of the range with H(n) <= target: exact, always */
    uint64_t stored;   /* entries written to hits[]: count when count <= cap, else 0 */
} bm_header_hits_result_t; /* 56 bytes */

int bm_search_header_hits_gpu(bm_ctx_t* ctx, const uint8_t header[80], uint32_t nonce_lo, uint32_t nonce_hi,
                              const uint8_t target[32], bm_header_hit_t* hits, size_t cap,
                              bm_header_hits_result_t* out);

/* ---- version rolling: one header under several version fields -------------
 * After 2^32 nonces a miner changes the header, and the cheapest change is the
 * version field (BIP 320: the bits of mask 0x1fffe000 are free).  The version
 * lies in the header's first 64-byte block, so the second block's message
 * schedule is the same for every version, and a kernel that runs several
 * versions side by side computes it once per nonce (overt AsicBoost).
 *
 * H(i, n) is bm_search_header_gpu's H(n) of the header whose bytes 0..3 are
 * le32(versions[i]).  Bytes 0..3 and 76..79 of the caller's header are ignored.
 * bm_search_header_versions_gpu scans [nonce_lo, nonce_hi] for every version.
 *   found = 1: the pair minimising (n, i) lexicographically among all pairs of
 *     the range with i < nver and H(i, n) <= target: the smallest nonce at
 *     which any version hits, then the smallest index.  A repeated version is
 *     legal and loses the tie to its first occurrence.
 *   found = 0: the whole range was scanned for every version; the pair
 *     minimises (H(i, n) >> 192, n, i).
 *   hash = H(version_index, nonce) in full, recomputed on the host, which also
 *     checks the device's claim (BM_EINTERNAL if it does not hold).
 *   nonce_lo > nonce_hi: found = 0, hash all 0xFF, nonce = 0xFFFFFFFF,
 *     version_index = 0, version = versions[0].
 * The result never depends on timing, residency, streams, BTCMINER_CHUNK,
 * blocks per CU, the split or on how the versions are grouped into launches:
 * the list is cut into groups of 4, 2 and 1 versions (BTCMINER_HEADER_GROUP =
 * 1, 2 or 4 caps the group size), one launch per device and group, and all of
 * a device's launches share its hit word, so a later group scans only up to the
 * best hit so far.
 * nver == 0, nver > BM_MAX_HEADER_VERSIONS or a NULL ctx, header, versions,
 * target or out: BM_EINVAL.  A rank context with world > 1: BM_EINVAL.  On
 * failure `out` is untouched and the context stays usable.
 * Contexts: as for bm_search_header_gpu; the nonce range is split and every
 * device runs every version over its piece; the combine is by host copies.
 * bm_ctx_set_balance does not learn from these calls; bm_ctx_set_test_fault
 * applies; bm_ctx_last_stats lists one launch per device and group (nonces =
 * the piece's size times the group's versions); bm_ctx_last_target_stats
 * counts (nonce, version) pairs in nonces_dispatched.
 *
 * Share enumeration across versions is bm_search_header_versions_hits_gpu, below.
 * Extranonce2 and merkle rolling is bm_search_job_shares_gpu, below.
 * Out of scope: ntime rolling; cancelling across devices; rank groups; the LSP
 * server protocol. */
#define BM_MAX_HEADER_VERSIONS 64
typedef struct bm_header_versions_result {
    uint8_t hash[32];       /* as bm_header_result_t: most significant byte first */
    uint32_t nonce;
    uint32_t version_index; /* index into versions[] */
    uint32_t version;       /* versions[version_index] */
    int32_t found;
} bm_header_versions_result_t; /* 48 bytes */

int bm_search_header_versions_gpu(bm_ctx_t* ctx, const uint8_t header[80], const uint32_t* versions, size_t nver,
                                  uint32_t nonce_lo, uint32_t nonce_hi, const uint8_t target[32],
                                  bm_header_versions_result_t* out);

/* ---- version-rolling shares: every (nonce, version) pair that meets a target
 * bm_search_header_versions_hits_gpu scans all of [nonce_lo, nonce_hi] under
 * every version (no early exit) and returns every pair (n, i), i < nver, with
 * H(i, n) <= target, plus the best share over all pairs: what a pool miner with
 * version rolling on submits.  H(i, n), `hash` and `target` are as for
 * bm_search_header_versions_gpu: 256-bit numbers written MOST significant byte
 * first, compared over the full 256 bits.
 *   hits[0 .. stored) holds {H(i, n), n, i, versions[i], 0} for every hit,
 *     ascending by (nonce, version_index), each pair exactly once (every hash
 *     recomputed on the host).  A version that appears twice in the list yields
 *     two entries with different indices.  count is exact, always.
 *   All or nothing, as in bm_search_header_hits_gpu: count > cap writes NOTHING
 *     to hits, stored = 0, and the call still succeeds with the exact count.
 *   hits == NULL with cap == 0 is a pure count.  cap > BM_MAX_HEADER_HITS, or
 *     hits == NULL with cap > 0: BM_EINVAL.
 *   out->hash / nonce / version_index / version: the pair minimising
 *     (H(i, n) >> 192, n, i), with its full hash: exactly the answer of
 *     bm_search_header_versions_gpu at target 0.
 *   nonce_lo > nonce_hi: count = stored = 0 and that call's empty answer: hash
 *     all 0xFF, nonce = 0xFFFFFFFF, version_index = 0, version = versions[0];
 *     hits untouched.
 * nver == 0, nver > BM_MAX_HEADER_VERSIONS or a NULL ctx, header, versions,
 * target or out: BM_EINVAL, before anything is dereferenced.  A rank context
 * with world > 1: BM_EINVAL.  On any failure `hits` and `out` are untouched and
 * the context stays usable (a device buffer that cannot grow to cap: BM_ENOMEM).
 * The result never depends on timing, residency, streams, BTCMINER_CHUNK,
 * blocks per CU, the split or the grouping (BTCMINER_HEADER_GROUP).
 * Contexts: one device, or one process over several (a device listed N times
 * included): the nonce range is cut by the partitioner, every device runs every
 * group of versions over its piece, one launch of header_versions_hits_kernel<M>
 * per device and group, all of a device's launches appending 16-byte entries
 * {H(i, n) >> 192, (n << 32) | i} through one counter into one buffer; the host
 * sorts them by (n, i), recomputes each full hash and checks the device's claim
 * (BM_EINTERNAL if one fails) -- always by host copies.
 * bm_ctx_set_balance does not learn from these calls; bm_ctx_set_test_fault
 * applies; bm_ctx_last_stats lists one launch per device and group and counts
 * (nonce, version) pairs in nonces; bm_ctx_last_target_stats is not touched.
 * Cost: that of a full bm_search_header_versions_gpu scan while hits are rare.
 *
 * Extranonce2 and merkle rolling is bm_search_job_shares_gpu, below.
 * Out of scope: ntime rolling; cancelling across devices; rank groups; the LSP
 * server protocol. */
typedef struct bm_header_version_hit {
    uint8_t hash[32];        /* H(version_index, nonce), most significant byte first */
    uint32_t nonce;
    uint32_t version_index;  /* index into versions[] */
    uint32_t version;        /* versions[version_index] */
    uint32_t reserved;       /* 0 */
} bm_header_version_hit_t;   /* 48 bytes */
typedef struct bm_header_versions_hits_result {
    uint8_t hash[32];        /* the best share over all pairs, in full */
    uint32_t nonce, version_index, version, reserved;
    uint64_t count;          /* pairs (n, i), n in [lo, hi], i < nver, H(i, n) <= target: exact, always */
    uint64_t stored;         /* entries written to hits[]: count when count <= cap, else 0 */
} bm_header_versions_hits_result_t; /* 64 bytes */

int bm_search_header_versions_hits_gpu(bm_ctx_t* ctx, const uint8_t header[80], const uint32_t* versions,
                                       size_t nver, uint32_t nonce_lo, uint32_t nonce_hi, const uint8_t target[32],
                                       bm_header_version_hit_t* hits, size_t cap,
                                       bm_header_versions_hits_result_t* out);

/* ---- Stratum jobs: extranonce2 rolling over the version-rolling shares -------
 * A pool hands out a job, not a header: a coinbase in two halves, the miner's
 * extranonce1, the size of extranonce2, a merkle branch, prevhash, version,
 * nbits, ntime and a difficulty.  For a value of extranonce2
 *   coinbase = coinb1 || extranonce1 || BE(extranonce2, extranonce2_size) || coinb2
 *   root     = sha256d(coinbase); for each branch entry: root = sha256d(root || entry)
 *   header   = le32(version) || prevhash || root || le32(ntime) || le32(nbits) || 00000000
 * extranonce2 is serialised big-endian, so mining.submit's extranonce2 string is
 * the zero-padded hex of the integer.  The branch entries are the 32 bytes of
 * each hex string as sent (raw digest order).  prevhash holds bytes 4..35 of the
 * header; mining.notify sends it with each 4-byte word reversed
 * (bm_job_prevhash_from_stratum undoes that; in and out may be the same array).
 *
 * The three entries below are pure CPU: no context, no GPU.
 * bm_job_header: the 80 bytes above.  BM_EINVAL for a NULL job or header, a NULL
 *   pointer with a non-zero length, extranonce2_size outside 1..8, extranonce2 >=
 *   2^(8 * size), nbranch > BM_MAX_JOB_BRANCH, or a coinbase longer than
 *   BM_MAX_JOB_COINBASE; header is untouched then.
 * bm_target_from_difficulty: target = floor(diff1 / difficulty), diff1 = 0xffff *
 *   2^208 (the target of nbits 1d00ffff), exact for the double's rational value
 *   (one big-integer division, no floating point in the quotient), saturating at
 *   2^256 - 1; most significant byte first.  BM_EINVAL for a NaN, an infinity, a
 *   value <= 0 or a NULL target.
 * bm_target_from_difficulty_fx: the same for a difficulty in units of 2^-32 (the unit
 *   of the ledger's weights): target = floor(0xffff * 2^240 / difficulty_fx), exact
 *   integer arithmetic; it never saturates (difficulty_fx = 1 gives 0xffff * 2^240).
 *   Below 2^53 it is bm_target_from_difficulty(difficulty_fx / 2^32) byte for byte.
 *   BM_EINVAL for 0 or a NULL target.
 *
 * bm_search_job_shares_gpu: for every extranonce2 of [en2_lo, en2_hi], ascending,
 * the header of (job, extranonce2, ntime) is scanned by the version-rolling share
 * enumeration over versions[0 .. nver) and [nonce_lo, nonce_hi]: a host loop of
 * bm_search_header_versions_hits_gpu's own call, one per header (job->version is
 * not used: every header's version field comes from versions[]).  H, `hash` and
 * `target` are as there: most significant byte first, compared over 256 bits.
 *   shares[0 .. stored) holds every hit, ascending by (extranonce2, nonce,
 *     version_index), each triple exactly once.  is_block = 1 when the hash is
 *     also <= bm_header_target_from_bits(job->nbits); an nbits that does not
 *     decode leaves it 0.  count is exact, always.
 *   All or nothing over the whole call: count > cap writes NOTHING to shares,
 *     stored = 0, and the call still succeeds with the exact count (once the
 *     running count passes cap, the remaining headers run as pure counts).
 *     shares == NULL with cap == 0 is a pure count.  cap > BM_MAX_HEADER_HITS, or
 *     shares == NULL with cap > 0: BM_EINVAL.
 *   out->hash / extranonce2 / nonce / version_index / version: the share
 *     minimising (H >> 192, extranonce2, nonce, version_index) over everything
 *     scanned, with its full hash.  headers = extranonce2 values scanned.
 *   en2_lo > en2_hi or nonce_lo > nonce_hi: nothing is scanned: hash all 0xFF,
 *     nonce = 0xFFFFFFFF, extranonce2 = en2_lo, version_index = 0, version =
 *     versions[0], count = stored = headers = 0; shares untouched.
 *   More than BM_MAX_JOB_HEADERS values in [en2_lo, en2_hi], or en2_hi >=
 *     2^(8 * size): BM_EINVAL.  en2_hi = 2^64 - 1 with size 8 is legal.
 * A NULL ctx, job, versions, target or out, nver == 0 or > BM_MAX_HEADER_VERSIONS,
 * or a job bm_job_header refuses: BM_EINVAL, before anything else is
 * dereferenced.  A rank context with world > 1: BM_EINVAL.  On any failure
 * `shares` and `out` are untouched and the context stays usable.
 * The result never depends on timing, residency, streams, BTCMINER_CHUNK, blocks
 * per CU, the split or the grouping (BTCMINER_HEADER_GROUP): it is the inner
 * call's, header by header.  bm_ctx_set_test_fault applies to each inner call.
 * bm_ctx_last_stats describes the LAST inner call only (one header; an empty
 * range: an empty inner call); bm_ctx_last_target_stats is not touched.
 * Cost: headers x one bm_search_header_versions_hits_gpu call; building a header
 * is two host hashes of the coinbase plus one per branch entry.
 *
 * Out of scope: a network Stratum client; ntime rolling inside the call;
 * cancelling across devices; rank groups; the LSP server protocol. */
#define BM_MAX_JOB_COINBASE (1u << 16) /* bytes of coinb1 + extranonce1 + extranonce2 + coinb2 */
#define BM_MAX_JOB_BRANCH 32
#define BM_MAX_JOB_HEADERS 4096        /* extranonce2 values per call */
typedef struct bm_job {
    const uint8_t* coinb1;
    size_t coinb1_len;
    const uint8_t* extranonce1;
    size_t extranonce1_len;
    uint32_t extranonce2_size; /* 1..8 bytes */
    const uint8_t* coinb2;
    size_t coinb2_len;
    const uint8_t* branch;     /* nbranch * 32 bytes, as sent (raw digest order) */
    size_t nbranch;
    uint8_t prevhash[32];      /* header byte order (bytes 4..35 of the header) */
    uint32_t version, nbits;   /* as integers: the header holds le32 of them */
} bm_job_t;
typedef struct bm_job_share {
    uint8_t hash[32];          /* most significant byte first, recomputed on the host */
    uint64_t extranonce2;
    uint32_t nonce, ntime;
    uint32_t version_index, version;
    uint32_t is_block;         /* 1: hash also <= the target of job->nbits */
    uint32_t reserved;         /* 0 */
} bm_job_share_t;              /* 64 bytes */
typedef struct bm_job_shares_result {
    uint8_t hash[32];          /* best share over everything scanned */
    uint64_t extranonce2;
    uint32_t nonce, version_index, version, reserved;
    uint64_t count, stored;
    uint64_t headers;          /* extranonce2 values scanned */
} bm_job_shares_result_t;      /* 80 bytes */

int bm_job_prevhash_from_stratum(const uint8_t in[32], uint8_t out[32]);
int bm_job_header(const bm_job_t* job, uint64_t extranonce2, uint32_t ntime, uint32_t version, uint8_t header[80]);
int bm_target_from_difficulty(double difficulty, uint8_t target[32]);
int bm_target_from_difficulty_fx(uint64_t difficulty_fx, uint8_t target[32]);
int bm_search_job_shares_gpu(bm_ctx_t* ctx, const bm_job_t* job, uint32_t ntime, uint64_t en2_lo, uint64_t en2_hi,
                             const uint32_t* versions, size_t nver, uint32_t nonce_lo, uint32_t nonce_hi,
                             const uint8_t target[32], bm_job_share_t* shares, size_t cap,
                             bm_job_shares_result_t* out);

/* ---- pool-side share verification: a batch of mining.submit tuples ------------
 * What a pool, a proxy or a test of a miner does with the (extranonce2, ntime,
 * nonce, version) tuples it receives for a job: rebuild each header, hash it and
 * decide between an accepted share, a block and a reject.  Every submission needs
 * a merkle root of its own (its coinbase under its extranonce2, the branch, the
 * header's double hash: about 45 compressions under a 12-entry branch), so this
 * is per-item work, and bm_job_verify_gpu gives one lane to each submission.
 *
 *   verdicts[i] belongs to submits[i]; the order is the caller's.
 *   submits[i].version is the FULL header version field (a caller composes it
 *     from the job's version and mining.submit's version bits); reserved is
 *     ignored.
 *   verdicts[i].hash = H of bm_job_header(job, extranonce2, ntime, version) with
 *     nonce in bytes 76..79, most significant byte first like every header call.
 *   verdicts[i].status = the OR of
 *     BM_SUBMIT_SHARE   hash <= target,
 *     BM_SUBMIT_BLOCK   hash <= bm_header_target_from_bits(job->nbits); an nbits
 *                       that does not decode leaves it clear everywhere.  The two
 *                       flags are independent: a share target below the block
 *                       target can give BLOCK without SHARE,
 *     BM_SUBMIT_INVALID extranonce2 >= 2^(8 * extranonce2_size): nothing is
 *                       hashed, hash is all 0xFF and status is exactly this flag,
 *     both compares over the full 256 bits.  verdicts[i].reserved = 0.
 *   out: n and how many verdicts carry each flag.
 *   n == 0 succeeds with a zero *out and touches neither array (both may be NULL).
 * BM_EINVAL: n > BM_MAX_JOB_SUBMITS; a NULL job, target or out (or ctx); NULL
 * submits or verdicts with n > 0; a job bm_job_header refuses; a rank context
 * with world > 1.  On any failure `verdicts` and `out` are untouched and the
 * context stays usable.
 *
 * bm_job_verify_cpu is pure CPU, no context: the specification, and what a
 * caller without a GPU uses.  bm_job_verify_gpu gives byte-identical `verdicts`
 * and `out`, on the first device of ctx (like bm_header_hash_gpu): one
 * host-to-device copy (the job's tail template, its branch and the submissions),
 * one launch of job_verify_kernel and one copy back, on that device's stream.
 * The host then recomputes entry 0, entry n - 1 and every entry flagged BLOCK
 * with the CPU path and returns BM_EINTERNAL on any difference: a tripwire, not
 * the result -- everything else is the device's claim.  bm_ctx_last_stats is left
 * as the previous call left it.
 *
 * Out of scope: duplicate detection across batches; vardiff; a network Stratum
 * server; splitting a batch over devices; rank groups.  Submissions of many
 * sessions (an extranonce1 and a target each) in one call, and an ntime window:
 * bm_pool_verify_gpu, below. */
#define BM_MAX_JOB_SUBMITS (1u << 20)
#define BM_SUBMIT_SHARE 1u   /* hash <= target */
#define BM_SUBMIT_BLOCK 2u   /* hash <= the target of job->nbits (needs a decodable nbits) */
#define BM_SUBMIT_INVALID 4u /* extranonce2 >= 2^(8 * extranonce2_size): not hashed */
typedef struct bm_job_submit {
    uint64_t extranonce2;
    uint32_t ntime, nonce;
    uint32_t version;  /* the full header version field */
    uint32_t reserved; /* ignored */
} bm_job_submit_t;     /* 24 bytes */
typedef struct bm_job_verdict {
    uint8_t hash[32];  /* most significant byte first; all 0xFF for an INVALID entry */
    uint32_t status;   /* BM_SUBMIT_* */
    uint32_t reserved; /* 0 */
} bm_job_verdict_t;    /* 40 bytes */
typedef struct bm_job_verify_result {
    uint64_t n;        /* submissions */
    uint64_t shares, blocks, invalid; /* verdicts with BM_SUBMIT_SHARE / _BLOCK / _INVALID */
} bm_job_verify_result_t; /* 32 bytes */

int bm_job_verify_cpu(const bm_job_t* job, const uint8_t target[32], const bm_job_submit_t* submits, size_t n,
                      bm_job_verdict_t* verdicts, bm_job_verify_result_t* out);
int bm_job_verify_gpu(bm_ctx_t* ctx, const bm_job_t* job, const uint8_t target[32], const bm_job_submit_t* submits,
                      size_t n, bm_job_verdict_t* verdicts, bm_job_verify_result_t* out);

/* ---- pool-side share verification across sessions: one job, many workers --------
 * A pool sends the same job to every connection; each connection has its own
 * extranonce1 and its own difficulty.  bm_pool_verify_gpu is bm_job_verify_gpu with
 * extranonce1 and the share target as per-submission data: submits[i].session picks
 * sessions[s], and an ntime window is checked along the way.  One call covers one
 * job's submissions from every session; bm_job_verify_* is unchanged beside it.
 *
 *   job->extranonce1 is ignored and may be NULL.  job->extranonce1_len is the size
 *     of EVERY session's extranonce1 and must be 1..8: the first extranonce1_len
 *     bytes of sessions[s].extranonce1 count, the rest are ignored.  Everything
 *     else about the job is checked as bm_job_header checks it.
 *   verdicts[i] belongs to submits[i]; the order is the caller's.  verdicts reuses
 *     bm_job_verdict_t.
 *   verdicts[i].hash = H of bm_job_header for that same job with extranonce1 =
 *     sessions[s].extranonce1, under the submission's (extranonce2, ntime, version:
 *     the full header field), with nonce in bytes 76..79, most significant byte
 *     first.
 *   verdicts[i].status = the OR of
 *     BM_SUBMIT_SHARE   hash <= sessions[s].target,
 *     BM_SUBMIT_BLOCK   hash <= bm_header_target_from_bits(job->nbits), as in
 *                       bm_job_verify_gpu (independent of SHARE; clear everywhere
 *                       for an nbits that does not decode),
 *     BM_SUBMIT_NTIME   ntime < ntime_lo || ntime > ntime_hi.  It is OR-ed in: the
 *                       hash and the other flags are computed all the same, and the
 *                       caller decides what to do with a share outside the window.
 *                       A caller who wants no window passes 0, 0xFFFFFFFF;
 *                       ntime_lo > ntime_hi flags every hashed entry,
 *     BM_SUBMIT_INVALID extranonce2 >= 2^(8 * extranonce2_size), or session >=
 *                       nsessions: nothing is hashed, hash is all 0xFF and status
 *                       is exactly this flag (no NTIME either),
 *     both compares over the full 256 bits.  verdicts[i].reserved = 0.
 *   out: n and how many verdicts carry each flag.
 *   n == 0 succeeds with a zero *out and touches no array (submits and verdicts may
 *     be NULL).  nsessions == 0 with n > 0 is legal (sessions may be NULL then):
 *     every entry is INVALID.
 *   Duplicate detection is bm_share_set_verify's, below: this call flags none.
 * BM_EINVAL: n > BM_MAX_JOB_SUBMITS or nsessions > BM_MAX_POOL_SESSIONS; a NULL
 * job or out (or ctx); NULL submits or verdicts with n > 0; NULL sessions with
 * nsessions > 0; extranonce1_len outside 1..8; a job bm_job_header refuses
 * otherwise; a rank context with world > 1.  On any failure `verdicts` and `out`
 * are untouched and the context stays usable.
 *
 * bm_pool_verify_cpu is pure CPU, no context: the specification.
 * bm_pool_verify_gpu gives byte-identical `verdicts` and `out`, on the first device
 * of ctx: one host-to-device copy (the job's tail template, its branch, the session
 * table and the submissions), one launch of pool_verify_kernel (one lane per
 * submission) and one copy back, on that device's stream.  The host then
 * recomputes entry 0, entry n - 1 and every entry flagged BLOCK with the CPU path
 * and returns BM_EINTERNAL on any difference: a tripwire, not the result.
 * bm_ctx_last_stats is left as the previous call left it.
 *
 * Out of scope: duplicate detection (bm_share_set_verify, below); vardiff policy; a
 * network Stratum server; several jobs in one call; splitting a batch over devices;
 * rank groups. */
#define BM_MAX_POOL_SESSIONS (1u << 20)
#define BM_SUBMIT_NTIME 8u            /* ntime outside [ntime_lo, ntime_hi]; hashed all the same */
typedef struct bm_pool_session {
    uint8_t extranonce1[8];           /* the first job->extranonce1_len bytes count */
    uint8_t target[32];               /* this session's share target, most significant byte first */
} bm_pool_session_t;                  /* 40 bytes */
typedef struct bm_pool_submit {
    uint64_t extranonce2;
    uint32_t ntime, nonce, version;   /* version: the full header field, as in bm_job_submit_t */
    uint32_t session;                 /* index into sessions[] */
} bm_pool_submit_t;                   /* 24 bytes, bm_job_submit_t's layout with reserved put to use */
typedef struct bm_pool_verify_result {
    uint64_t n;                       /* submissions */
    uint64_t shares, blocks, invalid, ntime; /* verdicts with BM_SUBMIT_SHARE / _BLOCK / _INVALID / _NTIME */
} bm_pool_verify_result_t;            /* 40 bytes */

int bm_pool_verify_cpu(const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                       const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                       bm_job_verdict_t* verdicts, bm_pool_verify_result_t* out);
int bm_pool_verify_gpu(bm_ctx_t* ctx, const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                       const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                       bm_job_verdict_t* verdicts, bm_pool_verify_result_t* out);

/* ---- duplicate-share detection: a set of header hashes ----------------------------
 * A pool that pays for shares must not pay twice for one.  A bm_share_set_t is an
 * opaque set of 32-byte header hashes with a fixed `capacity`; it is cleared by
 * the caller when its jobs retire (bm_share_set_clear).  bm_share_set_create makes
 * it on the first device of ctx, where it lives across calls; bm_share_set_create_cpu
 * makes it in host memory, with no context: the specification.
 *
 * bm_share_set_verify is bm_pool_verify_* plus the set.  It processes the batch as
 * if one submission at a time, in the caller's order:
 *   verdicts[i].hash and .status are exactly bm_pool_verify_cpu's for the same
 *     arguments, but for one more flag.
 *   A submission is ELIGIBLE when its status has BM_SUBMIT_SHARE or BM_SUBMIT_BLOCK
 *     and not BM_SUBMIT_INVALID.  BM_SUBMIT_NTIME does not matter: it stays
 *     advisory.  An ineligible submission never touches the set and is never
 *     flagged, however often it repeats.
 *   An eligible submission whose hash is in the set -- from an earlier call, or from
 *     a lower index of this batch -- gets BM_SUBMIT_DUPLICATE OR-ed into its status;
 *     its other bits and its hash are unchanged.
 *   An eligible submission whose hash is not in the set is recorded and not flagged:
 *     of equal hashes inside one batch exactly the lowest index is the unflagged one.
 *   The key is the hash, all 256 bits of it, not the tuple: the same work from two
 *     sessions that share an extranonce1 is a duplicate; the same (extranonce2,
 *     ntime, nonce, version) under different extranonce1 values is not.
 *   out: bm_pool_verify_result_t's five counts, then `duplicates` (verdicts with
 *     BM_SUBMIT_DUPLICATE), `recorded` (hashes this call added) and `count` (the
 *     set's size after the call).
 *   All or nothing: if the batch's new distinct hashes do not fit (count + new >
 *     capacity) the call returns BM_EFULL, `verdicts` and `out` are untouched, the set
 *     is exactly as before, and a later call behaves as if this one never happened.
 *   n == 0 is legal and changes nothing (*out: zeros and the set's count).
 * BM_EINVAL: everything bm_pool_verify_* refuses, a NULL set, and at creation a NULL
 * out (or ctx), a capacity of 0 or above BM_MAX_SHARE_SET, a rank context with
 * world > 1.  A device allocation that fails is BM_ENOMEM and leaves the context
 * usable.  On any failure `verdicts` and `out` are untouched and the set is as before.
 * Calls on one set are serialized by the caller, as calls on one context are (the
 * set uses its context's buffers and stream); two sets on one context are
 * independent.  bm_share_set_destroy(NULL) is fine; a device set is destroyed before
 * its context.  bm_share_set_clear forgets every hash (its jobs have retired);
 * bm_share_set_count reports the size and the capacity (either pointer may be NULL).
 *
 * The device set is an insert-only open-addressing table of 32-bit entry ids over a
 * key array keys[capacity] of 32-byte hashes.  The slot count is the smallest power
 * of two that is at least 2 * capacity and at least 16, and a hash's HOME SLOT is
 *     (its least significant 32 bits: hash[28..31] as a big-endian integer) mod slots
 * -- the least significant end, because an accepted share's most significant words
 * are zero by construction.  Probing is linear, wraps at the table's end and visits
 * at most `slots` slots; equality is over all 256 bits, never a tag.  One call is
 * bm_pool_verify_gpu's stage and pool_verify_kernel, then on the same stream
 *   share_insert_kernel   eligible lanes claim a slot with atomicCAS(EMPTY, 0x80000000
 *                         | i) or, meeting their own key, atomicMin their id into it:
 *                         the lowest index wins, or the persistent entry stays;
 *   share_resolve_kernel  a later launch: a lane whose slot holds its id is a winner,
 *                         any other eligible lane ORs in BM_SUBMIT_DUPLICATE; the
 *                         winners are counted with one atomicAdd per wave;
 *   one copy back (the verdicts and two control words), then
 *   share_commit_kernel   winners copy their key to keys[count + rank] and store that
 *                         id in their slot -- or share_rollback_kernel: winners store
 *                         EMPTY, which restores the table exactly (BM_EFULL).
 * No lane spins, retries or waits on another; the verdict bytes depend only on the
 * arguments and the set's contents.  The host tripwire is bm_pool_verify_gpu's, with
 * BM_SUBMIT_DUPLICATE masked off.  bm_ctx_last_stats is left alone.
 *
 * Out of scope: vardiff policy; a network Stratum server; expiring or removing
 * entries; sets over several devices or rank groups.  Several jobs in one call:
 * bm_share_set_verify_jobs, below. */
#define BM_SUBMIT_DUPLICATE 16u       /* an eligible hash the set already held (bm_share_set_verify only) */
#define BM_MAX_SHARE_SET (1u << 24)
typedef struct bm_share_set bm_share_set_t;
typedef struct bm_share_set_result {
    uint64_t n, shares, blocks, invalid, ntime; /* as bm_pool_verify_result_t */
    uint64_t duplicates;              /* verdicts with BM_SUBMIT_DUPLICATE */
    uint64_t recorded;                /* hashes this call added */
    uint64_t count;                   /* the set's size after the call */
} bm_share_set_result_t;              /* 64 bytes */

int bm_share_set_create(bm_ctx_t* ctx, size_t capacity, bm_share_set_t** out);
int bm_share_set_create_cpu(size_t capacity, bm_share_set_t** out);
void bm_share_set_destroy(bm_share_set_t* set);
int bm_share_set_clear(bm_share_set_t* set);
int bm_share_set_count(const bm_share_set_t* set, uint64_t* count, uint64_t* capacity);
int bm_share_set_verify(bm_share_set_t* set, const bm_job_t* job, const bm_pool_session_t* sessions, size_t nsessions,
                        const bm_pool_submit_t* submits, size_t n, uint32_t ntime_lo, uint32_t ntime_hi,
                        bm_job_verdict_t* verdicts, bm_share_set_result_t* out);

/* ---- pool-side share verification over several live jobs in one call ------------
 * A pool sends a new job every few tens of seconds and the earlier ones stay valid
 * until the next block, so a batch read off the sockets mixes the submissions of
 * several job ids.  bm_jobs_verify_* is bm_pool_verify_* with a table of jobs, each
 * with its own ntime window, and a job index per submission; all jobs share the
 * session table.
 *   verdicts[i] is byte for byte what bm_pool_verify_cpu(&jobs[j].job, sessions,
 *     nsessions, &that submission, 1, jobs[j].ntime_lo, jobs[j].ntime_hi, ...) gives,
 *     j = submits[i].job: jobs[j].job is read as bm_pool_verify_* reads a job
 *     (extranonce1 ignored, extranonce1_len 1..8 the size every session's
 *     extranonce1 has under THIS job: its first extranonce1_len bytes count).
 *   job >= njobs is BM_SUBMIT_INVALID exactly (hash all 0xFF, no other flag), as an
 *     unknown session and an oversized extranonce2 are.
 *   The order of `verdicts` is the caller's; `out` counts flags over the whole batch.
 *   n == 0 succeeds and touches no array.  njobs == 0 with n > 0 is legal (`jobs`
 *     may be NULL then): every entry is INVALID.
 *   Jobs may differ in every field: the sizes of both extranonces, the coinbase's
 *     length, the branch depth, nbits (decodable or not) and the window.
 * BM_EINVAL: njobs > BM_MAX_POOL_JOBS; NULL `jobs` with njobs > 0; any job that
 * bm_pool_verify_* refuses, whether or not a submission names it (all jobs are
 * checked before anything is staged); everything bm_pool_verify_* refuses otherwise,
 * a rank context with world > 1 among it.  On any failure `verdicts` and `out` are
 * untouched and the context stays usable.
 *
 * bm_jobs_verify_cpu is pure CPU, no context: the specification.
 * bm_jobs_verify_gpu gives byte-identical `verdicts` and `out`, on the first device
 * of ctx.  The host groups the batch by job while it stages it (one stable counting
 * sort, the scatter being the copy into the pinned buffer; the staged record carries
 * the submission's original index where the caller's has `job`) and cuts every group
 * into 64-lane workgroups, listed in a block table: no workgroup spans two jobs, so
 * every loop of jobs_verify_kernel is wave-uniform and a workgroup's job descriptor,
 * tail template and branch come through scalar loads.  One copy up (the job
 * descriptors, all tails, all branches, the session table, the staged submissions,
 * the block table), one launch, one copy back; verdicts are stored at the original
 * index.  The host recomputes entries 0 and n - 1, every entry flagged BLOCK and the
 * lowest-index submission of each job with the CPU path: BM_EINTERNAL on a difference.
 *
 * bm_share_set_verify_jobs is bm_share_set_verify over that verdict, on a CPU set or
 * a device set: eligibility, lowest index wins, the all-or-nothing BM_EFULL and the
 * poisoning are unchanged.  A set's key is the header hash, which already separates
 * jobs (their coinbase, branch, prevhash or nbits differ): one set may hold several
 * jobs' shares, is cleared by the caller when its jobs retire (bm_share_set_clear:
 * a new block height), and may be fed by bm_share_set_verify and
 * bm_share_set_verify_jobs alternately.  Two jobs[] entries with identical content
 * give identical hashes: the same tuple under both is a duplicate.
 *
 * Out of scope: vardiff policy (a session whose difficulty changed between jobs is
 * two session entries); a network Stratum server; splitting a batch over devices;
 * rank groups; expiring single jobs from a set. */
#define BM_MAX_POOL_JOBS 64
typedef struct bm_pool_job {
    bm_job_t job;                     /* as bm_pool_verify_* reads it: extranonce1 ignored, extranonce1_len 1..8 */
    uint32_t ntime_lo, ntime_hi;      /* this job's window, inclusive */
} bm_pool_job_t;
typedef struct bm_jobs_submit {
    uint64_t extranonce2;
    uint32_t ntime, nonce, version, session; /* as bm_pool_submit_t */
    uint32_t job;                     /* index into jobs[] */
    uint32_t reserved;                /* ignored */
} bm_jobs_submit_t;                   /* 32 bytes */

int bm_jobs_verify_cpu(const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions, size_t nsessions,
                       const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                       bm_pool_verify_result_t* out);
int bm_jobs_verify_gpu(bm_ctx_t* ctx, const bm_pool_job_t* jobs, size_t njobs, const bm_pool_session_t* sessions,
                       size_t nsessions, const bm_jobs_submit_t* submits, size_t n, bm_job_verdict_t* verdicts,
                       bm_pool_verify_result_t* out);
int bm_share_set_verify_jobs(bm_share_set_t* set, const bm_pool_job_t* jobs, size_t njobs,
                             const bm_pool_session_t* sessions, size_t nsessions, const bm_jobs_submit_t* submits,
                             size_t n, bm_job_verdict_t* verdicts, bm_share_set_result_t* out);

/* ---- share accounting: a per-account ledger ------------------------------------------
 * A pool verifies shares to pay for them: each accepted share is credited to an
 * account, weighted by the difficulty it was mined at, and the per-account reject
 * counts feed vardiff and ban rules.  A bm_ledger_t is an opaque table of `rows`
 * bm_ledger_row_t counters.  bm_ledger_create makes it on the first device of ctx,
 * where it lives across calls as a share set does; bm_ledger_create_cpu makes it in
 * host memory, with no context: the specification.  It holds tallies, not policy:
 * no vardiff rule and no payout scheme.
 *
 * bm_ledger_verify_jobs verifies a batch, de-duplicates it and credits it in one call.
 *   With a set, `verdicts` and the first eight fields of `out` are byte for byte
 *     bm_share_set_verify_jobs's for the same arguments and the same set, and the set
 *     changes as it does there.  With set == NULL they are bm_jobs_verify_cpu's, the
 *     three set fields (duplicates, recorded, count) zero.
 *   accounts[s] is the row of session s and weights[s] its weight (its difficulty in
 *     the caller's fixed-point unit).  accounts == NULL: session s -> row s.
 *     weights == NULL: 1 each.  Several sessions may share a row, with different
 *     weights.
 *   Every submission with session < nsessions falls into exactly one CLASS, by its
 *     final status; the first rule that applies decides:
 *       1. BM_SUBMIT_INVALID               -> invalid  (an unknown job among them)
 *       2. BM_SUBMIT_NTIME                 -> ntime
 *       3. BM_SUBMIT_DUPLICATE             -> duplicates
 *       4. BM_SUBMIT_SHARE or _BLOCK       -> accepted, and also blocks with _BLOCK
 *       5. otherwise                       -> above_target
 *     and the class word of row accounts[session] grows by one.  An accepted
 *     submission also adds weights[session] to the row's `work` (wrapping) and lowers
 *     its `best` to hash[0..7] read as a big-endian integer.  out->credited and
 *     out->work count the same credit over the whole call.
 *   A submission with session >= nsessions touches no row and counts in
 *     out->unattributed.  out->n = the call's row class deltas + unattributed.
 *   Every sum is an integer add or a min: the rows depend on the multiset of
 *     submissions, never on their order, and a device ledger holds the same bytes as
 *     a CPU ledger.  `work` is a sum over submissions, not weight x count per row.
 *   All or nothing: on any failure (BM_EINVAL, the set's BM_EFULL, a tripwire's
 *     BM_EINTERNAL, a failed allocation) `verdicts`, `out`, the ledger and the set are
 *     as before.  The exception is the share set's: a failure after the ledger
 *     kernel's launch (a HIP error, or control words that do not match) poisons the
 *     ledger until bm_ledger_clear -- every call on it but clear and destroy returns
 *     BM_EINTERNAL -- and, with a set, the set too, whose commit has been enqueued.
 *   n == 0 is legal and changes nothing (*out: zeros and the set's count).
 * bm_ledger_read copies rows [first, first + count) out; bm_ledger_drain does the
 * same and then resets exactly those rows to empty (seven zeros and best =
 * UINT64_MAX); bm_ledger_clear empties every row; bm_ledger_rows reports the size.
 * bm_ledger_set_peel sets the device kernel's combine rounds (below; 0..64, default
 * 64: a wave combines until no lane is pending); a CPU ledger accepts and ignores it.
 * BM_EINVAL: everything bm_share_set_verify_jobs or bm_jobs_verify_* refuses; a NULL
 * ledger; `rows` of 0 or above BM_MAX_LEDGER_ROWS; any accounts[s] >= rows (every
 * session is checked before anything is staged); accounts == NULL with nsessions >
 * rows; a device ledger with a CPU set, a CPU ledger with a device set, a set on
 * another context; first + count > rows; rounds > 64; a rank context with world > 1.
 * Calls on one ledger are serialized by the caller, as calls on one context are; two
 * ledgers on one context are independent.  bm_ledger_destroy(NULL) is fine; a device
 * ledger is destroyed before its context.
 *
 * The device call is bm_share_set_verify_jobs's (or bm_jobs_verify_gpu's) with
 * accounts[] and weights[] in the same single copy up, and ledger_credit_kernel
 * launched once the call can no longer be refused: after share_commit_kernel is
 * enqueued, or without a set after the tripwire.  One lane per staged record reads its
 * session, its final status and the first two hash words.  Before any global atomic a
 * wave combines, for up to `rounds` rounds: the row of its first pending lane, a ballot
 * of the lanes on that row, popcounts for the class counts, a wave sum for `work`, a
 * wave min for `best`, then that row's non-zero updates once (64-bit no-return
 * atomicAdd / atomicMin).  Lanes still pending issue their own atomics; rounds = 0 is
 * the per-lane form.  Nothing spins or waits on another lane.  The kernel also sums the
 * call's class totals and work into seven control words, which the host compares with
 * the totals of the verdicts: BM_EINTERNAL and a poisoned ledger on a difference.
 *
 * Out of scope: vardiff and payout policy; a network Stratum server; ledgers over
 * several devices or rank groups; single-job entries (njobs = 1 serves them). */
#define BM_MAX_LEDGER_ROWS (1u << 20)
typedef struct bm_ledger bm_ledger_t;
typedef struct bm_ledger_row {          /* 64 bytes; an empty row is seven zeros and best = UINT64_MAX */
    uint64_t accepted;      /* credited submissions */
    uint64_t blocks;        /* credited submissions with BM_SUBMIT_BLOCK */
    uint64_t above_target;  /* hashed, neither SHARE nor BLOCK */
    uint64_t ntime;         /* outside their job's window */
    uint64_t duplicates;    /* BM_SUBMIT_DUPLICATE */
    uint64_t invalid;       /* BM_SUBMIT_INVALID with a known session */
    uint64_t work;          /* sum of the session's weight over credited submissions, modulo 2^64 */
    uint64_t best;          /* min over credited submissions of hash[0..7] read as a big-endian u64 */
} bm_ledger_row_t;
typedef struct bm_ledger_result {       /* 88 bytes */
    uint64_t n, shares, blocks, invalid, ntime, duplicates, recorded, count; /* bm_share_set_result_t's; the last three 0 without a set */
    uint64_t credited;      /* submissions of class accepted */
    uint64_t unattributed;  /* session >= nsessions: no row was touched */
    uint64_t work;          /* this call's credited work, modulo 2^64 */
} bm_ledger_result_t;

int bm_ledger_create(bm_ctx_t* ctx, size_t rows, bm_ledger_t** out);
int bm_ledger_create_cpu(size_t rows, bm_ledger_t** out);
void bm_ledger_destroy(bm_ledger_t* ledger);
int bm_ledger_clear(bm_ledger_t* ledger);
int bm_ledger_rows(const bm_ledger_t* ledger, uint64_t* rows);
int bm_ledger_read(bm_ledger_t* ledger, size_t first, size_t count, bm_ledger_row_t* out);
int bm_ledger_drain(bm_ledger_t* ledger, size_t first, size_t count, bm_ledger_row_t* out);
int bm_ledger_set_peel(bm_ledger_t* ledger, uint32_t rounds);
int bm_ledger_verify_jobs(bm_ledger_t* ledger, bm_share_set_t* set /* or NULL */, const bm_pool_job_t* jobs,
                          size_t njobs, const bm_pool_session_t* sessions, size_t nsessions,
                          const uint32_t* accounts /* nsessions entries, or NULL */,
                          const uint64_t* weights /* nsessions entries, or NULL */, const bm_jobs_submit_t* submits,
                          size_t n, bm_job_verdict_t* verdicts, bm_ledger_result_t* out);

/* ---- sessions: a device-resident session table with vardiff retargeting ---------------
 * The sessions of a pool change slowly -- a connect, a disconnect, a retarget -- while
 * submissions arrive all the time.  A bm_sessions_t is an opaque table of `capacity`
 * slots that keeps what the pool calls take per session -- the bm_pool_session_t, the
 * account and the weight -- and a bm_session_state_t per slot.  bm_sessions_create makes
 * it on the first device of ctx, where it lives across calls as a share set and a ledger
 * do, so that a verify call copies no session up; bm_sessions_create_cpu makes it in host
 * memory, with no context: the specification.  Difficulty is a uint64_t in units of
 * 2^-32 ("fx"), the unit of the ledger's weights; T(d) = bm_target_from_difficulty_fx(d).
 *
 * bm_sessions_set: slot index[j] (index == NULL: slot j) becomes the session
 *   {init[j].extranonce1, target = T(difficulty_fx)} with account init[j].account and
 *   weight difficulty_fx, its state {difficulty_fx, since_ms = now_ms, accepted = 0,
 *   retargets = 0}.  difficulty_fx == 0 CLOSES the slot: target all zero (nothing is at
 *   or below it), weight 0, never evaluated by a retarget.  `count` is 1 + the highest
 *   index set since the last clear; a never-set slot below it is a closed slot with zero
 *   extranonce1 and account 0.  An index that appears twice in one call: the later entry
 *   wins.  All or nothing: an index >= capacity is BM_EINVAL and nothing changes.
 * bm_sessions_get: slots [first, first + count) as the three arrays the pool calls take
 *   and their states; any output may be NULL.  first + count may reach capacity (slots
 *   past the table's count read as closed, never-set slots).
 * bm_sessions_clear: count = 0, every slot never set; lifts poisoning (below).
 * bm_sessions_count: the count and the capacity (either pointer may be NULL, not both).
 *
 * bm_sessions_verify_jobs is bm_ledger_verify_jobs over the table: with sessions,
 *   accounts and weights as bm_sessions_get(0, count) returns them and nsessions = count,
 *   `verdicts`, `out`, the ledger and the set end up byte for byte as bm_ledger_verify_jobs
 *   leaves them; with ledger == NULL as if against a scratch ledger (no row anywhere
 *   changes).  TALLY: every submission of ledger class accepted (rule 4 above) with
 *   session < count also adds 1 to that slot's state.accepted.  All or nothing as
 *   bm_ledger_verify_jobs: on any refusal the table, the ledger, the set, `verdicts` and
 *   `out` are as before.  A failure after the tally's launch (a HIP error, or a control
 *   word that does not match out->credited) POISONS the table until bm_sessions_clear:
 *   every call on it but clear, count and destroy returns BM_EINTERNAL.
 *   BM_EINVAL: everything bm_ledger_verify_jobs refuses; a CPU table with a device ledger
 *   or set or the reverse; objects on another context; any account of a slot below count
 *   >= the ledger's rows.
 *
 * bm_sessions_retarget applies one vardiff step at now_ms to every slot below count.  All
 *   arithmetic is exact and unsigned; nothing is floating point.  For an OPEN slot
 *   (difficulty_fx != 0) with state {old, since_ms, accepted, retargets}:
 *     1. elapsed = now_ms >= since_ms ? now_ms - since_ms : 0.
 *     2. The slot is EVALUATED when elapsed >= window_ms, or burst != 0 && accepted >= burst.
 *     3. D = max(elapsed, 1), N = min(accepted, 2^32 - 1) * target_ms,
 *        ideal = floor(old * N / D)                                  (a 128-bit product).
 *     4. new = min(max(ideal, max(1, floor(old / max_down))), sat64(old * max_up)).
 *     5. new is clamped to [min_difficulty_fx, max_difficulty_fx].
 *     6. The slot is UNCHANGED when |new - old| * 1000 <= old * band_permille.
 *     7. Every evaluated slot gets since_ms = now_ms, accepted = 0.
 *     8. A changed slot also gets difficulty_fx = weight = new, target = T(new),
 *        retargets += 1,
 *     9. and yields one entry of `changes`, which is ascending by session.
 *   *out counts the open, evaluated and changed slots, and the changed ones with new > old
 *   (raised) and new < old (lowered).  changed > cap: BM_EFULL; *out still holds the exact
 *   counts, `changes` is untouched and the table is exactly as before, windows and
 *   counters included.  target_ms is 1..2^32-1, 1 <= min <= max, max_up and max_down >= 1,
 *   band_permille <= 1000: BM_EINVAL otherwise, and for a NULL table, policy or out, or
 *   NULL changes with cap != 0.
 *   A retarget takes effect at the next verify call: shares of jobs sent before the
 *   caller's mining.set_difficulty are judged at the new difficulty (real pools keep a
 *   grace period), so a few above-target rejects may follow a raise.
 *
 * On the device the table is four arrays -- bm_pool_session_t[capacity], uint32_t
 * accounts[capacity], uint64_t weights[capacity], the layouts jobs_verify_kernel and
 * ledger_credit_kernel read, and the states -- and the host keeps a mirror of the first
 * three (the verify tripwire and bm_sessions_get read it; states are read back).
 * bm_sessions_set resolves repeated indices on the host and scatters the staged records
 * (sessions_set_kernel: one lane per record, no two writers of a slot).  The verify call is
 * bm_ledger_verify_jobs's with the table's arrays neither staged nor copied: the existing
 * kernels get the table's pointers, and sessions_tally_kernel runs where
 * ledger_credit_kernel runs, one lane per staged record, one no-return atomicAdd per
 * accepted lane (vardiff itself keeps a session at a few shares per window) and one per
 * wave into a control word that the host compares with out->credited.
 * sessions_retarget_kernel takes one lane per slot below count and runs twice: a decide
 * pass that only reads the table, counts, and compacts the changes into a list (only
 * changed lanes run the 256-bit by 64-bit division), and, once the host has seen that the
 * list fits and has recomputed every target in it (BM_EINTERNAL and a poisoned table on a
 * difference), an apply pass that rewrites the slots.  The host sorts the list by session
 * and applies it to its mirror.
 *
 * Calls on one table are serialized by the caller; a device table is destroyed before its
 * context; bm_sessions_destroy(NULL) is fine.  Out of scope: the grace period above; the
 * single-job and per-call-array entry points taking a table; tables over several devices
 * or rank groups (BM_EINVAL); a network Stratum server; payout policy. */
typedef struct bm_sessions bm_sessions_t;
typedef struct bm_session_init {        /* 24 bytes */
    uint8_t extranonce1[8];
    uint64_t difficulty_fx;             /* 0: the slot is closed */
    uint32_t account, reserved;
} bm_session_init_t;
typedef struct bm_session_state {       /* 32 bytes */
    uint64_t difficulty_fx;             /* 0: closed */
    uint64_t since_ms;                  /* start of the slot's window */
    uint64_t accepted;                  /* accepted submissions since then */
    uint64_t retargets;                 /* changes since the slot was set */
} bm_session_state_t;
typedef struct bm_vardiff_policy {      /* 48 bytes */
    uint64_t target_ms;                 /* the time one share should take, 1..2^32-1 */
    uint64_t window_ms;                 /* a slot is evaluated once its window is this long */
    uint64_t min_difficulty_fx, max_difficulty_fx;
    uint32_t burst;                     /* or once it has this many accepted shares; 0: off */
    uint32_t band_permille;             /* a change within old * band / 1000 is none, 0..1000 */
    uint32_t max_up, max_down;          /* one step multiplies by at most max_up, divides by at most max_down */
} bm_vardiff_policy_t;
typedef struct bm_vardiff_change {      /* 56 bytes */
    uint32_t session, reserved;
    uint64_t old_fx, new_fx;
    uint8_t target[32];                 /* T(new_fx), most significant byte first */
} bm_vardiff_change_t;
typedef struct bm_vardiff_result {      /* 40 bytes */
    uint64_t open, evaluated, changed, raised, lowered;
} bm_vardiff_result_t;

int bm_sessions_create(bm_ctx_t* ctx, size_t capacity, bm_sessions_t** out);   /* capacity 1..BM_MAX_POOL_SESSIONS */
int bm_sessions_create_cpu(size_t capacity, bm_sessions_t** out);
void bm_sessions_destroy(bm_sessions_t* table);
int bm_sessions_clear(bm_sessions_t* table);
int bm_sessions_count(const bm_sessions_t* table, uint64_t* count, uint64_t* capacity);
int bm_sessions_set(bm_sessions_t* table, const uint32_t* index /* k entries, or NULL: 0..k-1 */, size_t k,
                    const bm_session_init_t* init, uint64_t now_ms);
int bm_sessions_get(bm_sessions_t* table, size_t first, size_t count, bm_pool_session_t* sessions,
                    uint32_t* accounts, uint64_t* weights, bm_session_state_t* state);
int bm_sessions_verify_jobs(bm_sessions_t* table, bm_ledger_t* ledger /* or NULL */, bm_share_set_t* set /* or NULL */,
                            const bm_pool_job_t* jobs, size_t njobs, const bm_jobs_submit_t* submits, size_t n,
                            bm_job_verdict_t* verdicts, bm_ledger_result_t* out);
int bm_sessions_retarget(bm_sessions_t* table, uint64_t now_ms, const bm_vardiff_policy_t* policy,
                         bm_vardiff_change_t* changes, size_t cap, bm_vardiff_result_t* out);

/* Batched bitcoin.Hash (hash.go:11-15) on the first device of ctx:
 * out[i] = Hash(msg, nonces[i]) for i < n. */
int bm_hash_gpu(bm_ctx_t* ctx, const uint8_t* msg, size_t len, const uint64_t* nonces, size_t n,
                uint64_t* out);

/* ---- measurement (used by bench.py; does not change results) ---------- */

#define BM_MAX_LAUNCH_STATS 64

typedef struct bm_launch_stat {
    int32_t device;       /* index into the context's device list */
    int32_t p;            /* byte position of the last digit in its SHA block */
    int32_t nbv;          /* varying blocks per task (1 or 2) */
    int32_t pad_block;    /* 1 when a constant padding block follows (the generic kernel: its
                             K + W from kernargs); 2 + K: the same, run by a kernel with that
                             block's constants folded in, after K whole prefix blocks (2: a
                             one-block message, search_kernel_padc; 3..17: K = 1..15,
                             search_kernel_padk, whose entering state is the midstate) */
    int32_t digits;       /* decimal digits of every nonce in the launch */
    int32_t inner_digits; /* digits iterated by each thread's inner loop */
    uint64_t nonces;      /* nonces the launch is responsible for */
    uint32_t grid;        /* workgroups launched (256 threads each) */
    uint32_t tasks_per_thread; /* approx. tasks per lane (dynamic dequeue) */
    double ms;            /* launch duration from HIP events on its stream (0 if timing off) */
    double clock_ghz;     /* average shader clock over the launch: s_memtime cycles over
                             s_memrealtime ticks stamped by workgroup 0 (timing on, and a
                             library built with BM_CLOCK_PROBE=1; 0 otherwise) */
} bm_launch_stat_t;

/* How the last search combined its partials (bm_stats_t.combine_used). */
#define BM_COMBINED_NONE 0  /* nothing to combine (empty range) */
#define BM_COMBINED_RCCL 1  /* one RCCL allgather (the devices of the context, or the ranks of its group) */
#define BM_COMBINED_HOST 2  /* device-to-host copies of every device's partial */
#define BM_COMBINED_LOCAL 3 /* a rank context outside a group: this rank's own partial */
#define BM_MAX_STAT_DEVICES 16

typedef struct bm_stats {
    uint32_t launches;     /* search-kernel launches of the last call */
    uint32_t recorded;     /* entries filled in launch[] (<= BM_MAX_LAUNCH_STATS) */
    double wall_ms;        /* host wall time of the last bm_search_gpu call */
    double kernel_ms;      /* SUM of launch durations (timing on); launches on
                              different streams overlap, so this can exceed span_ms */
    double span_ms;        /* first launch's start to the last launch's end on
                              one device (timing on; max over devices) */
    uint64_t nonces;       /* nonces this process scanned in the last call */
    int32_t combine_used;  /* BM_COMBINED_*: how the partials were combined */
    int32_t rccl_status;   /* the RCCL failure this context fell back from or
                              stopped on (BM_ERCCL / BM_ETIMEDOUT), 0 if none */
    uint32_t devices;      /* entries of dev_nonces / dev_span_ms / dev_rccl_* */
    uint32_t reserved;
    uint64_t dev_nonces[BM_MAX_STAT_DEVICES];  /* nonces each device of the context scanned */
    double dev_span_ms[BM_MAX_STAT_DEVICES];   /* each device's first operation to the end of
                                                  its reduction (timing on) */
    /* What RCCL itself reports about the communicator the last call's
     * combine ran over (combine_used = BM_COMBINED_RCCL; otherwise 0 / -1),
     * so a multi-GPU measurement can show that the collective really spanned
     * N ranks on N devices: */
    int32_t rccl_nranks;   /* ncclCommCount: ranks in the communicator */
    int32_t rccl_rank;     /* ncclCommUserRank of this process's (first) device */
    int32_t dev_rccl_rank[BM_MAX_STAT_DEVICES];   /* ncclCommUserRank of each device of the context */
    int32_t dev_rccl_device[BM_MAX_STAT_DEVICES]; /* ncclCommCuDevice: the HIP device RCCL runs that
                                                     rank on */
    /* ABI 7: what the combine and the start of a call cost, so a multi-GPU
     * line can be read without a rerun. */
    int32_t rccl_version;      /* ncclGetVersion of the RCCL the library runs on (e.g. 22703); 0 if
                                  it cannot say.  Filled on every call. */
    int32_t start_threads;     /* host threads that submitted the devices' work (1, or one per
                                  device of a multi-device context) */
    double rccl_init_ms;       /* host time the current communicator took to form: ncclCommInitAll
                                  (one process), or bm_ctx_join_rank's init, which includes waiting
                                  for every rank to arrive; 0 without a communicator */
    double rccl_allgather_ms;  /* the last call's allgather, from HIP events around it on the
                                  (first) device's stream (timing on): it starts when this
                                  device's own work is done, so it includes the wait for the
                                  slowest peer; max over the devices of a context; 0 otherwise */
    double combine_ms;         /* host time from the end of this process's own work (its devices'
                                  reductions, seen on the host) to the end of the combine: the wait
                                  for the peers, the allgather or host copies, the result copy.
                                  Without timing or balance in a one-process context, from the
                                  enqueue of the combine instead */
    double dev_allgather_ms[BM_MAX_STAT_DEVICES]; /* each device's allgather event pair (timing on) */
    double dev_start_ms[BM_MAX_STAT_DEVICES];     /* host time at which each device's first
                                  operation of the call was submitted, relative to the earliest
                                  device's (its stream is idle then, so this is when it starts);
                                  set_balance measures rates from that common start (timing or
                                  balance on) */
    bm_launch_stat_t launch[BM_MAX_LAUNCH_STATS];
} bm_stats_t;

/* Enable per-launch HIP event timing (default off). */
int bm_ctx_set_timing(bm_ctx_t* ctx, int enable);
int bm_ctx_last_stats(const bm_ctx_t* ctx, bm_stats_t* out);

/* How much of the range the last bm_search_target_gpu handed out to waves.
 * Summed over a device's launches; each launch contributes min(its final
 * dequeue counter, its task count) x nonces per task, capped at the launch's
 * own nonce count (read back from the counters the kernels use anyway).  An
 * upper bound on the nonces hashed: equal to the range size when nothing was
 * found, and at least nonce - lower + 1 on the device that holds the hit.
 * Zero after a failed call or an empty range. */
typedef struct bm_target_stats {
    uint64_t nonces_dispatched;                    /* all devices */
    uint64_t dev_dispatched[BM_MAX_STAT_DEVICES];  /* each device of the context */
    uint32_t devices;                              /* entries of dev_dispatched */
    uint32_t reserved;
} bm_target_stats_t;
int bm_ctx_last_target_stats(const bm_ctx_t* ctx, bm_target_stats_t* out);

/* Occupancy override for the search kernels: workgroups of 256 threads kept
 * resident per CU (0 = ask the runtime).  Exposed for tuning. */
int bm_ctx_set_blocks_per_cu(bm_ctx_t* ctx, int blocks_per_cu);

/* Planner knob: a digit-count segment whose high digits take more than
 * max_windows distinct values is run as ONE launch whose tasks re-compress
 * the block holding them (nbv = 2) instead of one launch per value
 * (default 64; 0 forces nbv = 2 wherever the digits straddle a block).
 * Results do not depend on it. */
int bm_ctx_set_max_windows(bm_ctx_t* ctx, int max_windows);

/* Nonces per kernel task = 10^digits, the digits a lane steps in its inner
 * loop.  0 (default): per launch, 100-nonce tasks, or 10-nonce tasks for a
 * launch too small to give every resident lane two 100-nonce tasks; 1 or 2:
 * forced (tests use it to cover both loop shapes at small sizes).  Results do
 * not depend on it. */
int bm_ctx_set_task_digits(bm_ctx_t* ctx, int digits);

/* How a context combines its per-device 16-byte partials:
 * BM_COMBINE_AUTO (default): RCCL allgather when the context has > 1
 * distinct device, a plain device-to-host copy otherwise; BM_COMBINE_RCCL:
 * always RCCL (also for one device: exercises the collective path on a
 * single GPU; BM_EINVAL on a context that lists a device twice);
 * BM_COMBINE_HOST: device-to-host copies of every partial, no RCCL.
 * When RCCL fails at run time (ncclCommInitAll or the allgather), the
 * context aborts its communicators, combines that call and every later one
 * by host copies, and reports it: combine_used = BM_COMBINED_HOST,
 * rccl_status = BM_ERCCL.  The answer is the same either way. */
#define BM_COMBINE_AUTO 0
#define BM_COMBINE_RCCL 1
#define BM_COMBINE_HOST 2
int bm_ctx_set_combine(bm_ctx_t* ctx, int mode);

/* ---- the multi-GPU range partitioner (results never depend on it) -----
 * A search's range is cut into one contiguous piece per slot: the devices of
 * a context, or the ranks of an RCCL group.  Default: near-equal pieces.
 * GPUs run this kernel at different clocks (PMC put it at 2.09-2.23 GHz on
 * the MI355Xs measured), and a search ends when its slowest slot does;
 * pieces in proportion to each slot's speed end together.
 *
 * bm_ctx_set_split: n integer shares, one per slot (n = devices of the
 *   context, or world of a rank context), each >= 1; slot i gets the nonces
 *   [lower + B_i, lower + B_{i+1} - 1] with B_i = floor(count * (s_0 + ... +
 *   s_{i-1}) / S), S = sum of the shares (exact integer arithmetic, so every
 *   rank of a group derives the same pieces from the same shares).  Every
 *   rank of a group must set the same shares.  n = 0: back to near-equal.
 * bm_ctx_set_balance: a multi-device context sets its own shares after each
 *   search in which every device's piece held >= 2^30 nonces: each device's
 *   nonces over the time from the call's common start (the earliest device's
 *   first operation; bm_stats_t.dev_start_ms) to its reduction, scaled so the
 *   fastest device has 65536 -- a device that starts late gets a smaller
 *   piece.  Each device's work is submitted from a host thread of its own, so
 *   the starts are close anyway.  BM_EINVAL on a rank context of more than
 *   one rank: a rank sees only its own device, so a group exchanges its rates
 *   itself and calls bm_ctx_set_split (bench.py does, over its rendezvous).
 * bm_ctx_get_split: the shares the next search will use (*n = 0: near-equal).
 * bm_split_range: the pieces themselves, pure CPU: lo[i] > hi[i] marks an
 *   empty piece; shares = NULL gives the near-equal pieces. */
#define BM_MAX_SLOTS 1024
int bm_ctx_set_split(bm_ctx_t* ctx, const uint32_t* shares, int n);
int bm_ctx_get_split(const bm_ctx_t* ctx, uint32_t* shares, int cap, int* n);
int bm_ctx_set_balance(bm_ctx_t* ctx, int enable);
int bm_split_range(uint64_t lower, uint64_t upper, const uint32_t* shares, int n, uint64_t* lo, uint64_t* hi);

/* ---- test entries (do not change search results) ---------------------- */

/* Lexicographic (hash, nonce) min of n partials on the first device of ctx,
 * computed by the reductions the search runs above its per-lane scans
 * (ds_swizzle/readlane wave min, LDS workgroup min, second-pass kernel).
 * Pins the tie rule (equal hashes -> smallest nonce, miner.go:61) on inputs
 * the search itself cannot produce.  n <= BM_MAX_REDUCE. */
#define BM_MAX_REDUCE (1u << 24)
int bm_reduce_gpu(bm_ctx_t* ctx, const bm_result_t* parts, size_t n, bm_result_t* out);

/* Make every later bm_search_gpu fail with BM_EINTERNAL after enqueueing
 * `launches` search launches (-1: off).  Exercises the failure path: the
 * call drains what it queued and the context stays usable.  On a joined
 * rank context the failure reaches the whole group through the status word
 * of the allgather (the others return BM_EPEER). */
int bm_ctx_set_test_fault(bm_ctx_t* ctx, int launches);

/* Make RCCL fail on purpose (0: off): 1 = the next communicator set-up
 * (ncclCommInitAll, or bm_ctx_join_rank), 2 = every allgather, before it is
 * enqueued.  A multi-device context then falls back to host copies; a
 * joined rank context fails the call (at world 1 only: a real group's peers
 * would wait for it until their peer timeout).  3 = a joined rank context's
 * allgather succeeds but its last slot carries a failure status, as a failed
 * peer's slot does: the call returns BM_EPEER and the group stays joined. */
int bm_ctx_set_test_rccl_fault(bm_ctx_t* ctx, int where);

/* Hold back the submission of device `device`'s work (an index into the
 * context's device list) by delay_us microseconds at the start of every later
 * search (0: off): a late-starting GPU, on demand, for the balance test. */
int bm_ctx_set_test_start_delay(bm_ctx_t* ctx, int device, int delay_us);

/* ---- host-side plan introspection (pure CPU; used by the CPU tests) ---- */

/* One kernel launch of a search: every nonce n = nonce_base + v with v in
 * [vlo, vhi] has exactly `digits` decimal digits and a message whose bytes
 * before the varying SHA-256 block(s) are constant (folded into mid[]). */
typedef struct bm_segment {
    int32_t p;            /* byte index of the last digit inside the last varying block */
    int32_t nbv;          /* varying blocks (1, or 2 when a task also re-compresses the block before) */
    int32_t pad_block;    /* 1: a constant padding block follows the varying block */
    int32_t digits;       /* decimal digits of every nonce */
    int32_t nd;           /* digits of v that live in the varying block(s) */
    int32_t max_inner;    /* max digits the inner loop may iterate (all in one word) */
    uint64_t vlo, vhi;    /* inclusive range of v */
    uint64_t nonce_base;  /* nonce = nonce_base + v */
    uint32_t mid[8];      /* SHA-256 state before the varying block(s) */
    uint32_t tmpl[32];    /* varying block words, big-endian, digit bytes = '0' */
    uint32_t pad_w[16];   /* words of the constant padding block (pad_block) */
} bm_segment_t;

/* Fill up to cap segments for (msg, [lower, upper]); *nseg gets the count
 * needed (call with cap = 0 to size). */
int bm_plan_segments(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                     bm_segment_t* segs, int cap, int* nseg);
/* Same with an explicit max_windows (see bm_ctx_set_max_windows). */
int bm_plan_segments_ex(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, int max_windows,
                        bm_segment_t* segs, int cap, int* nseg);

#ifdef __cplusplus
}
#endif
#endif /* BTCMINER_H */
