"""ctypes binding of libbtcminer.so (C ABI: include/btcminer.h).

The library is built in-tree (``make -C distributed_bitcoin_minter_amd/csrc``)
and loaded from this package directory.  There is no fallback: if the
library is missing, or there is no gfx950 device, calls raise.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BTCMINER_LIB overrides the library path (used to A/B kernel build variants;
# they must be built from the same ABI version)
LIB_PATH = os.environ.get("BTCMINER_LIB") or os.path.join(_HERE, "libbtcminer.so")

BM_OK = 0
BM_EINVAL = -1
BM_ENODEV = -2
BM_EHIP = -3
BM_ERCCL = -4
BM_ENOMEM = -5
BM_EINTERNAL = -6
BM_EPEER = -7
BM_ETIMEDOUT = -8
BM_EFULL = -9
BM_MAX_LAUNCH_STATS = 64
BM_MAX_STAT_DEVICES = 16
BM_RCCL_ID_BYTES = 128
BM_ABI_VERSION = 7
BM_DEFAULT_PEER_TIMEOUT_MS = 600_000
BM_COMBINE_AUTO, BM_COMBINE_RCCL, BM_COMBINE_HOST = 0, 1, 2
# bm_stats_t.combine_used
BM_COMBINED_NONE, BM_COMBINED_RCCL, BM_COMBINED_HOST, BM_COMBINED_LOCAL = 0, 1, 2, 3
COMBINED_NAMES = {0: "none", 1: "rccl", 2: "host", 3: "local"}
U64_MAX = (1 << 64) - 1

c_u64 = ctypes.c_uint64
c_u32 = ctypes.c_uint32
c_i32 = ctypes.c_int32


class Result(ctypes.Structure):
    _fields_ = [("hash", c_u64), ("nonce", c_u64)]


class LaunchStat(ctypes.Structure):
    _fields_ = [("device", c_i32), ("p", c_i32), ("nbv", c_i32), ("pad_block", c_i32), ("digits", c_i32),
                ("inner_digits", c_i32), ("nonces", c_u64), ("grid", c_u32), ("tasks_per_thread", c_u32),
                ("ms", ctypes.c_double), ("clock_ghz", ctypes.c_double)]


class Stats(ctypes.Structure):
    _fields_ = [("launches", c_u32), ("recorded", c_u32), ("wall_ms", ctypes.c_double),
                ("kernel_ms", ctypes.c_double), ("span_ms", ctypes.c_double), ("nonces", c_u64),
                ("combine_used", c_i32), ("rccl_status", c_i32), ("devices", c_u32), ("reserved", c_u32),
                ("dev_nonces", c_u64 * BM_MAX_STAT_DEVICES), ("dev_span_ms", ctypes.c_double * BM_MAX_STAT_DEVICES),
                ("rccl_nranks", c_i32), ("rccl_rank", c_i32), ("dev_rccl_rank", c_i32 * BM_MAX_STAT_DEVICES),
                ("dev_rccl_device", c_i32 * BM_MAX_STAT_DEVICES),
                # ABI 7: the RCCL version, the communicator's set-up time, the allgather's
                # event pair and each device's start against the earliest device's
                ("rccl_version", c_i32), ("start_threads", c_i32), ("rccl_init_ms", ctypes.c_double),
                ("rccl_allgather_ms", ctypes.c_double), ("combine_ms", ctypes.c_double),
                ("dev_allgather_ms", ctypes.c_double * BM_MAX_STAT_DEVICES),
                ("dev_start_ms", ctypes.c_double * BM_MAX_STAT_DEVICES),
                ("launch", LaunchStat * BM_MAX_LAUNCH_STATS)]


class TargetResult(ctypes.Structure):
    _fields_ = [("hash", c_u64), ("nonce", c_u64), ("found", c_i32), ("reserved", c_i32)]


class TargetStats(ctypes.Structure):
    _fields_ = [("nonces_dispatched", c_u64), ("dev_dispatched", c_u64 * BM_MAX_STAT_DEVICES),
                ("devices", c_u32), ("reserved", c_u32)]


BM_MAX_HITS = 1 << 22


class HitsResult(ctypes.Structure):
    _fields_ = [("hash", c_u64), ("nonce", c_u64), ("count", c_u64), ("stored", c_u64)]


class HeaderResult(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("nonce", c_u32), ("found", c_i32)]


HEADER_BYTES = 80
U32_MAX = (1 << 32) - 1
U256_MAX = (1 << 256) - 1
BM_MAX_HEADER_HASHES = 1 << 24
BM_MAX_HEADER_HITS = 1 << 20
BM_MAX_HEADER_VERSIONS = 64
BIP320_MASK = 0x1fffe000  # the version bits BIP 320 leaves to the miner


class HeaderHit(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("nonce", c_u32), ("reserved", c_u32)]


class HeaderHitsResult(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("nonce", c_u32), ("reserved", c_u32), ("count", c_u64),
                ("stored", c_u64)]


class HeaderVersionsResult(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("nonce", c_u32), ("version_index", c_u32), ("version", c_u32),
                ("found", c_i32)]


class HeaderVersionHit(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("nonce", c_u32), ("version_index", c_u32), ("version", c_u32),
                ("reserved", c_u32)]


class HeaderVersionsHitsResult(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("nonce", c_u32), ("version_index", c_u32), ("version", c_u32),
                ("reserved", c_u32), ("count", c_u64), ("stored", c_u64)]


BM_MAX_JOB_COINBASE = 1 << 16
BM_MAX_JOB_BRANCH = 32
BM_MAX_JOB_HEADERS = 4096
DIFF1_TARGET = 0xffff << 208  # the target of difficulty 1 (nbits 1d00ffff)


class JobStruct(ctypes.Structure):
    """bm_job_t: the pointers are borrowed (Job keeps the buffers alive)."""
    _fields_ = [("coinb1", ctypes.c_char_p), ("coinb1_len", ctypes.c_size_t),
                ("extranonce1", ctypes.c_char_p), ("extranonce1_len", ctypes.c_size_t),
                ("extranonce2_size", c_u32),
                ("coinb2", ctypes.c_char_p), ("coinb2_len", ctypes.c_size_t),
                ("branch", ctypes.c_char_p), ("nbranch", ctypes.c_size_t),
                ("prevhash", ctypes.c_uint8 * 32), ("version", c_u32), ("nbits", c_u32)]


class JobShare(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("extranonce2", c_u64), ("nonce", c_u32), ("ntime", c_u32),
                ("version_index", c_u32), ("version", c_u32), ("is_block", c_u32), ("reserved", c_u32)]


class JobSharesResult(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("extranonce2", c_u64), ("nonce", c_u32), ("version_index", c_u32),
                ("version", c_u32), ("reserved", c_u32), ("count", c_u64), ("stored", c_u64), ("headers", c_u64)]


BM_MAX_JOB_SUBMITS = 1 << 20
BM_SUBMIT_SHARE, BM_SUBMIT_BLOCK, BM_SUBMIT_INVALID = 1, 2, 4


class JobSubmit(ctypes.Structure):
    """bm_job_submit_t: version is the full header version field."""
    _fields_ = [("extranonce2", c_u64), ("ntime", c_u32), ("nonce", c_u32), ("version", c_u32), ("reserved", c_u32)]


class JobVerdict(ctypes.Structure):
    """bm_job_verdict_t: hash most significant byte first, status the OR of
    BM_SUBMIT_SHARE / BM_SUBMIT_BLOCK / BM_SUBMIT_INVALID."""
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("status", c_u32), ("reserved", c_u32)]

    @property
    def value(self) -> int:
        """The hash as an integer (all ones for an INVALID entry)."""
        return int.from_bytes(bytes(self.hash), "big")

    @property
    def is_share(self) -> bool:
        return bool(self.status & BM_SUBMIT_SHARE)

    @property
    def is_block(self) -> bool:
        return bool(self.status & BM_SUBMIT_BLOCK)

    @property
    def is_invalid(self) -> bool:
        return bool(self.status & BM_SUBMIT_INVALID)

    @property
    def is_ntime(self) -> bool:
        """ntime outside the window (Context.verify_pool_submits only)."""
        return bool(self.status & 8)  # BM_SUBMIT_NTIME

    @property
    def is_duplicate(self) -> bool:
        """An eligible hash the share set already held (ShareSet.verify only)."""
        return bool(self.status & 16)  # BM_SUBMIT_DUPLICATE


class JobVerifyResult(ctypes.Structure):
    _fields_ = [("n", c_u64), ("shares", c_u64), ("blocks", c_u64), ("invalid", c_u64)]


BM_MAX_POOL_SESSIONS = 1 << 20
BM_SUBMIT_NTIME = 8


class PoolSessionStruct(ctypes.Structure):
    """bm_pool_session_t: the first extranonce1_len bytes of extranonce1 count;
    target most significant byte first."""
    _fields_ = [("extranonce1", ctypes.c_uint8 * 8), ("target", ctypes.c_uint8 * 32)]


class PoolSession:
    """One connection of a pool: its extranonce1 (1..8 bytes, the size the job
    states) and its share target as an integer."""
    __slots__ = ("extranonce1", "target")

    def __init__(self, extranonce1: bytes, target: int):
        if not isinstance(extranonce1, (bytes, bytearray)) or not 1 <= len(extranonce1) <= 8:
            raise ValueError(f"extranonce1 must be 1..8 bytes, got {extranonce1!r}")
        if not isinstance(target, int) or isinstance(target, bool) or not 0 <= target < 1 << 256:
            raise ValueError("target must be in 0..2^256-1")
        self.extranonce1, self.target = bytes(extranonce1), target

    def __repr__(self):
        return f"PoolSession({self.extranonce1!r}, {self.target:#x})"

    def __eq__(self, other):
        return isinstance(other, PoolSession) and (self.extranonce1, self.target) == (other.extranonce1, other.target)

    def __hash__(self):
        return hash((self.extranonce1, self.target))


class PoolSubmit(ctypes.Structure):
    """bm_pool_submit_t: bm_job_submit_t with the session index where that one
    has `reserved`; version is the full header version field."""
    _fields_ = [("extranonce2", c_u64), ("ntime", c_u32), ("nonce", c_u32), ("version", c_u32), ("session", c_u32)]


class PoolVerifyResult(ctypes.Structure):
    _fields_ = [("n", c_u64), ("shares", c_u64), ("blocks", c_u64), ("invalid", c_u64), ("ntime", c_u64)]


BM_SUBMIT_DUPLICATE = 16
BM_MAX_SHARE_SET = 1 << 24


class ShareSetResult(ctypes.Structure):
    """bm_share_set_result_t: PoolVerifyResult's counts, then the verdicts flagged
    DUPLICATE, the hashes the call added and the set's size after it."""
    _fields_ = [("n", c_u64), ("shares", c_u64), ("blocks", c_u64), ("invalid", c_u64), ("ntime", c_u64),
                ("duplicates", c_u64), ("recorded", c_u64), ("count", c_u64)]


BM_MAX_POOL_JOBS = 64


class PoolJobStruct(ctypes.Structure):
    """bm_pool_job_t: a job as the pool calls read it, and its ntime window."""
    _fields_ = [("job", JobStruct), ("ntime_lo", c_u32), ("ntime_hi", c_u32)]


class JobsSubmit(ctypes.Structure):
    """bm_jobs_submit_t: PoolSubmit with the index of the submission's job."""
    _fields_ = [("extranonce2", c_u64), ("ntime", c_u32), ("nonce", c_u32), ("version", c_u32), ("session", c_u32),
                ("job", c_u32), ("reserved", c_u32)]


BM_MAX_LEDGER_ROWS = 1 << 20
BM_LEDGER_NO_BEST = (1 << 64) - 1


class LedgerRow(ctypes.Structure):
    """bm_ledger_row_t: one account's tallies.  An empty row is seven zeros and
    best = 2^64 - 1."""
    _fields_ = [("accepted", c_u64), ("blocks", c_u64), ("above_target", c_u64), ("ntime", c_u64),
                ("duplicates", c_u64), ("invalid", c_u64), ("work", c_u64), ("best", c_u64)]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)

    @property
    def rejected(self) -> int:
        """Every submission of the row that was not credited."""
        return self.above_target + self.ntime + self.duplicates + self.invalid


class LedgerResult(ctypes.Structure):
    """bm_ledger_result_t: ShareSetResult's counts (the last three 0 without a
    set), then the call's credited submissions, those of unknown sessions and the
    credited work."""
    _fields_ = [("n", c_u64), ("shares", c_u64), ("blocks", c_u64), ("invalid", c_u64), ("ntime", c_u64),
                ("duplicates", c_u64), ("recorded", c_u64), ("count", c_u64),
                ("credited", c_u64), ("unattributed", c_u64), ("work", c_u64)]


class SessionInit(ctypes.Structure):
    """bm_session_init_t: what bm_sessions_set takes per slot; difficulty_fx in
    units of 2^-32, 0 closes the slot."""
    _fields_ = [("extranonce1", ctypes.c_uint8 * 8), ("difficulty_fx", c_u64), ("account", c_u32), ("reserved", c_u32)]


class SessionState(ctypes.Structure):
    """bm_session_state_t: a slot's difficulty, the start of its window, the
    accepted submissions since then and its changes since it was set."""
    _fields_ = [("difficulty_fx", c_u64), ("since_ms", c_u64), ("accepted", c_u64), ("retargets", c_u64)]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


class VardiffPolicyStruct(ctypes.Structure):
    """bm_vardiff_policy_t."""
    _fields_ = [("target_ms", c_u64), ("window_ms", c_u64), ("min_difficulty_fx", c_u64), ("max_difficulty_fx", c_u64),
                ("burst", c_u32), ("band_permille", c_u32), ("max_up", c_u32), ("max_down", c_u32)]


class VardiffChange(ctypes.Structure):
    """bm_vardiff_change_t: one changed slot of a retarget; target is T(new_fx)."""
    _fields_ = [("session", c_u32), ("reserved", c_u32), ("old_fx", c_u64), ("new_fx", c_u64),
                ("target", ctypes.c_uint8 * 32)]

    def as_tuple(self):
        return (self.session, self.old_fx, self.new_fx, int.from_bytes(bytes(self.target), "big"))


class VardiffResult(ctypes.Structure):
    """bm_vardiff_result_t: the open, evaluated and changed slots of a retarget,
    and the changed ones that went up and down."""
    _fields_ = [("open", c_u64), ("evaluated", c_u64), ("changed", c_u64), ("raised", c_u64), ("lowered", c_u64)]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


class Segment(ctypes.Structure):
    _fields_ = [("p", c_i32), ("nbv", c_i32), ("pad_block", c_i32), ("digits", c_i32), ("nd", c_i32),
                ("max_inner", c_i32), ("vlo", c_u64), ("vhi", c_u64), ("nonce_base", c_u64),
                ("mid", c_u32 * 8), ("tmpl", c_u32 * 32), ("pad_w", c_u32 * 16)]


class BtcMinerError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__(f"{what}: {strerror(status)} ({status})")


_lib = None
_variants = {}
# The same library built with BM_CLOCK_PROBE=1 (`make -C csrc probe`): its
# launches stamp the shader clock.  bench.py loads it beside the product
# library, only to measure the clock under the dominant kernel after the
# timed region; nothing else uses it.
PROBE_LIB_PATH = os.path.join(_HERE, "libbtcminer_probe.so")


def load(path=None):
    """Load libbtcminer.so once (or, with a path, another build of the same
    ABI, e.g. PROBE_LIB_PATH); raises OSError if it has not been built."""
    global _lib
    if path is not None and os.path.abspath(path) != os.path.abspath(LIB_PATH):
        path = os.path.abspath(path)
        if path not in _variants:
            _variants[path] = _open(path)
        return _variants[path]
    if _lib is not None:
        return _lib
    _lib = _open(LIB_PATH)
    return _lib


def _open(path):
    if not os.path.exists(path):
        raise OSError(f"{path} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')} -j8` "
                      "(or __graft_entry__.build())")
    # RTLD_NOW: every HIP/RCCL symbol of the library (and of the runtime it
    # pulls in) binds at load time.  A process that imports torch afterwards
    # maps torch's bundled HIP runtime too; lazy binding could then resolve
    # some of our calls into that second runtime.
    lib = ctypes.CDLL(path, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    P = ctypes.POINTER
    vp = ctypes.c_void_p
    sigs = {
        "bm_abi_version": ([], ctypes.c_int),
        "bm_strerror": ([ctypes.c_int], ctypes.c_char_p),
        "bm_device_count": ([P(ctypes.c_int)], ctypes.c_int),
        "bm_device_pci_bus_id": ([ctypes.c_int, ctypes.c_char_p, ctypes.c_int], ctypes.c_int),
        "bm_ctx_create": ([ctypes.c_int, P(vp)], ctypes.c_int),
        "bm_ctx_create_devices": ([P(ctypes.c_int), ctypes.c_int, P(vp)], ctypes.c_int),
        "bm_ctx_destroy": ([vp], ctypes.c_int),
        "bm_ctx_num_devices": ([vp, P(ctypes.c_int)], ctypes.c_int),
        "bm_rccl_unique_id": ([ctypes.c_char_p], ctypes.c_int),
        "bm_ctx_create_rank": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, P(vp)], ctypes.c_int),
        "bm_ctx_create_rank_local": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, P(vp)], ctypes.c_int),
        "bm_ctx_join_rank": ([vp, ctypes.c_char_p, ctypes.c_int], ctypes.c_int),
        "bm_ctx_leave_rank": ([vp], ctypes.c_int),
        "bm_ctx_rank_joined": ([vp, P(ctypes.c_int)], ctypes.c_int),
        "bm_ctx_set_peer_timeout": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_ctx_set_test_rccl_fault": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_ctx_set_test_start_delay": ([vp, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "bm_ctx_rank": ([vp, P(ctypes.c_int), P(ctypes.c_int)], ctypes.c_int),
        "bm_reduce_gpu": ([vp, P(Result), ctypes.c_size_t, P(Result)], ctypes.c_int),
        "bm_ctx_set_test_fault": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_search_gpu": ([vp, ctypes.c_char_p, ctypes.c_size_t, c_u64, c_u64, P(Result)], ctypes.c_int),
        "bm_search_target_gpu": ([vp, ctypes.c_char_p, ctypes.c_size_t, c_u64, c_u64, c_u64, P(TargetResult)],
                                 ctypes.c_int),
        "bm_ctx_last_target_stats": ([vp, P(TargetStats)], ctypes.c_int),
        "bm_search_hits_gpu": ([vp, ctypes.c_char_p, ctypes.c_size_t, c_u64, c_u64, c_u64, P(Result),
                                ctypes.c_size_t, P(HitsResult)], ctypes.c_int),
        "bm_search_header_gpu": ([vp, ctypes.c_char_p, c_u32, c_u32, ctypes.c_char_p, P(HeaderResult)], ctypes.c_int),
        "bm_search_header_hits_gpu": ([vp, ctypes.c_char_p, c_u32, c_u32, ctypes.c_char_p, P(HeaderHit),
                                       ctypes.c_size_t, P(HeaderHitsResult)], ctypes.c_int),
        "bm_search_header_versions_gpu": ([vp, ctypes.c_char_p, P(c_u32), ctypes.c_size_t, c_u32, c_u32,
                                           ctypes.c_char_p, P(HeaderVersionsResult)], ctypes.c_int),
        "bm_search_header_versions_hits_gpu": ([vp, ctypes.c_char_p, P(c_u32), ctypes.c_size_t, c_u32, c_u32,
                                                ctypes.c_char_p, P(HeaderVersionHit), ctypes.c_size_t,
                                                P(HeaderVersionsHitsResult)], ctypes.c_int),
        "bm_header_hash_gpu": ([vp, ctypes.c_char_p, P(c_u32), ctypes.c_size_t, P(ctypes.c_uint8)], ctypes.c_int),
        "bm_header_target_from_bits": ([c_u32, P(ctypes.c_uint8)], ctypes.c_int),
        "bm_job_prevhash_from_stratum": ([ctypes.c_char_p, P(ctypes.c_uint8)], ctypes.c_int),
        "bm_job_header": ([P(JobStruct), c_u64, c_u32, c_u32, P(ctypes.c_uint8)], ctypes.c_int),
        "bm_target_from_difficulty": ([ctypes.c_double, P(ctypes.c_uint8)], ctypes.c_int),
        "bm_search_job_shares_gpu": ([vp, P(JobStruct), c_u32, c_u64, c_u64, P(c_u32), ctypes.c_size_t, c_u32, c_u32,
                                      ctypes.c_char_p, P(JobShare), ctypes.c_size_t, P(JobSharesResult)],
                                     ctypes.c_int),
        "bm_job_verify_cpu": ([P(JobStruct), ctypes.c_char_p, P(JobSubmit), ctypes.c_size_t, P(JobVerdict),
                               P(JobVerifyResult)], ctypes.c_int),
        "bm_job_verify_gpu": ([vp, P(JobStruct), ctypes.c_char_p, P(JobSubmit), ctypes.c_size_t, P(JobVerdict),
                               P(JobVerifyResult)], ctypes.c_int),
        "bm_pool_verify_cpu": ([P(JobStruct), P(PoolSessionStruct), ctypes.c_size_t, P(PoolSubmit), ctypes.c_size_t,
                                c_u32, c_u32, P(JobVerdict), P(PoolVerifyResult)], ctypes.c_int),
        "bm_pool_verify_gpu": ([vp, P(JobStruct), P(PoolSessionStruct), ctypes.c_size_t, P(PoolSubmit),
                                ctypes.c_size_t, c_u32, c_u32, P(JobVerdict), P(PoolVerifyResult)], ctypes.c_int),
        "bm_jobs_verify_cpu": ([P(PoolJobStruct), ctypes.c_size_t, P(PoolSessionStruct), ctypes.c_size_t, P(JobsSubmit),
                                ctypes.c_size_t, P(JobVerdict), P(PoolVerifyResult)], ctypes.c_int),
        "bm_jobs_verify_gpu": ([vp, P(PoolJobStruct), ctypes.c_size_t, P(PoolSessionStruct), ctypes.c_size_t,
                                P(JobsSubmit), ctypes.c_size_t, P(JobVerdict), P(PoolVerifyResult)], ctypes.c_int),
        "bm_share_set_verify_jobs": ([vp, P(PoolJobStruct), ctypes.c_size_t, P(PoolSessionStruct), ctypes.c_size_t,
                                      P(JobsSubmit), ctypes.c_size_t, P(JobVerdict), P(ShareSetResult)], ctypes.c_int),
        "bm_share_set_create": ([vp, ctypes.c_size_t, P(vp)], ctypes.c_int),
        "bm_share_set_create_cpu": ([ctypes.c_size_t, P(vp)], ctypes.c_int),
        "bm_share_set_destroy": ([vp], None),
        "bm_share_set_clear": ([vp], ctypes.c_int),
        "bm_share_set_count": ([vp, P(c_u64), P(c_u64)], ctypes.c_int),
        "bm_share_set_verify": ([vp, P(JobStruct), P(PoolSessionStruct), ctypes.c_size_t, P(PoolSubmit), ctypes.c_size_t,
                                 c_u32, c_u32, P(JobVerdict), P(ShareSetResult)], ctypes.c_int),
        "bm_ledger_create": ([vp, ctypes.c_size_t, P(vp)], ctypes.c_int),
        "bm_ledger_create_cpu": ([ctypes.c_size_t, P(vp)], ctypes.c_int),
        "bm_ledger_destroy": ([vp], None),
        "bm_ledger_clear": ([vp], ctypes.c_int),
        "bm_ledger_rows": ([vp, P(c_u64)], ctypes.c_int),
        "bm_ledger_read": ([vp, ctypes.c_size_t, ctypes.c_size_t, P(LedgerRow)], ctypes.c_int),
        "bm_ledger_drain": ([vp, ctypes.c_size_t, ctypes.c_size_t, P(LedgerRow)], ctypes.c_int),
        "bm_ledger_set_peel": ([vp, c_u32], ctypes.c_int),
        "bm_ledger_verify_jobs": ([vp, vp, P(PoolJobStruct), ctypes.c_size_t, P(PoolSessionStruct), ctypes.c_size_t,
                                   P(c_u32), P(c_u64), P(JobsSubmit), ctypes.c_size_t, P(JobVerdict),
                                   P(LedgerResult)], ctypes.c_int),
        "bm_target_from_difficulty_fx": ([c_u64, P(ctypes.c_uint8)], ctypes.c_int),
        "bm_sessions_create": ([vp, ctypes.c_size_t, P(vp)], ctypes.c_int),
        "bm_sessions_create_cpu": ([ctypes.c_size_t, P(vp)], ctypes.c_int),
        "bm_sessions_destroy": ([vp], None),
        "bm_sessions_clear": ([vp], ctypes.c_int),
        "bm_sessions_count": ([vp, P(c_u64), P(c_u64)], ctypes.c_int),
        "bm_sessions_set": ([vp, P(c_u32), ctypes.c_size_t, P(SessionInit), c_u64], ctypes.c_int),
        "bm_sessions_get": ([vp, ctypes.c_size_t, ctypes.c_size_t, P(PoolSessionStruct), P(c_u32), P(c_u64),
                             P(SessionState)], ctypes.c_int),
        "bm_sessions_verify_jobs": ([vp, vp, vp, P(PoolJobStruct), ctypes.c_size_t, P(JobsSubmit), ctypes.c_size_t,
                                     P(JobVerdict), P(LedgerResult)], ctypes.c_int),
        "bm_sessions_retarget": ([vp, c_u64, P(VardiffPolicyStruct), P(VardiffChange), ctypes.c_size_t,
                                  P(VardiffResult)], ctypes.c_int),
        "bm_hash_gpu": ([vp, ctypes.c_char_p, ctypes.c_size_t, P(c_u64), ctypes.c_size_t, P(c_u64)],
                        ctypes.c_int),
        "bm_ctx_set_timing": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_ctx_last_stats": ([vp, P(Stats)], ctypes.c_int),
        "bm_ctx_set_blocks_per_cu": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_ctx_set_max_windows": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_ctx_set_combine": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_ctx_set_task_digits": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_ctx_set_split": ([vp, P(ctypes.c_uint32), ctypes.c_int], ctypes.c_int),
        "bm_ctx_get_split": ([vp, P(ctypes.c_uint32), ctypes.c_int, P(ctypes.c_int)], ctypes.c_int),
        "bm_ctx_set_balance": ([vp, ctypes.c_int], ctypes.c_int),
        "bm_split_range": ([c_u64, c_u64, P(ctypes.c_uint32), ctypes.c_int, P(c_u64), P(c_u64)], ctypes.c_int),
        "bm_plan_segments": ([ctypes.c_char_p, ctypes.c_size_t, c_u64, c_u64, P(Segment), ctypes.c_int,
                              P(ctypes.c_int)], ctypes.c_int),
        "bm_plan_segments_ex": ([ctypes.c_char_p, ctypes.c_size_t, c_u64, c_u64, ctypes.c_int, P(Segment),
                                 ctypes.c_int, P(ctypes.c_int)], ctypes.c_int),
    }
    for name, (args, res) in sigs.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:  # a build from before the call was added (the ABI version did not change)
            raise OSError(f"{path}: no {name}; rebuild it") from None
        fn.argtypes = args
        fn.restype = res
    # the stats structs above are this ABI's layout: any other build (an
    # older BTCMINER_LIB variant included) would be misread, so it is refused
    if lib.bm_abi_version() != BM_ABI_VERSION:
        raise OSError(f"{path}: ABI version {lib.bm_abi_version()}, expected {BM_ABI_VERSION}; rebuild it")
    return lib


def strerror(status):
    try:
        return load().bm_strerror(status).decode()
    except OSError:
        return f"status {status}"


def check(status, what):
    if status != BM_OK:
        raise BtcMinerError(status, what)


def device_count():
    n = ctypes.c_int(0)
    check(load().bm_device_count(ctypes.byref(n)), "bm_device_count")
    return n.value


def device_pci_bus_id(device: int) -> str:
    """PCI bus id of a visible device, e.g. "0000:05:00.0"."""
    buf = ctypes.create_string_buffer(64)
    check(load().bm_device_pci_bus_id(device, buf, len(buf)), "bm_device_pci_bus_id")
    return buf.value.decode()


DEFAULT_MAX_WINDOWS = 64


def plan_segments(msg: bytes, lower: int, upper: int, max_windows: int = DEFAULT_MAX_WINDOWS):
    """Host-side launch plan (pure CPU): list of Segment structs."""
    lib = load()
    n = ctypes.c_int(0)
    f = lib.bm_plan_segments_ex
    check(f(msg, len(msg), lower, upper, max_windows, None, 0, ctypes.byref(n)), "bm_plan_segments")
    arr = (Segment * max(n.value, 1))()
    check(f(msg, len(msg), lower, upper, max_windows, arr, n.value, ctypes.byref(n)), "bm_plan_segments")
    return list(arr[: n.value])


def split_range(lower: int, upper: int, n: int, shares=None):
    """The library's partitioner (bm_split_range, pure CPU): n inclusive
    pieces of [lower, upper], None for an empty one; shares None: near-equal."""
    lo, hi = (c_u64 * n)(), (c_u64 * n)()
    sh = (ctypes.c_uint32 * n)(*shares) if shares is not None else None
    check(load().bm_split_range(lower, upper, sh, n, lo, hi), "bm_split_range")
    return [(a, b) if a <= b else None for a, b in zip(lo, hi)]


def bits_to_target(nbits: int) -> int:
    """Bitcoin's compact target (a block header's `bits` field) as an integer
    (bm_header_target_from_bits, pure CPU); ValueError for a negative or
    overflowing form."""
    if not 0 <= nbits <= U32_MAX:
        raise ValueError(f"bits must be in 0..2^32-1, got {nbits}")
    buf = (ctypes.c_uint8 * 32)()
    if load().bm_header_target_from_bits(nbits, buf) != BM_OK:
        raise ValueError(f"bits {nbits:#010x} is negative or overflows 256 bits")
    return int.from_bytes(bytes(buf), "big")


def roll_versions(base: int, count: int, mask: int = BIP320_MASK):
    """`count` version fields rolled from `base` inside `mask` (BIP 320's by
    default): the i-th is base with the bits of i deposited into the mask's
    bit positions, lowest first (base's own bits under the mask are replaced).
    ValueError when count exceeds the
    2^popcount(mask) values the mask holds."""
    for v, what in ((base, "base"), (mask, "mask")):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U32_MAX:
            raise ValueError(f"{what} must be in 0..2^32-1, got {v!r}")
    if not isinstance(count, int) or isinstance(count, bool) or count < 0:
        raise ValueError(f"count must be a non-negative integer, got {count!r}")
    positions = [b for b in range(32) if mask >> b & 1]
    if count > 1 << len(positions):
        raise ValueError(f"mask {mask:#010x} holds {1 << len(positions)} versions, {count} asked for")
    out = []
    for i in range(count):
        v = base & ~mask
        for k, b in enumerate(positions):
            v |= (i >> k & 1) << b
        out.append(v)
    return out


def difficulty_to_target(difficulty) -> int:
    """A pool's share difficulty as a target: floor(diff1 / difficulty), diff1 =
    0xffff * 2^208, exact for the float's rational value and saturating at
    2^256-1 (bm_target_from_difficulty, pure CPU); ValueError for a NaN, an
    infinity or a value <= 0."""
    if isinstance(difficulty, bool) or not isinstance(difficulty, (int, float)):
        raise ValueError(f"difficulty must be a number, got {difficulty!r}")
    try:
        d = float(difficulty)
    except OverflowError:
        raise ValueError(f"difficulty {difficulty!r} does not fit a double") from None
    buf = (ctypes.c_uint8 * 32)()
    if load().bm_target_from_difficulty(d, buf) != BM_OK:
        raise ValueError(f"difficulty must be a finite number above 0, got {difficulty!r}")
    return int.from_bytes(bytes(buf), "big")


def difficulty_fx_to_target(difficulty_fx: int) -> int:
    """A difficulty in units of 2^-32 as a target: floor(0xffff * 2^240 /
    difficulty_fx), exact and never saturating (bm_target_from_difficulty_fx, pure
    CPU); ValueError outside 1..2^64-1."""
    if not isinstance(difficulty_fx, int) or isinstance(difficulty_fx, bool) or not 1 <= difficulty_fx <= U64_MAX:
        raise ValueError(f"difficulty_fx must be in 1..2^64-1, got {difficulty_fx!r}")
    buf = (ctypes.c_uint8 * 32)()
    check(load().bm_target_from_difficulty_fx(difficulty_fx, buf), "bm_target_from_difficulty_fx")
    return int.from_bytes(bytes(buf), "big")


def _hex_bytes(text, what, length=None) -> bytes:
    try:
        if not isinstance(text, str):
            raise ValueError
        raw = bytes.fromhex(text)
    except ValueError:
        raise ValueError(f"{what} must be a hex string, got {text!r}") from None
    if length is not None and len(raw) != length:
        raise ValueError(f"{what} must be {length} bytes, got {len(raw)}")
    return raw


def _u32(v, what) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U32_MAX:
        raise ValueError(f"{what} must be in 0..2^32-1, got {v!r}")
    return v


class Job:
    """A Stratum job (bm_job_t) that owns its buffers: the coinbase halves, the
    miner's extranonce1, the size of extranonce2, the merkle branch (a list of
    32-byte entries as sent), prevhash in header byte order, and version, nbits
    and ntime as integers.  job_id is carried for submit_params only."""

    def __init__(self, coinb1: bytes, extranonce1: bytes, extranonce2_size: int, coinb2: bytes, branch=(),
                 prevhash: bytes = bytes(32), version: int = 0, nbits: int = 0, ntime: int = 0, job_id: str = ""):
        self.coinb1, self.extranonce1, self.coinb2 = bytes(coinb1), bytes(extranonce1), bytes(coinb2)
        self.branch = [bytes(b) for b in branch]
        self.prevhash = bytes(prevhash)
        if isinstance(extranonce2_size, bool) or not isinstance(extranonce2_size, int) or not 1 <= extranonce2_size <= 8:
            raise ValueError(f"extranonce2_size must be in 1..8, got {extranonce2_size!r}")
        if len(self.prevhash) != 32 or any(len(b) != 32 for b in self.branch):
            raise ValueError("prevhash and every branch entry are 32 bytes")
        if len(self.branch) > BM_MAX_JOB_BRANCH:
            raise ValueError(f"at most {BM_MAX_JOB_BRANCH} branch entries, got {len(self.branch)}")
        if len(self.coinb1) + len(self.extranonce1) + extranonce2_size + len(self.coinb2) > BM_MAX_JOB_COINBASE:
            raise ValueError(f"the coinbase is longer than {BM_MAX_JOB_COINBASE} bytes")
        self.extranonce2_size = extranonce2_size
        self.version, self.nbits, self.ntime = _u32(version, "version"), _u32(nbits, "nbits"), _u32(ntime, "ntime")
        self.job_id = job_id
        self._branch = b"".join(self.branch)
        self.struct = JobStruct(self.coinb1, len(self.coinb1), self.extranonce1, len(self.extranonce1),
                                extranonce2_size, self.coinb2, len(self.coinb2), self._branch, len(self.branch),
                                (ctypes.c_uint8 * 32)(*self.prevhash), self.version, self.nbits)

    @classmethod
    def from_notify(cls, params, extranonce1_hex: str, extranonce2_size: int):
        """From the nine params of mining.notify (job id, prevhash, coinb1,
        coinb2, merkle branch, version, nbits, ntime, clean_jobs) and what
        mining.subscribe answered.  prevhash comes word-swapped and version,
        nbits and ntime as big-endian hex, as Stratum sends them."""
        params = list(params)
        if len(params) != 9:
            raise ValueError(f"mining.notify has 9 params, got {len(params)}")
        job_id, prevhash, coinb1, coinb2, branch, version, nbits, ntime, _clean = params
        if not isinstance(branch, (list, tuple)):
            raise ValueError("the merkle branch must be a list of hex strings")
        swapped = (ctypes.c_uint8 * 32)()
        check(load().bm_job_prevhash_from_stratum(_hex_bytes(prevhash, "prevhash", 32), swapped),
              "bm_job_prevhash_from_stratum")
        words = [int.from_bytes(_hex_bytes(v, what, 4), "big")
                 for v, what in ((version, "version"), (nbits, "nbits"), (ntime, "ntime"))]
        return cls(_hex_bytes(coinb1, "coinb1"), _hex_bytes(extranonce1_hex, "extranonce1"), extranonce2_size,
                   _hex_bytes(coinb2, "coinb2"), [_hex_bytes(b, "a branch entry", 32) for b in branch],
                   bytes(swapped), words[0], words[1], words[2], job_id=str(job_id))

    def _check_extranonce2(self, v, what="extranonce2"):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 1 << (8 * self.extranonce2_size):
            raise ValueError(f"{what} must be in 0..2^{8 * self.extranonce2_size}-1, got {v!r}")
        return v

    def header(self, extranonce2: int, ntime=None, version=None, nonce: int = 0) -> bytes:
        """The 80-byte header of this job under extranonce2 (bm_job_header, pure
        CPU); ntime and version default to the job's own."""
        self._check_extranonce2(extranonce2)
        ntime = _u32(self.ntime if ntime is None else ntime, "ntime")
        version = _u32(self.version if version is None else version, "version")
        buf = (ctypes.c_uint8 * HEADER_BYTES)()
        check(load().bm_job_header(ctypes.byref(self.struct), extranonce2, ntime, version, buf), "bm_job_header")
        return bytes(buf)[:76] + _u32(nonce, "nonce").to_bytes(4, "little")


def submit_params(worker: str, job_id: str, share, mask: int = BIP320_MASK):
    """mining.submit's params for a share of Context.search_job_shares (a dict
    with extranonce2, extranonce2_size, ntime, nonce and version): [worker, job
    id, extranonce2, ntime, nonce, version bits], all hex; the last is BIP 310's
    version_bits, the share's version under the negotiated mask."""
    _u32(mask, "mask")
    size = share["extranonce2_size"]
    return [worker, job_id, "%0*x" % (2 * size, share["extranonce2"]), "%08x" % share["ntime"],
            "%08x" % share["nonce"], "%08x" % (share["version"] & mask)]


def _hex_field(text, digits, what) -> int:
    if not isinstance(text, str) or len(text) != digits or any(c not in "0123456789abcdefABCDEF" for c in text):
        raise ValueError(f"{what} must be {digits} hex digits, got {text!r}")
    return int(text, 16)


def parse_submit(params, job, mask: int = BIP320_MASK):
    """The inverse of submit_params: mining.submit's params as sent ([worker, job
    id, extranonce2, ntime, nonce] and, with version rolling, version bits) ->
    a dict with extranonce2, extranonce2_size, ntime, nonce and version, the full
    header version (job.version & ~mask) | bits; five params give job.version.
    ValueError, with the reason first, for a wrong param count ("malformed"),
    another job's id ("job-id"), an extranonce2 that is not 2 * extranonce2_size
    hex digits ("extranonce2"), a field that is not 8 hex digits ("malformed") or
    version bits outside the mask ("version-bits")."""
    _u32(mask, "mask")
    if not isinstance(params, (list, tuple)) or len(params) not in (5, 6):
        raise ValueError("malformed: mining.submit has 5 or 6 params")
    if params[1] != job.job_id:
        raise ValueError(f"job-id: the job is {job.job_id!r}, got {params[1]!r}")
    try:
        en2 = _hex_field(params[2], 2 * job.extranonce2_size, "extranonce2")
    except ValueError as e:
        raise ValueError(f"extranonce2: {e}") from None
    try:
        ntime, nonce = _hex_field(params[3], 8, "ntime"), _hex_field(params[4], 8, "nonce")
        bits = _hex_field(params[5], 8, "version bits") if len(params) == 6 else None
    except ValueError as e:
        raise ValueError(f"malformed: {e}") from None
    version = job.version
    if bits is not None:
        if bits & ~mask:
            raise ValueError(f"version-bits: {bits:08x} has bits outside the mask {mask:08x}")
        version = (job.version & ~mask & U32_MAX) | bits
    return {"extranonce2": en2, "extranonce2_size": job.extranonce2_size, "ntime": ntime, "nonce": nonce,
            "version": version}


def _submit_array(submits):
    """A (JobSubmit * n) array from one (used as it is) or from an iterable of
    dicts (extranonce2, ntime, nonce, version: parse_submit's, or the shares of
    Context.search_job_shares) or (extranonce2, ntime, nonce, version) tuples."""
    if isinstance(submits, ctypes.Array) and submits._type_ is JobSubmit:
        return submits
    rows = []
    for s in submits:
        row = tuple(s[k] for k in ("extranonce2", "ntime", "nonce", "version")) if isinstance(s, dict) else tuple(s)
        if len(row) != 4:
            raise ValueError(f"a submission is (extranonce2, ntime, nonce, version), got {s!r}")
        if not isinstance(row[0], int) or isinstance(row[0], bool) or not 0 <= row[0] <= U64_MAX:
            raise ValueError(f"extranonce2 must be in 0..2^64-1, got {row[0]!r}")
        for v, what in zip(row[1:], ("ntime", "nonce", "version")):
            _u32(v, what)
        rows.append(row)
    arr = (JobSubmit * len(rows))()
    for a, row in zip(arr, rows):
        a.extranonce2, a.ntime, a.nonce, a.version = row
    return arr


def _verify(call, what, job, submits, target):
    if not isinstance(job, Job):
        raise ValueError("job must be a Job")
    arr = _submit_array(submits)
    if len(arr) > BM_MAX_JOB_SUBMITS:
        raise ValueError(f"at most {BM_MAX_JOB_SUBMITS} submissions per call, got {len(arr)}")
    tgt = _target_bytes(target)
    verdicts = (JobVerdict * len(arr))()
    r = JobVerifyResult()
    check(call(ctypes.byref(job.struct), tgt, arr if len(arr) else None, len(arr), verdicts if len(arr) else None,
               ctypes.byref(r)), what)
    return verdicts, r


def verify_submits_cpu(job, submits, target):
    """Context.verify_submits without a GPU or a context (bm_job_verify_cpu, pure
    CPU): the specification of the GPU entry, byte-identical to it."""
    return _verify(load().bm_job_verify_cpu, "bm_job_verify_cpu", job, submits, target)


def parse_pool_submit(params, job, sessions_by_worker, mask: int = BIP320_MASK):
    """parse_submit for a pool: params[0], the worker's name, is resolved to its
    session index through sessions_by_worker (a mapping name -> index), which
    the result carries as "session" beside parse_submit's fields.  Raises
    parse_submit's reasons, and ValueError("worker: ...") for a name the mapping
    does not hold."""
    sub = parse_submit(params, job, mask)
    worker = params[0]
    if not isinstance(worker, str) or worker not in sessions_by_worker:
        raise ValueError(f"worker: no session for {worker!r}")
    return dict(sub, session=sessions_by_worker[worker])


def _session_array(sessions, size):
    """A (PoolSessionStruct * n) array from one (used as it is) or from an
    iterable of PoolSession or (extranonce1, target) pairs, each extranonce1 of
    size bytes."""
    if isinstance(sessions, ctypes.Array) and sessions._type_ is PoolSessionStruct:
        return sessions
    rows = [s if isinstance(s, PoolSession) else PoolSession(*s) for s in sessions]
    arr = (PoolSessionStruct * len(rows))()
    for a, s in zip(arr, rows):
        if len(s.extranonce1) != size:
            raise ValueError(f"every session's extranonce1 is {size} bytes (the job's), got {s.extranonce1!r}")
        ctypes.memmove(a.extranonce1, s.extranonce1, size)
        ctypes.memmove(a.target, s.target.to_bytes(32, "big"), 32)
    return arr


def _pool_submit_array(submits):
    """A (PoolSubmit * n) array from one (used as it is) or from an iterable of
    dicts (extranonce2, ntime, nonce, version, session: parse_pool_submit's) or
    (extranonce2, ntime, nonce, version, session) tuples."""
    if isinstance(submits, ctypes.Array) and submits._type_ is PoolSubmit:
        return submits
    keys = ("extranonce2", "ntime", "nonce", "version", "session")
    rows = []
    for s in submits:
        row = tuple(s[k] for k in keys) if isinstance(s, dict) else tuple(s)
        if len(row) != 5:
            raise ValueError(f"a pool submission is (extranonce2, ntime, nonce, version, session), got {s!r}")
        if not isinstance(row[0], int) or isinstance(row[0], bool) or not 0 <= row[0] <= U64_MAX:
            raise ValueError(f"extranonce2 must be in 0..2^64-1, got {row[0]!r}")
        for v, what in zip(row[1:], keys[1:]):
            _u32(v, what)
        rows.append(row)
    arr = (PoolSubmit * len(rows))()
    for a, row in zip(arr, rows):
        a.extranonce2, a.ntime, a.nonce, a.version, a.session = row
    return arr


def _pool_verify(call, what, job, sessions, submits, ntime_lo, ntime_hi, result=None):
    if not isinstance(job, Job):
        raise ValueError("job must be a Job")
    if not 1 <= len(job.extranonce1) <= 8:
        raise ValueError(f"the job's extranonce1 gives the size of every session's: 1..8 bytes, got {len(job.extranonce1)}")
    ses = _session_array(sessions, len(job.extranonce1))
    arr = _pool_submit_array(submits)
    if len(arr) > BM_MAX_JOB_SUBMITS:
        raise ValueError(f"at most {BM_MAX_JOB_SUBMITS} submissions per call, got {len(arr)}")
    if len(ses) > BM_MAX_POOL_SESSIONS:
        raise ValueError(f"at most {BM_MAX_POOL_SESSIONS} sessions per call, got {len(ses)}")
    _u32(ntime_lo, "ntime_lo"), _u32(ntime_hi, "ntime_hi")
    verdicts = (JobVerdict * len(arr))()
    r = (result or PoolVerifyResult)()
    check(call(ctypes.byref(job.struct), ses if len(ses) else None, len(ses), arr if len(arr) else None, len(arr),
               ntime_lo, ntime_hi, verdicts if len(arr) else None, ctypes.byref(r)), what)
    return verdicts, r


def verify_pool_submits_cpu(job, sessions, submits, ntime_lo: int = 0, ntime_hi: int = (1 << 32) - 1):
    """Context.verify_pool_submits without a GPU or a context (bm_pool_verify_cpu,
    pure CPU): the specification of the GPU entry, byte-identical to it."""
    return _pool_verify(load().bm_pool_verify_cpu, "bm_pool_verify_cpu", job, sessions, submits, ntime_lo, ntime_hi)


class PoolJob:
    """One live job of a pool (bm_pool_job_t): a Job, read as the pool calls read
    it (its extranonce1 gives the size only), and its own ntime window, inclusive."""
    __slots__ = ("job", "ntime_lo", "ntime_hi")

    def __init__(self, job, ntime_lo: int = 0, ntime_hi: int = U32_MAX):
        if not isinstance(job, Job):
            raise ValueError("job must be a Job")
        if not 1 <= len(job.extranonce1) <= 8:
            raise ValueError(f"a pool job's extranonce1 gives the size of every session's: 1..8 bytes, got {len(job.extranonce1)}")
        self.job, self.ntime_lo, self.ntime_hi = job, _u32(ntime_lo, "ntime_lo"), _u32(ntime_hi, "ntime_hi")

    def __repr__(self):
        return f"PoolJob({self.job.job_id!r}, {self.ntime_lo}, {self.ntime_hi})"


def parse_jobs_submit(params, jobs_by_id, index, mask: int = BIP320_MASK):
    """parse_pool_submit over several live jobs: params[1], the job id, picks the
    job through jobs_by_id, a mapping id -> (index into the call's jobs, Job); the
    result carries that index as "job" beside parse_pool_submit's fields.  Raises
    parse_pool_submit's reasons -- but for "job-id" -- and ValueError("job: ...")
    for an id the mapping does not hold."""
    if not isinstance(params, (list, tuple)) or len(params) not in (5, 6):
        raise ValueError("malformed: mining.submit has 5 or 6 params")
    job_id = params[1]
    if not isinstance(job_id, str) or job_id not in jobs_by_id:
        raise ValueError(f"job: no live job {job_id!r}")
    j, job = jobs_by_id[job_id]
    return dict(parse_pool_submit(params, job, index, mask), job=j)


def _jobs_array(jobs):
    """(a (PoolJobStruct * n) array, the PoolJob rows that keep its buffers alive)
    from an iterable of PoolJob, Job (no window) or (job, ntime_lo, ntime_hi)."""
    rows = [j if isinstance(j, PoolJob) else PoolJob(j) if isinstance(j, Job) else PoolJob(*j) for j in jobs]
    if len(rows) > BM_MAX_POOL_JOBS:
        raise ValueError(f"at most {BM_MAX_POOL_JOBS} jobs per call, got {len(rows)}")
    arr = (PoolJobStruct * len(rows))()
    for a, r in zip(arr, rows):
        ctypes.memmove(ctypes.byref(a.job), ctypes.byref(r.job.struct), ctypes.sizeof(JobStruct))
        a.ntime_lo, a.ntime_hi = r.ntime_lo, r.ntime_hi
    return arr, rows


def _jobs_session_array(sessions, size):
    """A (PoolSessionStruct * n) array from one (used as it is) or from an iterable
    of PoolSession or (extranonce1, target) pairs, each extranonce1 at least size
    bytes (the longest any of the call's jobs reads: a job reads its first
    extranonce1_len bytes)."""
    if isinstance(sessions, ctypes.Array) and sessions._type_ is PoolSessionStruct:
        return sessions
    rows = [s if isinstance(s, PoolSession) else PoolSession(*s) for s in sessions]
    arr = (PoolSessionStruct * len(rows))()
    for a, s in zip(arr, rows):
        if len(s.extranonce1) < size:
            raise ValueError(f"every session's extranonce1 is at least {size} bytes (the jobs' longest), got {s.extranonce1!r}")
        ctypes.memmove(a.extranonce1, s.extranonce1, len(s.extranonce1))
        ctypes.memmove(a.target, s.target.to_bytes(32, "big"), 32)
    return arr


def _jobs_submit_array(submits):
    """A (JobsSubmit * n) array from one (used as it is) or from an iterable of
    dicts (extranonce2, ntime, nonce, version, session, job: parse_jobs_submit's)
    or (extranonce2, ntime, nonce, version, session, job) tuples."""
    if isinstance(submits, ctypes.Array) and submits._type_ is JobsSubmit:
        return submits
    keys = ("extranonce2", "ntime", "nonce", "version", "session", "job")
    rows = []
    for s in submits:
        row = tuple(s[k] for k in keys) if isinstance(s, dict) else tuple(s)
        if len(row) != 6:
            raise ValueError(f"a submission over several jobs is (extranonce2, ntime, nonce, version, session, job), got {s!r}")
        if not isinstance(row[0], int) or isinstance(row[0], bool) or not 0 <= row[0] <= U64_MAX:
            raise ValueError(f"extranonce2 must be in 0..2^64-1, got {row[0]!r}")
        for v, what in zip(row[1:], keys[1:]):
            _u32(v, what)
        rows.append(row)
    arr = (JobsSubmit * len(rows))()
    for a, row in zip(arr, rows):
        a.extranonce2, a.ntime, a.nonce, a.version, a.session, a.job = row
    return arr


def _jobs_verify(call, what, jobs, sessions, submits, result=None):
    jarr, rows = _jobs_array(jobs)
    ses = _jobs_session_array(sessions, max((len(r.job.extranonce1) for r in rows), default=0))
    arr = _jobs_submit_array(submits)
    if len(arr) > BM_MAX_JOB_SUBMITS:
        raise ValueError(f"at most {BM_MAX_JOB_SUBMITS} submissions per call, got {len(arr)}")
    if len(ses) > BM_MAX_POOL_SESSIONS:
        raise ValueError(f"at most {BM_MAX_POOL_SESSIONS} sessions per call, got {len(ses)}")
    verdicts = (JobVerdict * len(arr))()
    r = (result or PoolVerifyResult)()
    check(call(jarr if len(jarr) else None, len(jarr), ses if len(ses) else None, len(ses), arr if len(arr) else None,
               len(arr), verdicts if len(arr) else None, ctypes.byref(r)), what)
    return verdicts, r


def verify_jobs_submits_cpu(jobs, sessions, submits):
    """Context.verify_jobs_submits without a GPU or a context (bm_jobs_verify_cpu,
    pure CPU): the specification of the GPU entry, byte-identical to it."""
    return _jobs_verify(load().bm_jobs_verify_cpu, "bm_jobs_verify_cpu", jobs, sessions, submits)


class ShareSet:
    """A bm_share_set_t: the set of header hashes behind duplicate-share detection,
    cleared by the caller when its jobs retire (the key is the header hash, which
    separates jobs: one set may hold several jobs' shares).  ShareSet(ctx, capacity) lives on the first device of
    ctx, across calls, and is closed before ctx; ShareSet.cpu(capacity) lives in
    host memory and needs no GPU: the specification.  Not thread-safe, and a device
    set shares its context's buffers: one call at a time per context."""

    def __init__(self, ctx, capacity: int, lib_path=None):
        self._h = None
        if not isinstance(capacity, int) or isinstance(capacity, bool) or not 1 <= capacity <= BM_MAX_SHARE_SET:
            raise ValueError(f"capacity must be in 1..{BM_MAX_SHARE_SET}, got {capacity!r}")
        h = ctypes.c_void_p()
        if ctx is None:
            self._lib = load(lib_path)
            check(self._lib.bm_share_set_create_cpu(capacity, ctypes.byref(h)), "bm_share_set_create_cpu")
        else:
            self._lib = ctx._lib
            check(self._lib.bm_share_set_create(ctx.handle, capacity, ctypes.byref(h)), "bm_share_set_create")
        self._ctx = ctx  # a device set must not outlive its context
        self._h = h

    @classmethod
    def cpu(cls, capacity: int, lib_path=None):
        """A set in host memory (bm_share_set_create_cpu)."""
        return cls(None, capacity, lib_path)

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("share set closed")
        return self._h

    def close(self):
        if self._h is not None:
            if self._ctx is None or self._ctx._h is not None:  # (a closed context took the device's memory with it)
                self._lib.bm_share_set_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sizes(self):
        count, capacity = c_u64(0), c_u64(0)
        check(self._lib.bm_share_set_count(self.handle, ctypes.byref(count), ctypes.byref(capacity)), "bm_share_set_count")
        return count.value, capacity.value

    @property
    def count(self) -> int:
        """Hashes the set holds."""
        return self._sizes()[0]

    @property
    def capacity(self) -> int:
        return self._sizes()[1]

    def clear(self):
        """Forget every hash: the set's jobs have retired (a new block height)."""
        check(self._lib.bm_share_set_clear(self.handle), "bm_share_set_clear")

    def verify(self, job, sessions, submits, ntime_lo: int = 0, ntime_hi: int = (1 << 32) - 1):
        """Context.verify_pool_submits plus the set (bm_share_set_verify) ->
        (verdicts, ShareSetResult): an eligible submission (SHARE or BLOCK, not
        INVALID) whose hash the set holds, from an earlier call or a lower index of
        this one, carries BM_SUBMIT_DUPLICATE; the others are recorded.  All or
        nothing: BtcMinerError with status BM_EFULL when the batch's new hashes do
        not fit, and the set is as before."""
        return _pool_verify(lambda *a: self._lib.bm_share_set_verify(self.handle, *a), "bm_share_set_verify", job,
                            sessions, submits, ntime_lo, ntime_hi, ShareSetResult)

    def verify_jobs(self, jobs, sessions, submits):
        """Context.verify_jobs_submits plus the set (bm_share_set_verify_jobs) ->
        (verdicts, ShareSetResult), as verify: the key is the header hash, so the
        set may be fed by verify and verify_jobs alternately, and the same tuple
        under two jobs[] entries of identical content is a duplicate."""
        return _jobs_verify(lambda *a: self._lib.bm_share_set_verify_jobs(self.handle, *a), "bm_share_set_verify_jobs",
                            jobs, sessions, submits, ShareSetResult)


class Ledger:
    """A bm_ledger_t: the per-account tallies behind share accounting -- `rows`
    LedgerRow counters fed by verify_jobs and read or drained at payout or
    retarget time.  Ledger(ctx, rows) lives on the first device of ctx, across
    calls, and is closed before ctx; Ledger.cpu(rows) lives in host memory and
    needs no GPU: the specification.  Not thread-safe, and a device ledger shares
    its context's buffers: one call at a time per context."""

    def __init__(self, ctx, rows: int, lib_path=None):
        self._h = None
        if not isinstance(rows, int) or isinstance(rows, bool) or not 1 <= rows <= BM_MAX_LEDGER_ROWS:
            raise ValueError(f"rows must be in 1..{BM_MAX_LEDGER_ROWS}, got {rows!r}")
        h = ctypes.c_void_p()
        if ctx is None:
            self._lib = load(lib_path)
            check(self._lib.bm_ledger_create_cpu(rows, ctypes.byref(h)), "bm_ledger_create_cpu")
        else:
            self._lib = ctx._lib
            check(self._lib.bm_ledger_create(ctx.handle, rows, ctypes.byref(h)), "bm_ledger_create")
        self._ctx = ctx  # a device ledger must not outlive its context
        self._h = h

    @classmethod
    def cpu(cls, rows: int, lib_path=None):
        """A ledger in host memory (bm_ledger_create_cpu)."""
        return cls(None, rows, lib_path)

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("ledger closed")
        return self._h

    def close(self):
        if self._h is not None:
            if self._ctx is None or self._ctx._h is not None:  # (a closed context took the device's memory with it)
                self._lib.bm_ledger_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self) -> int:
        rows = c_u64(0)
        check(self._lib.bm_ledger_rows(self.handle, ctypes.byref(rows)), "bm_ledger_rows")
        return rows.value

    def clear(self):
        """Empty every row."""
        check(self._lib.bm_ledger_clear(self.handle), "bm_ledger_clear")

    def set_peel(self, rounds: int):
        """The device kernel's combine rounds, 0..64 (a CPU ledger ignores them)."""
        check(self._lib.bm_ledger_set_peel(self.handle, _u32(rounds, "rounds")), "bm_ledger_set_peel")

    def _range(self, call, what, first, count):
        if count is None:
            count = max(self.rows - first, 0)
        for v, name in ((first, "first"), (count, "count")):
            if not isinstance(v, int) or isinstance(v, bool) or v < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
        out = (LedgerRow * count)()
        check(call(self.handle, first, count, out if count else None), what)
        return out

    def read(self, first: int = 0, count=None):
        """Rows [first, first + count) as a (LedgerRow * count) array; count None:
        to the end."""
        return self._range(self._lib.bm_ledger_read, "bm_ledger_read", first, count)

    def drain(self, first: int = 0, count=None):
        """read, then exactly those rows are empty again."""
        return self._range(self._lib.bm_ledger_drain, "bm_ledger_drain", first, count)

    def verify_jobs(self, jobs, sessions, submits, share_set=None, accounts=None, weights=None):
        """ShareSet.verify_jobs (or, without share_set, Context.verify_jobs_submits)
        plus the credit of every submission to the row of its session's account
        (bm_ledger_verify_jobs) -> (verdicts, LedgerResult).  accounts: one row
        index per session (None: session s -> row s); weights: one u64 per session
        (None: 1 each).  All or nothing, as ShareSet.verify_jobs."""
        if not isinstance(sessions, ctypes.Array):
            sessions = list(sessions)
        nses = len(sessions)
        acc = wgt = None
        if accounts is not None:
            accounts = [_u32(a, "account") for a in accounts]
            if len(accounts) != nses:
                raise ValueError(f"accounts has one entry per session ({nses}), got {len(accounts)}")
            acc = (c_u32 * max(nses, 1))(*accounts)
        if weights is not None:
            weights = list(weights)
            if len(weights) != nses:
                raise ValueError(f"weights has one entry per session ({nses}), got {len(weights)}")
            for w in weights:
                if not isinstance(w, int) or isinstance(w, bool) or not 0 <= w <= U64_MAX:
                    raise ValueError(f"a weight must be in 0..2^64-1, got {w!r}")
            wgt = (c_u64 * max(nses, 1))(*weights)
        sh = share_set.handle if share_set is not None else None
        return _jobs_verify(lambda *a: self._lib.bm_ledger_verify_jobs(self.handle, sh, *a[:4], acc, wgt, *a[4:]),
                            "bm_ledger_verify_jobs", jobs, sessions, submits, LedgerResult)


class VardiffPolicy:
    """bm_vardiff_policy_t: a share should take target_ms; a session is evaluated
    once its window is window_ms long or, with burst != 0, once it has `burst`
    accepted shares; one step multiplies the difficulty by at most max_up and
    divides it by at most max_down, inside [min_difficulty_fx, max_difficulty_fx],
    and a change within band_permille / 1000 of the old difficulty is none."""
    FIELDS = ("target_ms", "window_ms", "min_difficulty_fx", "max_difficulty_fx", "burst", "band_permille", "max_up",
              "max_down")

    def __init__(self, target_ms=10_000, window_ms=60_000, min_difficulty_fx=1, max_difficulty_fx=U64_MAX, burst=0,
                 band_permille=250, max_up=4, max_down=4):
        self.target_ms, self.window_ms = target_ms, window_ms
        self.min_difficulty_fx, self.max_difficulty_fx = min_difficulty_fx, max_difficulty_fx
        self.burst, self.band_permille, self.max_up, self.max_down = burst, band_permille, max_up, max_down

    @property
    def struct(self):
        s = VardiffPolicyStruct()
        for f, (_, t) in zip(self.FIELDS, VardiffPolicyStruct._fields_):
            v = getattr(self, f)
            top = U64_MAX if t is c_u64 else U32_MAX
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= top:
                raise ValueError(f"{f} must be in 0..{top}, got {v!r}")
            setattr(s, f, v)
        return s

    def __repr__(self):
        return "VardiffPolicy(%s)" % ", ".join(f"{f}={getattr(self, f)}" for f in self.FIELDS)


class SessionTable:
    """A bm_sessions_t: the pool's sessions -- extranonce1, share target, account
    and weight per slot -- and a SessionState per slot, kept across calls so that a
    verify call copies no session, with the vardiff step on top.
    SessionTable(ctx, capacity) lives on the first device of ctx and is closed
    before ctx; SessionTable.cpu(capacity) lives in host memory and needs no GPU:
    the specification.  Not thread-safe, and a device table shares its context's
    buffers: one call at a time per context."""

    def __init__(self, ctx, capacity: int, lib_path=None):
        self._h = None
        if not isinstance(capacity, int) or isinstance(capacity, bool) or not 1 <= capacity <= BM_MAX_POOL_SESSIONS:
            raise ValueError(f"capacity must be in 1..{BM_MAX_POOL_SESSIONS}, got {capacity!r}")
        h = ctypes.c_void_p()
        if ctx is None:
            self._lib = load(lib_path)
            check(self._lib.bm_sessions_create_cpu(capacity, ctypes.byref(h)), "bm_sessions_create_cpu")
        else:
            self._lib = ctx._lib
            check(self._lib.bm_sessions_create(ctx.handle, capacity, ctypes.byref(h)), "bm_sessions_create")
        self._ctx = ctx  # a device table must not outlive its context
        self._h = h

    @classmethod
    def cpu(cls, capacity: int, lib_path=None):
        """A table in host memory (bm_sessions_create_cpu)."""
        return cls(None, capacity, lib_path)

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("session table closed")
        return self._h

    def close(self):
        if self._h is not None:
            if self._ctx is None or self._ctx._h is not None:  # (a closed context took the device's memory with it)
                self._lib.bm_sessions_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sizes(self):
        count, capacity = c_u64(0), c_u64(0)
        check(self._lib.bm_sessions_count(self.handle, ctypes.byref(count), ctypes.byref(capacity)), "bm_sessions_count")
        return count.value, capacity.value

    @property
    def count(self) -> int:
        """1 + the highest slot set since the last clear."""
        return self._sizes()[0]

    @property
    def capacity(self) -> int:
        return self._sizes()[1]

    def clear(self):
        """count = 0 and every slot never set."""
        check(self._lib.bm_sessions_clear(self.handle), "bm_sessions_clear")

    def set(self, entries, now_ms: int, index=None):
        """Slot index[j] (index None: slot j) becomes entries[j], an
        (extranonce1, difficulty_fx, account) triple -- difficulty_fx 0 closes the
        slot -- with a fresh state whose window starts at now_ms
        (bm_sessions_set).  A slot named twice takes its later entry."""
        rows = [tuple(e) for e in entries]
        arr = (SessionInit * max(len(rows), 1))()
        for a, row in zip(arr, rows):
            if len(row) != 3:
                raise ValueError(f"an entry is (extranonce1, difficulty_fx, account), got {row!r}")
            en1, fx, account = row
            if not isinstance(en1, (bytes, bytearray)) or len(en1) > 8:
                raise ValueError(f"extranonce1 must be at most 8 bytes, got {en1!r}")
            if not isinstance(fx, int) or isinstance(fx, bool) or not 0 <= fx <= U64_MAX:
                raise ValueError(f"difficulty_fx must be in 0..2^64-1, got {fx!r}")
            ctypes.memmove(a.extranonce1, bytes(en1), len(en1))
            a.difficulty_fx, a.account = fx, _u32(account, "account")
        idx = None
        if index is not None:
            index = [_u32(i, "index") for i in index]
            if len(index) != len(rows):
                raise ValueError(f"index has one entry per session ({len(rows)}), got {len(index)}")
            idx = (c_u32 * max(len(rows), 1))(*index)
        if not isinstance(now_ms, int) or isinstance(now_ms, bool) or not 0 <= now_ms <= U64_MAX:
            raise ValueError(f"now_ms must be in 0..2^64-1, got {now_ms!r}")
        check(self._lib.bm_sessions_set(self.handle, idx, len(rows), arr, now_ms), "bm_sessions_set")

    def _range(self, first, count):
        if count is None:
            count = max(self.count - first, 0)
        for v, name in ((first, "first"), (count, "count")):
            if not isinstance(v, int) or isinstance(v, bool) or v < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
        return first, count

    def get(self, first: int = 0, count=None):
        """Slots [first, first + count) as the arrays the pool calls take ->
        ((PoolSessionStruct * count), accounts, weights); count None: up to the
        table's count (bm_sessions_get)."""
        first, count = self._range(first, count)
        ses, acc, wgt = (PoolSessionStruct * count)(), (c_u32 * count)(), (c_u64 * count)()
        check(self._lib.bm_sessions_get(self.handle, first, count, ses, acc, wgt, None), "bm_sessions_get")
        return ses, list(acc), list(wgt)

    def state(self, first: int = 0, count=None):
        """The states of slots [first, first + count) as a (SessionState * count) array."""
        first, count = self._range(first, count)
        out = (SessionState * count)()
        check(self._lib.bm_sessions_get(self.handle, first, count, None, None, None, out), "bm_sessions_get")
        return out

    def verify_jobs(self, jobs, submits, ledger=None, share_set=None):
        """Ledger.verify_jobs over the table's sessions, accounts and weights
        (bm_sessions_verify_jobs) -> (verdicts, LedgerResult); every accepted
        submission also counts in its slot's state.  ledger None: no row changes."""
        jarr, _rows = _jobs_array(jobs)
        arr = _jobs_submit_array(submits)
        if len(arr) > BM_MAX_JOB_SUBMITS:
            raise ValueError(f"at most {BM_MAX_JOB_SUBMITS} submissions per call, got {len(arr)}")
        verdicts = (JobVerdict * len(arr))()
        r = LedgerResult()
        check(self._lib.bm_sessions_verify_jobs(self.handle, ledger.handle if ledger is not None else None,
                                                share_set.handle if share_set is not None else None,
                                                jarr if len(jarr) else None, len(jarr), arr if len(arr) else None,
                                                len(arr), verdicts if len(arr) else None, ctypes.byref(r)),
              "bm_sessions_verify_jobs")
        return verdicts, r

    def retarget(self, now_ms: int, policy, cap=None):
        """One vardiff step at now_ms (bm_sessions_retarget) -> (changes, a list of
        VardiffChange ascending by session, VardiffResult); cap None: room for
        every slot.  BtcMinerError with status BM_EFULL when more than cap slots
        change: the table is as before."""
        if cap is None:
            cap = self.count
        if not isinstance(cap, int) or isinstance(cap, bool) or cap < 0:
            raise ValueError(f"cap must be a non-negative integer, got {cap!r}")
        p = policy.struct
        changes = (VardiffChange * max(cap, 1))()
        r = VardiffResult()
        check(self._lib.bm_sessions_retarget(self.handle, now_ms, ctypes.byref(p), changes if cap else None, cap,
                                             ctypes.byref(r)), "bm_sessions_retarget")
        return list(changes[: r.changed]), r


def _header_bytes(header) -> bytes:
    header = bytes(header)
    if len(header) != HEADER_BYTES:
        raise ValueError(f"a block header is {HEADER_BYTES} bytes, got {len(header)}")
    return header


def _target_bytes(target) -> bytes:
    """A target as 32 bytes, most significant first, from an int or 32 bytes."""
    if isinstance(target, int) and not isinstance(target, bool):
        if not 0 <= target <= U256_MAX:
            raise ValueError("target must be in 0..2^256-1")
        return target.to_bytes(32, "big")
    if isinstance(target, (bytes, bytearray)) and len(target) == 32:
        return bytes(target)
    raise ValueError("target must be an int in 0..2^256-1 or 32 bytes (most significant first)")


def rccl_unique_id() -> bytes:
    """RCCL unique id for a process group (rank 0 makes it, every rank
    passes it to Context(rank=..., world=..., unique_id=...))."""
    buf = ctypes.create_string_buffer(BM_RCCL_ID_BYTES)
    check(load().bm_rccl_unique_id(buf), "bm_rccl_unique_id")
    return buf.raw


class Context:
    """Owns a bm_ctx over one or more GPUs.  Not thread-safe (like the C ctx).

    Context(devices=[...]) / Context(num_gpus=N): one process, N devices.
    Context(devices=[d], rank=r, world=w): rank r of w (one process per GPU)
    outside a group: search() scans rank r's piece and returns its partial;
    join(uid) then makes it a member of the RCCL group.
    Context(devices=[d], rank=r, world=w, unique_id=uid): both steps at once
    (blocks until all w ranks join)."""

    def __init__(self, devices=None, num_gpus=0, rank=None, world=None, unique_id=None, lib_path=None):
        lib = load(lib_path)
        h = ctypes.c_void_p()
        if world is not None:
            if devices is None or len(devices) != 1 or rank is None:
                raise ValueError("a rank context takes devices=[device], rank and world")
            if unique_id is None:
                check(lib.bm_ctx_create_rank_local(devices[0], rank, world, ctypes.byref(h)),
                      "bm_ctx_create_rank_local")
            else:
                if len(unique_id) != BM_RCCL_ID_BYTES:
                    raise ValueError(f"unique_id must be {BM_RCCL_ID_BYTES} bytes")
                check(lib.bm_ctx_create_rank(devices[0], rank, world, unique_id, ctypes.byref(h)),
                      "bm_ctx_create_rank")
        elif devices is not None:
            ids = (ctypes.c_int * len(devices))(*devices)
            check(lib.bm_ctx_create_devices(ids, len(devices), ctypes.byref(h)), "bm_ctx_create_devices")
        else:
            check(lib.bm_ctx_create(num_gpus, ctypes.byref(h)), "bm_ctx_create")
        self._lib = lib
        self._h = h

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("context closed")
        return self._h

    def close(self):
        if self._h is not None:
            self._lib.bm_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_devices(self):
        n = ctypes.c_int(0)
        check(self._lib.bm_ctx_num_devices(self.handle, ctypes.byref(n)), "bm_ctx_num_devices")
        return n.value

    def rank(self):
        """(rank, world) of the context's process group ((0, 1) if none)."""
        r, w = ctypes.c_int(0), ctypes.c_int(0)
        check(self._lib.bm_ctx_rank(self.handle, ctypes.byref(r), ctypes.byref(w)), "bm_ctx_rank")
        return r.value, w.value

    def join(self, unique_id: bytes, timeout_ms: int = 0):
        """Join the RCCL group (bm_ctx_join_rank): every rank, same id."""
        if len(unique_id) != BM_RCCL_ID_BYTES:
            raise ValueError(f"unique_id must be {BM_RCCL_ID_BYTES} bytes")
        check(self._lib.bm_ctx_join_rank(self.handle, unique_id, timeout_ms), "bm_ctx_join_rank")

    def leave(self):
        check(self._lib.bm_ctx_leave_rank(self.handle), "bm_ctx_leave_rank")

    def joined(self) -> bool:
        j = ctypes.c_int(0)
        check(self._lib.bm_ctx_rank_joined(self.handle, ctypes.byref(j)), "bm_ctx_rank_joined")
        return bool(j.value)

    def set_peer_timeout(self, timeout_ms: int):
        check(self._lib.bm_ctx_set_peer_timeout(self.handle, timeout_ms), "bm_ctx_set_peer_timeout")

    def set_test_rccl_fault(self, where: int):
        check(self._lib.bm_ctx_set_test_rccl_fault(self.handle, where), "bm_ctx_set_test_rccl_fault")

    def set_test_start_delay(self, device: int, delay_us: int):
        """Test hook: hold back device `device`'s submission by delay_us at
        the start of every later search (a late-starting GPU)."""
        check(self._lib.bm_ctx_set_test_start_delay(self.handle, device, delay_us), "bm_ctx_set_test_start_delay")

    def reduce(self, pairs):
        """Lexicographic min of (hash, nonce) pairs by the GPU reductions
        (bm_reduce_gpu, a test entry)."""
        n = len(pairs)
        arr = (Result * max(n, 1))(*[Result(h, nn) for h, nn in pairs])
        r = Result()
        check(self._lib.bm_reduce_gpu(self.handle, arr, n, ctypes.byref(r)), "bm_reduce_gpu")
        return r.hash, r.nonce

    def set_test_fault(self, launches: int):
        check(self._lib.bm_ctx_set_test_fault(self.handle, launches), "bm_ctx_set_test_fault")

    def search(self, msg: bytes, lower: int, upper: int):
        """Inclusive [lower, upper] min-scan -> (hash, nonce)."""
        r = Result()
        check(self._lib.bm_search_gpu(self.handle, msg, len(msg), lower, upper, ctypes.byref(r)), "bm_search_gpu")
        return r.hash, r.nonce

    def search_target(self, msg: bytes, lower: int, upper: int, target: int):
        """The first nonce of [lower, upper] whose hash is <= target ->
        (True, hash, nonce); none -> (False, min hash, its nonce), the answer
        of search()."""
        r = TargetResult()
        check(self._lib.bm_search_target_gpu(self.handle, msg, len(msg), lower, upper, target, ctypes.byref(r)),
              "bm_search_target_gpu")
        return bool(r.found), r.hash, r.nonce

    def search_hits(self, msg: bytes, lower: int, upper: int, target: int, cap: int = 4096):
        """Every nonce of [lower, upper] whose hash is <= target ->
        (count, hits, (min hash, its nonce)): hits is the list of
        (hash, nonce) in ascending nonce order, or None when count > cap
        (nothing is returned then; count is still exact).  cap = 0 only
        counts."""
        r = HitsResult()
        buf = (Result * cap)() if cap > 0 else None
        check(self._lib.bm_search_hits_gpu(self.handle, msg, len(msg), lower, upper, target, buf, cap,
                                           ctypes.byref(r)), "bm_search_hits_gpu")
        hits = None if r.count > cap else [(buf[i].hash, buf[i].nonce) for i in range(r.stored)]
        return r.count, hits, (r.hash, r.nonce)

    def last_target_stats(self):
        """How much of the range the last search_target() handed out."""
        s = TargetStats()
        check(self._lib.bm_ctx_last_target_stats(self.handle, ctypes.byref(s)), "bm_ctx_last_target_stats")
        return s

    def search_header(self, header: bytes, nonce_lo: int = 0, nonce_hi: int = U32_MAX, target=U256_MAX):
        """Bitcoin block header: the first nonce of [nonce_lo, nonce_hi] whose
        double SHA-256 (as a little-endian 256-bit integer) is <= target ->
        (True, hash, nonce); none -> (False, hash, nonce) of the range's best
        share, the minimum of (hash >> 192, nonce).  target: an int or 32 bytes,
        most significant first.  An empty range gives (False, 2^256-1, 2^32-1)."""
        header = _header_bytes(header)
        for v, what in ((nonce_lo, "nonce_lo"), (nonce_hi, "nonce_hi")):
            if not isinstance(v, int) or not 0 <= v <= U32_MAX:
                raise ValueError(f"{what} must be in 0..2^32-1, got {v!r}")
        tgt = _target_bytes(target)
        r = HeaderResult()
        check(self._lib.bm_search_header_gpu(self.handle, header, nonce_lo, nonce_hi, tgt, ctypes.byref(r)),
              "bm_search_header_gpu")
        return bool(r.found), int.from_bytes(bytes(r.hash), "big"), r.nonce

    def search_header_versions(self, header: bytes, versions, nonce_lo: int = 0, nonce_hi: int = U32_MAX,
                               target=U256_MAX):
        """Bitcoin block header under each of `versions` (1..64 version
        fields; the header's own bytes 0..3 are ignored): the smallest nonce of
        [nonce_lo, nonce_hi] at which any version's double SHA-256 is <=
        target, and the smallest index among the versions that hit there ->
        (True, hash, nonce, version_index); none -> (False, hash, nonce,
        version_index) of the best share, the minimum of (hash >> 192, nonce,
        index).  An empty range gives (False, 2^256-1, 2^32-1, 0)."""
        header = _header_bytes(header)
        versions = list(versions)
        if not 1 <= len(versions) <= BM_MAX_HEADER_VERSIONS:
            raise ValueError(f"1..{BM_MAX_HEADER_VERSIONS} versions, got {len(versions)}")
        for v, what in [(nonce_lo, "nonce_lo"), (nonce_hi, "nonce_hi")] + [(v, "a version") for v in versions]:
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U32_MAX:
                raise ValueError(f"{what} must be in 0..2^32-1, got {v!r}")
        tgt = _target_bytes(target)
        arr = (c_u32 * len(versions))(*versions)
        r = HeaderVersionsResult()
        check(self._lib.bm_search_header_versions_gpu(self.handle, header, arr, len(versions), nonce_lo, nonce_hi,
                                                      tgt, ctypes.byref(r)), "bm_search_header_versions_gpu")
        return bool(r.found), int.from_bytes(bytes(r.hash), "big"), r.nonce, r.version_index

    def search_header_versions_hits(self, header: bytes, versions, nonce_lo: int = 0, nonce_hi: int = U32_MAX,
                                    target=U256_MAX, cap: int = 65536):
        """Bitcoin block header under each of `versions` (1..64 version fields):
        every (nonce, version index) pair of [nonce_lo, nonce_hi] whose double
        SHA-256 is <= target -> (count, hits, (best hash, best nonce, best
        index)): hits is the list of (hash, nonce, index) ascending by (nonce,
        index), or None when count > cap (nothing is returned then; count is
        still exact); the best share is search_header_versions()'s answer at
        target 0.  cap = 0 only counts.  An empty range gives
        (0, [], (2^256-1, 2^32-1, 0))."""
        header = _header_bytes(header)
        versions = list(versions)
        if not 1 <= len(versions) <= BM_MAX_HEADER_VERSIONS:
            raise ValueError(f"1..{BM_MAX_HEADER_VERSIONS} versions, got {len(versions)}")
        for v, what in [(nonce_lo, "nonce_lo"), (nonce_hi, "nonce_hi")] + [(v, "a version") for v in versions]:
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U32_MAX:
                raise ValueError(f"{what} must be in 0..2^32-1, got {v!r}")
        tgt = _target_bytes(target)
        if not isinstance(cap, int) or isinstance(cap, bool) or not 0 <= cap <= BM_MAX_HEADER_HITS:
            raise ValueError(f"cap must be in 0..{BM_MAX_HEADER_HITS}, got {cap!r}")
        arr = (c_u32 * len(versions))(*versions)
        r = HeaderVersionsHitsResult()
        buf = (HeaderVersionHit * cap)() if cap > 0 else None
        check(self._lib.bm_search_header_versions_hits_gpu(self.handle, header, arr, len(versions), nonce_lo,
                                                           nonce_hi, tgt, buf, cap, ctypes.byref(r)),
              "bm_search_header_versions_hits_gpu")
        hits = None
        if r.count <= cap:
            size = ctypes.sizeof(HeaderVersionHit)
            raw = ctypes.string_at(buf, size * r.stored) if buf is not None else b""
            hits = [(int.from_bytes(raw[o:o + 32], "big"), int.from_bytes(raw[o + 32:o + 36], "little"),
                     int.from_bytes(raw[o + 36:o + 40], "little")) for o in range(0, len(raw), size)]
        return r.count, hits, (int.from_bytes(bytes(r.hash), "big"), r.nonce, r.version_index)

    def search_job_shares(self, job, versions, en2_lo: int, en2_hi: int, nonce_lo: int = 0, nonce_hi: int = U32_MAX,
                          target=U256_MAX, cap: int = 65536, ntime=None):
        """A Stratum job under every extranonce2 of [en2_lo, en2_hi] (at most
        4096 values) and each of `versions`: every (extranonce2, nonce, version
        index) whose header hash is <= target -> (count, shares, best).  shares
        is a list of dicts (hash, extranonce2, extranonce2_size, ntime, nonce,
        version_index, version, is_block) ascending by (extranonce2, nonce,
        index), or None when count > cap (nothing is returned then; count is
        still exact, over the whole call); best is (hash, extranonce2, nonce,
        index), the minimum of (hash >> 192, extranonce2, nonce, index).  cap =
        0 only counts.  ntime defaults to the job's.  An empty range gives
        (0, [], (2^256-1, en2_lo, 2^32-1, 0))."""
        if not isinstance(job, Job):
            raise ValueError("job must be a Job")
        versions = list(versions)
        if not 1 <= len(versions) <= BM_MAX_HEADER_VERSIONS:
            raise ValueError(f"1..{BM_MAX_HEADER_VERSIONS} versions, got {len(versions)}")
        for v, what in [(nonce_lo, "nonce_lo"), (nonce_hi, "nonce_hi")] + [(v, "a version") for v in versions]:
            _u32(v, what)
        ntime = _u32(job.ntime if ntime is None else ntime, "ntime")
        for v, what in ((en2_lo, "en2_lo"), (en2_hi, "en2_hi")):
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U64_MAX:
                raise ValueError(f"{what} must be in 0..2^64-1, got {v!r}")
        if en2_lo <= en2_hi:
            job._check_extranonce2(en2_hi, "en2_hi")
            if en2_hi - en2_lo >= BM_MAX_JOB_HEADERS:
                raise ValueError(f"at most {BM_MAX_JOB_HEADERS} extranonce2 values per call, "
                                 f"got {en2_hi - en2_lo + 1}")
        tgt = _target_bytes(target)
        if not isinstance(cap, int) or isinstance(cap, bool) or not 0 <= cap <= BM_MAX_HEADER_HITS:
            raise ValueError(f"cap must be in 0..{BM_MAX_HEADER_HITS}, got {cap!r}")
        arr = (c_u32 * len(versions))(*versions)
        r = JobSharesResult()
        buf = (JobShare * cap)() if cap > 0 else None
        check(self._lib.bm_search_job_shares_gpu(self.handle, ctypes.byref(job.struct), ntime, en2_lo, en2_hi, arr,
                                                 len(versions), nonce_lo, nonce_hi, tgt, buf, cap, ctypes.byref(r)),
              "bm_search_job_shares_gpu")
        shares = None
        if r.count <= cap:
            shares = [{"hash": int.from_bytes(bytes(s.hash), "big"), "extranonce2": s.extranonce2,
                       "extranonce2_size": job.extranonce2_size, "ntime": s.ntime, "nonce": s.nonce,
                       "version_index": s.version_index, "version": s.version, "is_block": bool(s.is_block)}
                      for s in (buf[i] for i in range(r.stored))]
        return r.count, shares, (int.from_bytes(bytes(r.hash), "big"), r.extranonce2, r.nonce, r.version_index)

    def verify_submits(self, job, submits, target):
        """A batch of mining.submit tuples of a Stratum job against a share
        target, one GPU lane per submission (bm_job_verify_gpu, at most 2^20 per
        call) -> (verdicts, result).  submits: a (JobSubmit * n) array, or an
        iterable of dicts with extranonce2, ntime, nonce and version (the full
        header version: parse_submit's answer, or a share of search_job_shares)
        or of such 4-tuples.  verdicts is a (JobVerdict * n) array in the
        caller's order: hash (.value as an integer) and status (is_share: hash
        <= target; is_block: hash <= the target of the job's nbits; is_invalid:
        extranonce2 does not fit its field, nothing hashed); result is a
        JobVerifyResult with n and the count of each flag."""
        return _verify(lambda *a: self._lib.bm_job_verify_gpu(self.handle, *a), "bm_job_verify_gpu", job, submits,
                       target)

    def verify_pool_submits(self, job, sessions, submits, ntime_lo: int = 0, ntime_hi: int = U32_MAX):
        """One job's submissions from many sessions in one call, one GPU lane per
        submission (bm_pool_verify_gpu) -> (verdicts, result).  sessions: an
        iterable of PoolSession (or (extranonce1, target) pairs), each
        extranonce1 as long as job.extranonce1, whose bytes are not used
        otherwise; submits: a (PoolSubmit * n) array, or an iterable of dicts
        with extranonce2, ntime, nonce, version and session (parse_pool_submit's
        answer) or of such 5-tuples.  A verdict is verify_submits' with is_share
        against the session's own target, is_ntime for an ntime outside
        [ntime_lo, ntime_hi] (hashed all the same), and is_invalid also for a
        session index past the table; result is a PoolVerifyResult."""
        return _pool_verify(lambda *a: self._lib.bm_pool_verify_gpu(self.handle, *a), "bm_pool_verify_gpu", job,
                            sessions, submits, ntime_lo, ntime_hi)

    def verify_jobs_submits(self, jobs, sessions, submits):
        """The submissions of several live jobs in one call, one GPU lane per
        submission (bm_jobs_verify_gpu) -> (verdicts, result).  jobs: up to 64
        PoolJob (a Job and its own ntime window; a bare Job has no window);
        sessions: as verify_pool_submits takes them, shared by all jobs, each
        extranonce1 at least as long as the longest the jobs state (a job reads
        its first bytes); submits: a (JobsSubmit * n) array, or an iterable of
        dicts with extranonce2, ntime, nonce, version, session and job
        (parse_jobs_submit's answer) or of such 6-tuples.  verdicts[i] is
        verify_pool_submits' for submission i under its job and that job's
        window, in the caller's order; a job index past the table is_invalid."""
        return _jobs_verify(lambda *a: self._lib.bm_jobs_verify_gpu(self.handle, *a), "bm_jobs_verify_gpu", jobs,
                            sessions, submits)

    def search_header_hits(self, header: bytes, nonce_lo: int = 0, nonce_hi: int = U32_MAX, target=U256_MAX,
                           cap: int = 4096):
        """Bitcoin block header: every nonce of [nonce_lo, nonce_hi] whose
        double SHA-256 is <= target -> (count, hits, (best hash, best nonce)):
        hits is the list of (hash, nonce) in ascending nonce order, or None
        when count > cap (nothing is returned then; count is still exact);
        the best share is search_header()'s answer at target 0.  cap = 0 only
        counts.  An empty range gives (0, [], (2^256-1, 2^32-1))."""
        header = _header_bytes(header)
        for v, what in ((nonce_lo, "nonce_lo"), (nonce_hi, "nonce_hi")):
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= U32_MAX:
                raise ValueError(f"{what} must be in 0..2^32-1, got {v!r}")
        tgt = _target_bytes(target)
        if not isinstance(cap, int) or isinstance(cap, bool) or not 0 <= cap <= BM_MAX_HEADER_HITS:
            raise ValueError(f"cap must be in 0..{BM_MAX_HEADER_HITS}, got {cap!r}")
        r = HeaderHitsResult()
        buf = (HeaderHit * cap)() if cap > 0 else None
        check(self._lib.bm_search_header_hits_gpu(self.handle, header, nonce_lo, nonce_hi, tgt, buf, cap,
                                                  ctypes.byref(r)), "bm_search_header_hits_gpu")
        hits = None
        if r.count <= cap:
            raw = bytes(buf)[:ctypes.sizeof(HeaderHit) * r.stored] if buf is not None else b""
            hits = [(int.from_bytes(raw[o:o + 32], "big"), int.from_bytes(raw[o + 32:o + 36], "little"))
                    for o in range(0, len(raw), ctypes.sizeof(HeaderHit))]
        return r.count, hits, (int.from_bytes(bytes(r.hash), "big"), r.nonce)

    def header_hash_many(self, header: bytes, nonces):
        """The header's double SHA-256 under each nonce, as integers (the
        digest read little-endian), on the first device."""
        header = _header_bytes(header)
        nonces = list(nonces)
        for v in nonces:
            if not 0 <= v <= U32_MAX:
                raise ValueError(f"a nonce must be in 0..2^32-1, got {v!r}")
        n = len(nonces)
        arr = (c_u32 * max(n, 1))(*nonces)
        out = (ctypes.c_uint8 * (32 * max(n, 1)))()
        check(self._lib.bm_header_hash_gpu(self.handle, header, arr, n, out), "bm_header_hash_gpu")
        raw = bytes(out)
        return [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(n)]

    def hash_many(self, msg: bytes, nonces):
        n = len(nonces)
        arr = (c_u64 * max(n, 1))(*nonces)
        out = (c_u64 * max(n, 1))()
        check(self._lib.bm_hash_gpu(self.handle, msg, len(msg), arr, n, out), "bm_hash_gpu")
        return list(out[:n])

    def set_timing(self, on: bool):
        check(self._lib.bm_ctx_set_timing(self.handle, 1 if on else 0), "bm_ctx_set_timing")

    def set_combine(self, mode: int):
        check(self._lib.bm_ctx_set_combine(self.handle, mode), "bm_ctx_set_combine")

    def set_task_digits(self, digits: int):
        check(self._lib.bm_ctx_set_task_digits(self.handle, digits), "bm_ctx_set_task_digits")

    def set_max_windows(self, n: int):
        check(self._lib.bm_ctx_set_max_windows(self.handle, n), "bm_ctx_set_max_windows")

    def set_blocks_per_cu(self, n: int):
        check(self._lib.bm_ctx_set_blocks_per_cu(self.handle, n), "bm_ctx_set_blocks_per_cu")

    def set_split(self, shares):
        """Integer shares, one per slot (devices, or ranks of the group; the
        same on every rank), for the range partitioner; None: near-equal."""
        shares = list(shares or [])
        arr = (ctypes.c_uint32 * max(len(shares), 1))(*shares)
        check(self._lib.bm_ctx_set_split(self.handle, arr, len(shares)), "bm_ctx_set_split")

    def get_split(self):
        """The shares the next search will use ([] when near-equal)."""
        n = ctypes.c_int(0)
        check(self._lib.bm_ctx_get_split(self.handle, None, 0, ctypes.byref(n)), "bm_ctx_get_split")
        arr = (ctypes.c_uint32 * max(n.value, 1))()
        check(self._lib.bm_ctx_get_split(self.handle, arr, n.value, ctypes.byref(n)), "bm_ctx_get_split")
        return list(arr[: n.value])

    def set_balance(self, on: bool):
        """Multi-device contexts: shares follow each device's measured rate."""
        check(self._lib.bm_ctx_set_balance(self.handle, 1 if on else 0), "bm_ctx_set_balance")

    def last_stats(self):
        s = Stats()
        check(self._lib.bm_ctx_last_stats(self.handle, ctypes.byref(s)), "bm_ctx_last_stats")
        return s
