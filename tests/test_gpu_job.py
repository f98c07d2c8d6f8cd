"""bm_search_job_shares_gpu on the GPU against hashlib, never against the library
itself: every header is rebuilt here from the job's pieces (coinbase, branch
fold, field order) and every hash is sha256d of those 80 bytes read as a
little-endian integer.  The brute force of the enumeration cases (3 extranonce2
values x 2 versions x 16384 nonces = 98,304 hashes, once per branch) is computed
once and shared; the figures asserted beside the full lists are hashlib's."""
import ctypes
import functools
import hashlib
import struct

import pytest

from conftest import load_golden
from distributed_bitcoin_minter_amd import Context, Job, _lib, difficulty_to_target, roll_versions

pytestmark = pytest.mark.gpu

JOB = load_golden("stratum_genesis_job.json")
U32 = (1 << 32) - 1
U64 = (1 << 64) - 1
U256 = (1 << 256) - 1
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
BRANCH2 = [hashlib.sha256(b"branch 0").digest(), hashlib.sha256(b"branch 1").digest()]
VERS = roll_versions(1, 2)
EN2 = (28, 30)
NONCES = (0, 16383)
T = (1 << 246) - 1
BLOCK_TARGET = 0xffff << 208  # nbits 1d00ffff


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def make_job(branch=(), size=None):
    n = list(JOB["notify"])
    n[4] = [b.hex() for b in branch]
    return Job.from_notify(n, JOB["extranonce1"], JOB["extranonce2_size"] if size is None else size)


def prefix_of(job, en2, version, ntime=None):
    """The first 76 header bytes, from the job's pieces with hashlib."""
    root = sha256d(job.coinb1 + job.extranonce1 + en2.to_bytes(job.extranonce2_size, "big") + job.coinb2)
    for entry in job.branch:
        root = sha256d(root + entry)
    return struct.pack("<I", version) + job.prevhash + root + struct.pack("<II", job.ntime if ntime is None else ntime,
                                                                          job.nbits)


def scan(job, versions, en2_lo, en2_hi, lo, hi):
    """Every (hash, extranonce2, nonce, index) of the box, ascending by (extranonce2, nonce, index)."""
    out = []
    for e in range(en2_lo, en2_hi + 1):
        pre = [prefix_of(job, e, v) for v in versions]
        for n in range(lo, hi + 1):
            tail = struct.pack("<I", n)
            out += [(int.from_bytes(sha256d(p + tail), "little"), e, n, i) for i, p in enumerate(pre)]
    return out


@functools.lru_cache(maxsize=None)
def brute(with_branch=False):
    return tuple(scan(make_job(BRANCH2 if with_branch else ()), VERS, *EN2, *NONCES))


def best_of(rows):
    return min(rows, key=lambda s: (s[0] >> 192, s[1], s[2], s[3]))


def tup(share):
    return share["hash"], share["extranonce2"], share["nonce"], share["version_index"]


def check_fields(job, versions, shares, ntime=None):
    for s in shares:
        assert s["version"] == versions[s["version_index"]] and s["extranonce2_size"] == job.extranonce2_size
        assert s["ntime"] == (job.ntime if ntime is None else ntime)
        assert s["is_block"] == (s["hash"] <= BLOCK_TARGET)


def _raw(ctx, job, versions, en2_lo, en2_hi, lo, hi, target, buf, cap, out, ntime=None):
    arr = (ctypes.c_uint32 * len(versions))(*versions)
    return ctx._lib.bm_search_job_shares_gpu(ctx.handle, ctypes.byref(job.struct), job.ntime if ntime is None else ntime,
                                             en2_lo, en2_hi, arr, len(versions), lo, hi, target.to_bytes(32, "big"),
                                             buf, cap, ctypes.byref(out))


# ---- 1. genesis from its job ---------------------------------------------------------

def test_genesis_from_its_job(gpu_ctx):
    job = make_job()
    lo, hi = 2083236608, 2083237119
    target = difficulty_to_target(JOB["difficulty"])
    rows = scan(job, [1], 29, 29, lo, hi)
    want = [s for s in rows if s[0] <= target]
    assert want == [(GENESIS_HASH, 29, 2083236893, 0)]
    count, shares, best = gpu_ctx.search_job_shares(job, [1], 29, 29, lo, hi, target)
    assert count == 1 and [tup(s) for s in shares] == want and best == want[0] == best_of(rows)
    assert shares[0]["is_block"] is True and shares[0]["ntime"] == 0x495fab29 and shares[0]["version"] == 1
    # the neighbouring extranonce2 values hold no share in that window
    assert gpu_ctx.search_job_shares(job, [1], 28, 30, lo, hi, target)[:2] == (1, shares)


# ---- 2. enumeration ------------------------------------------------------------------

def test_enumeration(gpu_ctx):
    job = make_job()
    rows = brute()
    assert len(rows) == 98304
    want = [s for s in rows if s[0] <= T]
    assert len(want) == 91
    assert [sum(1 for s in want if (s[1], s[3]) == (e, i)) for e in (28, 29, 30) for i in (0, 1)] == [10, 15, 21, 15, 21, 9]
    b = best_of(rows)
    assert (b[0] >> 192, b[1], b[2], b[3]) == (91486837953700, 28, 15969, 1)
    count, shares, best = gpu_ctx.search_job_shares(job, VERS, *EN2, *NONCES, T)
    assert count == 91 and [tup(s) for s in shares] == want and best == b
    assert all(tup(x)[1:] < tup(y)[1:] for x, y in zip(shares, shares[1:]))
    check_fields(job, VERS, shares)
    assert not any(s["is_block"] for s in shares)
    # the stats are the last inner call's: one header, one launch of two versions
    st = gpu_ctx.last_stats()
    assert st.launches == 1 and st.nonces == 2 * 16384
    # another ntime is another set of headers
    rows2 = [(int.from_bytes(sha256d(prefix_of(job, 28, v, 0x495fab2a) + struct.pack("<I", n)), "little"), 28, n, i)
             for n in range(0, 4096) for i, v in enumerate(VERS)]
    count, shares, best = gpu_ctx.search_job_shares(job, VERS, 28, 28, 0, 4095, T, ntime=0x495fab2a)
    assert [tup(s) for s in shares] == [s for s in rows2 if s[0] <= T] and count == len(shares) and best == best_of(rows2)
    check_fields(job, VERS, shares, 0x495fab2a)


def test_enumeration_with_a_branch(gpu_ctx):
    job = make_job(BRANCH2)
    rows = brute(True)
    want = [s for s in rows if s[0] <= T]
    b = best_of(rows)
    assert len(want) == 116 and b[1:] == (29, 6496, 0)
    count, shares, best = gpu_ctx.search_job_shares(job, VERS, *EN2, *NONCES, T)
    assert count == 116 and [tup(s) for s in shares] == want and best == b
    check_fields(job, VERS, shares)


# ---- 3. all or nothing over the whole call -------------------------------------------

def test_all_or_nothing(gpu_ctx):
    job = make_job()
    want = [s for s in brute() if s[0] <= T]
    b = best_of(brute())
    per_header = [sum(1 for s in want if s[1] == e) for e in (28, 29, 30)]
    assert per_header == [25, 36, 30]
    # 90: one short.  25: the first header alone fills it.  20, 1: the first header alone overflows it.
    # 61: the first two headers fill it exactly
    for cap in (90, 61, 25, 20, 1):
        r = _lib.JobSharesResult()
        buf = (_lib.JobShare * cap)()
        ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
        before = bytes(buf)
        assert _raw(gpu_ctx, job, VERS, *EN2, *NONCES, T, buf, cap, r) == _lib.BM_OK
        assert (r.count, r.stored, r.headers) == (91, 0, 3), cap
        assert bytes(buf) == before, cap
        assert (int.from_bytes(bytes(r.hash), "big"), r.extranonce2, r.nonce, r.version_index) == b
        assert gpu_ctx.search_job_shares(job, VERS, *EN2, *NONCES, T, cap) == (91, None, b)
    for cap in (91, 92):
        r = _lib.JobSharesResult()
        buf = (_lib.JobShare * cap)()
        ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
        assert _raw(gpu_ctx, job, VERS, *EN2, *NONCES, T, buf, cap, r) == _lib.BM_OK
        assert (r.count, r.stored, r.headers, r.reserved, r.version) == (91, 91, 3, 0, VERS[b[3]])
        got = [(int.from_bytes(bytes(s.hash), "big"), s.extranonce2, s.nonce, s.version_index) for s in buf[:91]]
        assert got == want and all(s.reserved == 0 and s.ntime == job.ntime for s in buf[:91])
        assert bytes(buf)[91 * 64:] == b"\x5a" * (64 * (cap - 91))
    # a pure count: no buffer
    r = _lib.JobSharesResult()
    assert _raw(gpu_ctx, job, VERS, *EN2, *NONCES, T, None, 0, r) == _lib.BM_OK
    assert (r.count, r.stored, r.headers) == (91, 0, 3)
    assert gpu_ctx.search_job_shares(job, VERS, *EN2, *NONCES, T, 0) == (91, None, b)
    assert gpu_ctx.search_job_shares(job, VERS, *EN2, *NONCES, 0, 0) == (0, [], b)


# ---- 4. edges ------------------------------------------------------------------------

def test_empty_ranges(gpu_ctx):
    job = make_job()
    for en2, nonces in (((30, 28), NONCES), (EN2, (5, 4)), ((30, 28), (5, 4))):
        r = _lib.JobSharesResult()
        ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
        buf = (_lib.JobShare * 4)()
        ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
        assert _raw(gpu_ctx, job, VERS, *en2, *nonces, U256, buf, 4, r) == _lib.BM_OK
        assert bytes(r.hash) == b"\xff" * 32 and (r.nonce, r.extranonce2, r.version_index, r.version) == \
            (U32, en2[0], 0, VERS[0])
        assert (r.count, r.stored, r.headers, r.reserved) == (0, 0, 0, 0)
        assert bytes(buf) == b"\x5a" * ctypes.sizeof(buf)
        assert gpu_ctx.search_job_shares(job, VERS, *en2, *nonces, U256) == (0, [], (U256, en2[0], U32, 0))
        assert gpu_ctx.last_stats().launches == 0


def test_last_extranonce2_values_of_size_8(gpu_ctx):
    """[2^64-2, 2^64-1]: the loop ends on the last value and does not wrap."""
    job = make_job(size=8)
    lo, hi = 1000, 1511
    rows = scan(job, VERS, U64 - 1, U64, lo, hi)
    target = (1 << 251) - 1
    want = [s for s in rows if s[0] <= target]
    assert 20 <= len(want) <= 120 and {s[1] for s in want} == {U64 - 1, U64}
    count, shares, best = gpu_ctx.search_job_shares(job, VERS, U64 - 1, U64, lo, hi, target)
    assert count == len(want) and [tup(s) for s in shares] == want and best == best_of(rows)
    r = _lib.JobSharesResult()
    assert _raw(gpu_ctx, job, VERS, U64 - 1, U64, lo, hi, target, None, 0, r) == _lib.BM_OK and r.headers == 2


def test_top_of_the_nonce_space(gpu_ctx):
    job = make_job()
    lo, hi = U32 - 511, U32
    rows = scan(job, VERS, 28, 29, lo, hi)
    target = (1 << 251) - 1
    want = [s for s in rows if s[0] <= target]
    assert len(want) >= 20 and any(s[2] >= U32 - 64 for s in want)
    count, shares, best = gpu_ctx.search_job_shares(job, VERS, 28, 29, lo, hi, target)
    assert count == len(want) and [tup(s) for s in shares] == want and best == best_of(rows)
    assert gpu_ctx.last_stats().nonces == 2 * 512  # no wrap past 2^32-1


def test_too_many_headers_refused(gpu_ctx):
    job = make_job()
    r = _lib.JobSharesResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    before = bytes(r)
    assert _raw(gpu_ctx, job, VERS, 0, 4096, 0, 0, U256, None, 0, r) == _lib.BM_EINVAL  # 4097 values
    assert _raw(gpu_ctx, job, VERS, 0xfff0, 0x10000, 0, 0, U256, None, 0, r) == _lib.BM_EINVAL  # past the 2-byte field
    assert bytes(r) == before
    with Context(devices=[0], rank=1, world=2) as ctx:
        with pytest.raises(_lib.BtcMinerError) as ei:
            ctx.search_job_shares(job, VERS, 28, 28, 0, 100, 0)
        assert ei.value.status == _lib.BM_EINVAL
    # 4096 values are legal: with an empty nonce range the checks pass and nothing is scanned
    assert _raw(gpu_ctx, job, VERS, 0, 4095, 5, 4, U256, None, 0, r) == _lib.BM_OK and r.headers == 0
    assert _raw(gpu_ctx, job, VERS, 0xf001, 0xffff, 5, 4, U256, None, 0, r) == _lib.BM_OK
    assert _raw(gpu_ctx, job, VERS, 0, 4096, 5, 4, U256, None, 0, r) == _lib.BM_EINVAL
    # a long loop: 300 headers of one nonce each
    target = (1 << 252) - 1
    count, shares, best = gpu_ctx.search_job_shares(job, [1], 100, 399, 7, 7, target, 300)
    rows = scan(job, [1], 100, 399, 7, 7)
    assert count == len(shares) and [tup(s) for s in shares] == [s for s in rows if s[0] <= target]
    assert 5 <= count <= 60 and best == best_of(rows)


def test_failed_call_leaves_outputs_and_context_alone(gpu_ctx):
    job = make_job()
    r = _lib.JobSharesResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    buf = (_lib.JobShare * 128)()
    ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
    before = bytes(r), bytes(buf)
    gpu_ctx.set_test_fault(0)
    try:
        assert _raw(gpu_ctx, job, VERS, *EN2, *NONCES, T, buf, 128, r) == _lib.BM_EINTERNAL
        assert (bytes(r), bytes(buf)) == before
    finally:
        gpu_ctx.set_test_fault(-1)
    assert gpu_ctx.search(b"bradfitz", 0, 9999) == (1419516646206828, 9898)
    want = [s for s in brute() if s[0] <= T]
    count, shares, best = gpu_ctx.search_job_shares(job, VERS, *EN2, *NONCES, T, 128)
    assert count == 91 and [tup(s) for s in shares] == want and best == best_of(brute())


# ---- 5. split invariance -------------------------------------------------------------

def test_split_and_grouping_invariance(gpu_ctx, monkeypatch):
    job = make_job()
    want = gpu_ctx.search_job_shares(job, VERS, *EN2, *NONCES, T)
    assert want[0] == 91 and [tup(s) for s in want[1]] == [s for s in brute() if s[0] <= T]
    with Context(devices=[0, 0, 0]) as ctx:
        assert ctx.search_job_shares(job, VERS, *EN2, *NONCES, T) == want
        assert ctx.last_stats().devices == 3 and ctx.last_stats().launches == 3
        ctx.set_split([1, 5, 2])
        assert ctx.search_job_shares(job, VERS, *EN2, *NONCES, T) == want
    monkeypatch.setenv("BTCMINER_HEADER_GROUP", "1")  # read when a context is created
    with Context(devices=[0]) as ctx:
        assert ctx.search_job_shares(job, VERS, *EN2, *NONCES, T) == want
        assert ctx.last_stats().launches == 2  # one launch per version


# ---- 6. composition ------------------------------------------------------------------

def test_equals_the_per_header_calls(gpu_ctx):
    """The job call is the version-rolling share enumeration, header by header."""
    job = make_job()
    want = gpu_ctx.search_job_shares(job, VERS, *EN2, *NONCES, T)
    merged, bests = [], []
    for e in range(EN2[0], EN2[1] + 1):
        header = job.header(e)
        assert header[:76] == prefix_of(job, e, job.version)
        count, hits, (h, n, i) = gpu_ctx.search_header_versions_hits(header, VERS, *NONCES, T)
        merged += [(hh, e, nn, ii) for hh, nn, ii in hits]
        bests.append((h, e, n, i))
    assert [tup(s) for s in want[1]] == merged and want[0] == len(merged) == 91
    assert want[2] == best_of(bests)
