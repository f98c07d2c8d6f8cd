"""bm_pool_verify_gpu on the GPU against hashlib (tests/pool_verify_ref.py), never
against the library itself, but for the two tests that say so: the witness against
bm_job_verify_gpu and the comparison with the CPU entry.  The layout grid (900
jobs x 65 submissions over 7 sessions) is hashed once per process and shared with
the CPU entry's test."""
import ctypes
import random

import pytest

from conftest import load_golden
from distributed_bitcoin_minter_amd import Job, PoolSession, _lib, roll_versions, verify_pool_submits_cpu
import pool_verify_ref as ref
from pool_verify_ref import invalid_case, ladder_case, window_cases
import verify_ref

pytestmark = pytest.mark.gpu

JOB = load_golden("stratum_genesis_job.json")
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
U256 = ref.U256
LIMIT = _lib.BM_MAX_JOB_COINBASE


def genesis_job():
    return Job.from_notify(JOB["notify"], JOB["extranonce1"], JOB["extranonce2_size"])


def check(ctx, job, sessions, subs, lo=0, hi=ref.U32, want=None):
    """One call; every verdict and the counts against hashlib."""
    want = [ref.verdict(job, sessions, s, lo, hi) for s in subs] if want is None else want
    verdicts, r = ctx.verify_pool_submits(job, ref.session_array(sessions), ref.sub_array(subs), lo, hi)
    assert ref.as_tuples(verdicts) == want
    assert ref.result_tuple(r) == ref.counts(want)
    return want


# ---- layouts ---------------------------------------------------------------------------

def test_layout_grid(gpu_ctx):
    """The field's offset mod 64 x whole blocks before it x both sizes x the
    coinbase's length mod 64: every word and block edge the field can meet (16
    bytes at offsets 47 and 63 span five words; the block edge falls inside
    extranonce1, between the fields and inside extranonce2) and every padding
    edge, under per-session targets and an ntime window."""
    grid = ref.layout_grid()
    assert len(grid) == 900
    flagged = 0
    for label, job, sessions, subs, want in grid:
        verdicts, r = gpu_ctx.verify_pool_submits(job, ref.session_array(sessions), ref.sub_array(subs), *ref.GRID_WINDOW)
        assert ref.as_tuples(verdicts) == want, label
        assert ref.result_tuple(r) == ref.counts(want), label
        flagged += r.blocks
    assert flagged > 0  # some BLOCK flags were checked (and went through the host's tripwire)


@pytest.mark.parametrize("depth", [0, 1, 12, 32])
def test_branch_depths(gpu_ctx, depth):
    rng = random.Random(100 + depth)
    job = ref.synthetic_job(rng, 45, 4, 4, 250, depth)
    check(gpu_ctx, job, ref.synthetic_sessions(rng, 4), ref.random_subs(rng, 4, 65, 7))


@pytest.mark.parametrize("bulk", ["coinb2", "coinb1"])
def test_coinbase_limit(gpu_ctx, bulk):
    """BM_MAX_JOB_COINBASE bytes: the field near the front (the device runs its
    block and the 1,024 after it) or near the end (the host's midstate covers the
    bulk, the device runs two blocks)."""
    rng = random.Random(len(bulk))
    pos = 39 if bulk == "coinb2" else LIMIT - 30
    job = ref.synthetic_job(rng, pos, 8, 8, LIMIT, 1)
    assert len(job.coinb1) + 8 + 8 + len(job.coinb2) == LIMIT
    check(gpu_ctx, job, ref.synthetic_sessions(rng, 8), ref.random_subs(rng, 8, 65, 7))


# ---- batch edges and the session table ---------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_edges(gpu_ctx, n):
    """Around the workgroup of 64 and beyond one block; a canary verdict beyond n stays."""
    rng = random.Random(n)
    job = ref.synthetic_job(rng, 61, 8, 8, 130, 2)
    sessions = ref.synthetic_sessions(rng, 8)
    subs = ref.random_subs(rng, 8, max(n, 2), 7)[:n]
    want = [ref.verdict(job, sessions, s) for s in subs]
    verdicts = (_lib.JobVerdict * (n + 1))()
    ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
    r = _lib.PoolVerifyResult()
    rc = gpu_ctx._lib.bm_pool_verify_gpu(gpu_ctx.handle, ctypes.byref(job.struct), ref.session_array(sessions), 7,
                                         ref.sub_array(subs), n, 0, ref.U32, verdicts, ctypes.byref(r))
    assert rc == _lib.BM_OK
    assert ref.as_tuples(verdicts, n) == want and ref.result_tuple(r) == ref.counts(want)
    assert bytes(verdicts[n]) == b"\xa5" * 40


def test_empty_batch(gpu_ctx):
    job = genesis_job()
    verdicts, r = gpu_ctx.verify_pool_submits(job, [PoolSession(b"\xff\xff", 0)], [])
    assert len(verdicts) == 0 and ref.result_tuple(r) == (0,) * 5
    canary = (_lib.JobVerdict * 1)()
    ctypes.memset(canary, 0xA5, 40)
    r = _lib.PoolVerifyResult()
    assert gpu_ctx._lib.bm_pool_verify_gpu(gpu_ctx.handle, ctypes.byref(job.struct), None, 0, ref.sub_array([(1, 2, 3, 4, 0)]),
                                           0, 0, ref.U32, canary, ctypes.byref(r)) == _lib.BM_OK
    assert bytes(canary) == b"\xa5" * 40 and ref.result_tuple(r) == (0,) * 5


def test_large_session_table(gpu_ctx):
    """2^16 + 1 sessions: the table's ends and the index past 2^16 - 1, the first
    index past the table, and a full wave in which every lane has another session."""
    rng = random.Random(21)
    nses = (1 << 16) + 1
    job = ref.synthetic_job(rng, 50, 4, 4, 180, 1)
    sessions = [PoolSession(rng.randbytes(4), (1 << 255) if i % 2 else (1 << 254)) for i in range(nses)]
    picks = [0, (1 << 16) - 1, 1 << 16, nses] + [rng.randrange(nses) for _ in range(60)]
    wave = rng.sample(range(nses), 64)
    subs = [(rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), s) for s in picks + wave]
    assert len(subs) == 128 and len(set(wave)) == 64
    want = check(gpu_ctx, job, sessions, subs)
    assert want[3] == ref.INVALID_VERDICT and all(w != ref.INVALID_VERDICT for w in want[:3] + want[4:])


# ---- the compares ------------------------------------------------------------------------

def test_per_session_targets(gpu_ctx):
    """One hash under 29 sessions whose targets sit at H - 1, H, H + 1, at each
    32-bit word's edges and at the extremes: SHARE flips exactly at equality, per
    lane."""
    job, sessions, subs, expect = ladder_case()
    assert check(gpu_ctx, job, sessions, subs) == expect


def test_block_without_share(gpu_ctx):
    rng = random.Random(13)
    job = ref.synthetic_job(rng, 10, 4, 4, 100, 0, nbits=0x2100ffff)
    sessions = [PoolSession(rng.randbytes(4), 0), PoolSession(rng.randbytes(4), U256)]
    subs = ref.random_subs(rng, 4, 65, 2)
    want = check(gpu_ctx, job, sessions, subs)
    assert {st for (_, st), s in zip(want, subs) if s[4] == 0} == {2}
    for nbits in (0x1d80ffff, 0x2300ffff):  # an nbits that does not decode leaves BLOCK clear
        job = ref.synthetic_job(rng, 10, 4, 4, 100, 0, nbits=nbits)
        assert {st for _, st in check(gpu_ctx, job, sessions, subs)} == {0, 1}


def test_ntime_window(gpu_ctx):
    rng = random.Random(17)
    job = ref.synthetic_job(rng, 70, 2, 2, 150, 1)
    sessions = [PoolSession(rng.randbytes(2), U256), PoolSession(rng.randbytes(2), 0)]
    for lo, hi, subs, flagged in window_cases():
        want = check(gpu_ctx, job, sessions, subs, lo, hi)
        assert [bool(st & ref.NTIME) for _, st in want] == flagged, (lo, hi)


def test_invalid_entries(gpu_ctx):
    job, sessions, subs = invalid_case()
    want = check(gpu_ctx, job, sessions, subs, 100, 200)  # an INVALID entry first and last: the tripwire sees both
    assert want[0] == want[-1] == ref.INVALID_VERDICT and want[1][1] == 9
    # an INVALID-only batch, and no sessions at all
    only = [s for s, w in zip(subs, want) if w == ref.INVALID_VERDICT]
    assert len(only) == 50
    check(gpu_ctx, job, sessions, only)
    assert all(w == ref.INVALID_VERDICT for w in check(gpu_ctx, job, [], subs))


# ---- witnesses -----------------------------------------------------------------------------

def test_witness_against_the_single_session_entry(gpu_ctx):
    """With one session equal to (job.extranonce1, T) and the window open, the
    verdict bytes are bm_job_verify_gpu's on the same submissions: a second
    witness, not the reference (hashlib checks both elsewhere)."""
    rng = random.Random(23)
    job = verify_ref.synthetic_job(rng, 57, 3, 300, 12)
    assert len(job.extranonce1) == 4
    subs = verify_ref.random_subs(rng, 3, 300) + [(1 << 24, 1, 2, 3), (ref.U64, 1, 2, 3)]
    old_v, old_r = gpu_ctx.verify_submits(job, verify_ref.sub_array(subs), verify_ref.GRID_TARGET)
    new_v, new_r = gpu_ctx.verify_pool_submits(job, [PoolSession(job.extranonce1, verify_ref.GRID_TARGET)],
                                               ref.sub_array([s + (0,) for s in subs]))
    assert bytes(new_v) == bytes(old_v)
    assert ref.result_tuple(new_r) == verify_ref.result_tuple(old_r) + (0,) and new_r.invalid == 2


def test_gpu_against_the_cpu_entry(gpu_ctx):
    """The two entries are byte-identical on 10,000 random submissions over 500
    sessions, INVALID ones of both kinds included, and so is *out (hashlib
    checks a sample of them here, and all of each entry's answers elsewhere)."""
    rng = random.Random(15)
    job = ref.synthetic_job(rng, 57, 5, 3, 300, 12)
    sessions = [PoolSession(rng.randbytes(5), rng.choice((1 << 255, 1 << 254, U256, 0))) for _ in range(500)]
    subs = [(rng.getrandbits(24) if rng.random() < 0.95 else rng.getrandbits(64), rng.getrandbits(32), rng.getrandbits(32),
             rng.getrandbits(32), rng.randrange(500) if rng.random() < 0.95 else rng.randrange(500, 1 << 32))
            for _ in range(10000)]
    ses, arr = ref.session_array(sessions), ref.sub_array(subs)
    gpu_v, gpu_r = gpu_ctx.verify_pool_submits(job, ses, arr, *ref.GRID_WINDOW)
    cpu_v, cpu_r = verify_pool_submits_cpu(job, ses, arr, *ref.GRID_WINDOW)
    assert bytes(gpu_v) == bytes(cpu_v) and bytes(gpu_r) == bytes(cpu_r)
    assert 500 < gpu_r.invalid < 1500 and gpu_r.shares > 2000 and gpu_r.blocks > 0 and gpu_r.ntime > 3000
    for i in range(0, 10000, 97):
        assert (gpu_v[i].value, gpu_v[i].status) == ref.verdict(job, sessions, subs[i], *ref.GRID_WINDOW)


# ---- the context ---------------------------------------------------------------------------

def test_context_reuse(gpu_ctx):
    """A refused call, then a good one; small, large, small on one context; a
    search_header call and a bm_job_verify_gpu call in between leave the answers as
    they were (the two verifiers share the context's buffers)."""
    rng = random.Random(16)
    job = ref.synthetic_job(rng, 45, 4, 4, 250, 2)
    sessions = ref.synthetic_sessions(rng, 4)
    subs = ref.random_subs(rng, 4, 200, 7)
    verdicts = (_lib.JobVerdict * 200)()
    ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
    r = _lib.PoolVerifyResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    f, h = gpu_ctx._lib.bm_pool_verify_gpu, gpu_ctx.handle
    bad = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
    bad.extranonce1_len = 9
    ses, arr = ref.session_array(sessions), ref.sub_array(subs)
    assert f(h, ctypes.byref(bad), ses, 7, arr, 200, 0, ref.U32, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
    assert f(h, ctypes.byref(job.struct), None, 7, arr, 200, 0, ref.U32, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
    assert f(h, ctypes.byref(job.struct), ses, _lib.BM_MAX_POOL_SESSIONS + 1, arr, 200, 0, ref.U32, verdicts,
             ctypes.byref(r)) == _lib.BM_EINVAL
    assert bytes(verdicts) == b"\xa5" * (40 * 200) and bytes(r) == b"\x5a" * 40
    first = check(gpu_ctx, job, sessions, subs)
    header = genesis_job().header(29)
    assert gpu_ctx.search_header(header, 2083236608, 2083237119, 0xffff << 208) == (True, GENESIS_HASH, 2083236893)
    stats = bytes(gpu_ctx.last_stats())
    assert check(gpu_ctx, job, sessions, subs) == first
    assert bytes(gpu_ctx.last_stats()) == stats  # a verify call leaves the last statistics alone
    big = ref.random_subs(rng, 4, 3000, 7)
    check(gpu_ctx, job, sessions, big)
    assert check(gpu_ctx, job, sessions, subs) == first
    gjob = genesis_job()
    old, _ = gpu_ctx.verify_submits(gjob, [(29, gjob.ntime, 2083236893, 1)], 0xffff << 208)
    assert (old[0].value, old[0].status) == (GENESIS_HASH, 3)
    assert check(gpu_ctx, job, sessions, subs) == first


# ---- round trips ---------------------------------------------------------------------------

def test_round_trip_of_mined_shares(gpu_ctx):
    """Every share search_job_shares finds on the genesis job verifies as a SHARE
    with the same hash under the session that holds the job's extranonce1, BLOCK
    exactly where is_block; under a session with another extranonce1 none
    verifies.  hashlib agrees with all of it."""
    job = genesis_job()
    target = (1 << (256 - 12)) - 1  # 12 zero bits
    count, shares, _best = gpu_ctx.search_job_shares(job, roll_versions(1, 4), 28, 31, 0, (1 << 16) - 1, target)
    assert count == len(shares) > 16
    count1, block, _ = gpu_ctx.search_job_shares(job, [1], 29, 29, 2083236608, 2083237119, 0xffff << 208)
    assert count1 == 1 and block[0]["is_block"]
    shares = shares + block
    sessions = [PoolSession(b"\x00\x01", target), PoolSession(job.extranonce1, target)]  # (the golden sessions file's two)
    mine = [(s["extranonce2"], s["ntime"], s["nonce"], s["version"], 1) for s in shares]
    want = check(gpu_ctx, job, sessions, mine)
    assert [h for h, _ in want] == [s["hash"] for s in shares]
    assert [st for _, st in want] == [3 if s["is_block"] else 1 for s in shares] and want[-1] == (GENESIS_HASH, 3)
    theirs = [s[:4] + (0,) for s in mine]
    assert all(st == 0 for _, st in check(gpu_ctx, job, sessions, theirs))
