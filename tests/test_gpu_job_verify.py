"""bm_job_verify_gpu on the GPU against hashlib (tests/verify_ref.py), never
against the library itself: every verdict is rebuilt from the job's pieces
(coinbase, branch fold, field order) and sha256d of the 80 bytes.  The layout
grid (400 jobs x 65 submissions) is hashed once per process and shared with the
CPU entry's test; the one test that compares the two entries says so."""
import ctypes
import random

import pytest

from conftest import load_golden
from distributed_bitcoin_minter_amd import Context, Job, _lib, roll_versions, verify_submits_cpu
import verify_ref as ref

pytestmark = pytest.mark.gpu

JOB = load_golden("stratum_genesis_job.json")
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
U256 = ref.U256
LIMIT = _lib.BM_MAX_JOB_COINBASE


def genesis_job():
    return Job.from_notify(JOB["notify"], JOB["extranonce1"], JOB["extranonce2_size"])


def check(ctx, job, subs, target, want=None):
    """One call; every verdict and the counts against hashlib."""
    want = [ref.verdict(job, target, s) for s in subs] if want is None else want
    verdicts, r = ctx.verify_submits(job, ref.sub_array(subs), target)
    assert ref.as_tuples(verdicts) == want
    assert ref.result_tuple(r) == ref.counts(want)
    return want


# ---- layouts ---------------------------------------------------------------------------

def test_layout_grid(gpu_ctx):
    """extranonce2's offset mod 64 x whole blocks before it x its size x the
    coinbase's length mod 64: every word and block edge extranonce2 can meet
    (size 8 at offsets 57, 61, 63 crosses a block edge and spans three words)
    and every padding edge."""
    grid = ref.layout_grid()
    assert len(grid) == 400
    flagged = 0
    for label, job, subs, want in grid:
        verdicts, r = gpu_ctx.verify_submits(job, ref.sub_array(subs), ref.GRID_TARGET)
        assert ref.as_tuples(verdicts) == want, label
        assert ref.result_tuple(r) == ref.counts(want), label
        flagged += r.blocks
    assert flagged > 0  # some BLOCK flags were checked (and went through the host's tripwire)


@pytest.mark.parametrize("depth", [0, 1, 2, 12, 32])
def test_branch_depths(gpu_ctx, depth):
    rng = random.Random(100 + depth)
    job = ref.synthetic_job(rng, 45, 4, 250, depth)
    check(gpu_ctx, job, ref.random_subs(rng, 4, 65), ref.GRID_TARGET)


@pytest.mark.parametrize("bulk", ["coinb2", "coinb1"])
def test_coinbase_limit(gpu_ctx, bulk):
    """BM_MAX_JOB_COINBASE bytes: the bulk after extranonce2 (the device runs
    extranonce2's block and the 1,024 after it) or before it (the host's
    midstate covers it, the device runs two blocks)."""
    rng = random.Random(len(bulk))
    pos = 42 if bulk == "coinb2" else LIMIT - 30
    job = ref.synthetic_job(rng, pos, 8, LIMIT, 1)
    assert len(job.coinb1) + len(job.extranonce1) + 8 + len(job.coinb2) == LIMIT
    check(gpu_ctx, job, ref.random_subs(rng, 8, 65), ref.GRID_TARGET)


# ---- batch edges -----------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_edges(gpu_ctx, n):
    """Around the workgroup of 64 and beyond one block; a canary verdict beyond n stays."""
    rng = random.Random(n)
    job = ref.synthetic_job(rng, 61, 8, 130, 2)
    subs = ref.random_subs(rng, 8, max(n, 2))[:n]
    want = [ref.verdict(job, ref.GRID_TARGET, s) for s in subs]
    verdicts = (_lib.JobVerdict * (n + 1))()
    ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
    r = _lib.JobVerifyResult()
    rc = gpu_ctx._lib.bm_job_verify_gpu(gpu_ctx.handle, ctypes.byref(job.struct), ref.GRID_TARGET.to_bytes(32, "big"),
                                        ref.sub_array(subs), n, verdicts, ctypes.byref(r))
    assert rc == _lib.BM_OK
    assert ref.as_tuples(verdicts, n) == want and ref.result_tuple(r) == ref.counts(want)
    assert bytes(verdicts[n]) == b"\xa5" * 40


def test_empty_batch(gpu_ctx):
    job = genesis_job()
    verdicts, r = gpu_ctx.verify_submits(job, [], 0)
    assert len(verdicts) == 0 and ref.result_tuple(r) == (0, 0, 0, 0)
    canary = (_lib.JobVerdict * 1)()
    ctypes.memset(canary, 0xA5, 40)
    r = _lib.JobVerifyResult()
    assert gpu_ctx._lib.bm_job_verify_gpu(gpu_ctx.handle, ctypes.byref(job.struct), bytes(32), ref.sub_array([(1, 2, 3, 4)]),
                                          0, canary, ctypes.byref(r)) == _lib.BM_OK
    assert bytes(canary) == b"\xa5" * 40 and ref.result_tuple(r) == (0, 0, 0, 0)


# ---- the compares ----------------------------------------------------------------------

def _nbits_of(target):
    """The compact form of a target, or None when it has none (more than three
    significant bytes, or a mantissa with the sign bit)."""
    if target == 0:
        return None
    size = (target.bit_length() + 7) // 8
    mant = target >> (8 * (size - 3)) if size >= 3 else target << (8 * (3 - size))
    nbits = (size << 24) | mant
    return nbits if not mant & 0x800000 and ref.block_target(nbits) == target else None


def test_compare_ladder(gpu_ctx):
    """One submission with hash H; per 32-bit word k (0 = least significant):
    H + 2^32k with the lower words zero (set), H - 2^32k with the lower words all
    ones (clear), bit 31 of word k flipped (set when that raises the target), and
    H itself (set).  Each target once as the share target and, where a compact
    nbits can express it, once as the block target.  (A random hash has four
    significant bytes in its top word and nbits has three, so few rungs have a
    compact form; the block compare's words are pinned by
    test_block_compare_word_by_word and by the genesis block, whose compare is
    decided in the second word.)"""
    rng = random.Random(11)
    base = ref.synthetic_job(rng, 45, 4, 120, 1)
    sub = (0x01020304, 5, 6, 7)
    H, base_status = ref.verdict(base, 0, sub)
    words = [(H >> (32 * k)) & ref.U32 for k in range(8)]
    assert all(0 < w < ref.U32 for w in words)  # every rung exists for this hash
    rungs = [(H, True)]
    for k in range(8):
        rungs.append((((H >> (32 * k)) + 1) << (32 * k), True))                            # one above, lower words zero
        rungs.append(((((H >> (32 * k)) - 1) << (32 * k)) | ((1 << (32 * k)) - 1), False))  # one below, lower words ones
        rungs.append((H ^ (1 << (32 * k + 31)), not words[k] >> 31))                        # bit 31 of word k flipped
    assert len(rungs) == 25
    for t, is_set in rungs:
        assert (H <= t) == is_set
        assert check(gpu_ctx, base, [sub], t) == [(H, base_status | (1 if is_set else 0))], hex(t)
        # the same target as the block target, where a compact nbits can express it.  nbits is part of the
        # header, so the hash is another one; hashlib decides the flag, and the share target says the opposite
        nbits = _nbits_of(t)
        if nbits is not None:
            job = Job(base.coinb1, base.extranonce1, 4, base.coinb2, base.branch, base.prevhash, base.version, nbits,
                      base.ntime)
            h2 = ref.verdict(job, 0, sub)[0]
            share_t = 0 if h2 <= t else U256
            assert check(gpu_ctx, job, [sub], share_t) == [(h2, 2 if h2 <= t else 1)]


def test_block_compare_word_by_word(gpu_ctx):
    """The block compare at each word: nbits whose target's three mantissa bytes
    sit at every byte position, against 64 hashes each; hashlib decides.  Low
    positions give no BLOCK, the top ones give some: both answers occur."""
    rng = random.Random(12)
    seen = set()
    for exp in range(3, 35):
        mant = 0x00ffff if exp >= 33 else 0x7fffff
        job = ref.synthetic_job(rng, 3, 7, 64, 0, nbits=(exp << 24) | mant)
        want = check(gpu_ctx, job, ref.random_subs(rng, 7, 64), 1 << 254)
        seen |= {st for _, st in want}
    assert seen == {0, 1, 2, 3}


def test_flag_independence(gpu_ctx):
    """The share target below and the block target above the hash: BLOCK without SHARE."""
    rng = random.Random(13)
    job = ref.synthetic_job(rng, 10, 4, 100, 0, nbits=0x2100ffff)
    subs = ref.random_subs(rng, 4, 65)
    want = check(gpu_ctx, job, subs, 0)
    assert sum(1 for _, st in want if st == 2) >= 64 and all(st in (0, 2) for _, st in want)
    # an nbits that does not decode leaves BLOCK clear everywhere
    for nbits in (0x1d80ffff, 0x2300ffff):
        job = ref.synthetic_job(rng, 10, 4, 100, 0, nbits=nbits)
        want = check(gpu_ctx, job, subs, U256)
        assert all(st == 1 for _, st in want)


def test_invalid_entries(gpu_ctx):
    rng = random.Random(14)
    job = ref.synthetic_job(rng, 70, 2, 150, 1)
    subs = [(0x10000, 1, 2, 3), (0xffff, 1, 2, 3), (ref.U64, 1, 2, 3), (5, 6, 7, 8), (1 << 63, 1, 2, 3)] * 13
    want = check(gpu_ctx, job, subs, U256)  # an INVALID entry first: the host's recompute of entry 0 sees it
    assert want[0] == want[2] == want[4] == ref.INVALID_VERDICT and want[1][1] & 1
    verdicts, r = gpu_ctx.verify_submits(job, subs, U256)
    assert bytes(verdicts[0].hash) == b"\xff" * 32 and verdicts[0].status == 4 and r.invalid == 39
    job8 = ref.synthetic_job(rng, 61, 8, 130, 0)
    want = check(gpu_ctx, job8, [(ref.U64, 1, 2, 3), (ref.U64 - 1, 1, 2, 3)], U256)
    assert all(st & 1 for _, st in want)


# ---- round trips -----------------------------------------------------------------------

def _mined(ctx):
    job = genesis_job()
    versions = roll_versions(1, 4)
    target = (1 << (256 - 12)) - 1  # 12 zero bits
    count, shares, _best = ctx.search_job_shares(job, versions, 28, 31, 0, (1 << 16) - 1, target)
    assert count == len(shares) > 16
    return job, target, shares


def test_round_trip_of_mined_shares(gpu_ctx):
    """Every share search_job_shares finds on the genesis job verifies as a SHARE
    with the same hash, and BLOCK exactly where is_block; hashlib agrees."""
    job, target, shares = _mined(gpu_ctx)
    verdicts, r = gpu_ctx.verify_submits(job, shares, target)
    assert [v.value for v in verdicts] == [s["hash"] for s in shares]
    assert all(v.is_share and not v.is_invalid for v in verdicts)
    assert [v.is_block for v in verdicts] == [s["is_block"] for s in shares]
    assert ref.result_tuple(r) == (len(shares), len(shares), sum(s["is_block"] for s in shares), 0)
    subs = [(s["extranonce2"], s["ntime"], s["nonce"], s["version"]) for s in shares]
    assert ref.as_tuples(verdicts) == [ref.verdict(job, target, s) for s in subs]


def test_tampered_round_trip(gpu_ctx):
    """The same shares with one field off by one in 16 of them are no longer
    shares; hashlib decides the rare one that still is."""
    job, target, shares = _mined(gpu_ctx)
    subs = [[s["extranonce2"], s["ntime"], s["nonce"], s["version"]] for s in shares]
    tampered = list(range(0, len(subs), len(subs) // 16))[:16]
    for j, i in enumerate(tampered):
        subs[i][j % 4] += 1  # extranonce2, ntime, nonce and version in turn
    subs = [tuple(s) for s in subs]
    want = check(gpu_ctx, job, subs, target)
    lost = [i for i, (_, st) in enumerate(want) if not st & 1]
    assert set(lost) <= set(tampered) and len(lost) >= 15
    assert all(want[i][0] != shares[i]["hash"] for i in tampered)


def test_gpu_against_the_cpu_entry(gpu_ctx):
    """The two entries are byte-identical on 10,000 random submissions, INVALID
    ones included, and so is *out (hashlib checks a sample of them here, and all
    of each entry's answers elsewhere)."""
    rng = random.Random(15)
    job = ref.synthetic_job(rng, 57, 3, 300, 12)
    subs = [(rng.getrandbits(24) if rng.random() < 0.9 else rng.getrandbits(64), rng.getrandbits(32), rng.getrandbits(32),
             rng.getrandbits(32)) for _ in range(10000)]
    arr = ref.sub_array(subs)
    gpu_v, gpu_r = gpu_ctx.verify_submits(job, arr, ref.GRID_TARGET)
    cpu_v, cpu_r = verify_submits_cpu(job, arr, ref.GRID_TARGET)
    assert bytes(gpu_v) == bytes(cpu_v) and bytes(gpu_r) == bytes(cpu_r)
    assert 500 < gpu_r.invalid < 1500 and gpu_r.shares > 4000 and gpu_r.blocks > 0
    for i in range(0, 10000, 97):
        assert (gpu_v[i].value, gpu_v[i].status) == ref.verdict(job, ref.GRID_TARGET, subs[i])


# ---- the context -----------------------------------------------------------------------

def test_context_reuse(gpu_ctx):
    """A refused call, then a good one; a search between two verify calls leaves both as they were;
    bm_ctx_last_stats is the search's."""
    rng = random.Random(16)
    job = ref.synthetic_job(rng, 45, 4, 250, 2)
    subs = ref.random_subs(rng, 4, 200)
    verdicts = (_lib.JobVerdict * 200)()
    ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
    r = _lib.JobVerifyResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    f, h = gpu_ctx._lib.bm_job_verify_gpu, gpu_ctx.handle
    bad = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
    bad.extranonce2_size = 9
    tgt = ref.GRID_TARGET.to_bytes(32, "big")
    assert f(h, ctypes.byref(bad), tgt, ref.sub_array(subs), 200, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
    assert f(h, ctypes.byref(job.struct), tgt, ref.sub_array(subs), _lib.BM_MAX_JOB_SUBMITS + 1, verdicts,
             ctypes.byref(r)) == _lib.BM_EINVAL
    assert f(h, ctypes.byref(job.struct), None, ref.sub_array(subs), 200, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
    assert bytes(verdicts) == b"\xa5" * (40 * 200) and bytes(r) == b"\x5a" * 32
    first = check(gpu_ctx, job, subs, ref.GRID_TARGET)
    gjob = genesis_job()
    count, shares, _ = gpu_ctx.search_job_shares(gjob, [1], 29, 29, 2083236608, 2083237119, 0xffff << 208)
    assert count == 1 and shares[0]["hash"] == GENESIS_HASH
    stats = bytes(gpu_ctx.last_stats())
    assert check(gpu_ctx, job, subs, ref.GRID_TARGET) == first
    assert bytes(gpu_ctx.last_stats()) == stats  # a verify call leaves the last statistics alone
    assert check(gpu_ctx, gjob, [(29, gjob.ntime, 2083236893, 1)], 0xffff << 208) == [(GENESIS_HASH, 3)]
    # a bigger batch after a smaller one (the device buffer grows), then the small one again
    big = ref.random_subs(rng, 4, 3000)
    check(gpu_ctx, job, big, ref.GRID_TARGET)
    assert check(gpu_ctx, job, subs, ref.GRID_TARGET) == first


def test_rank_context_of_a_group_is_refused():
    job = genesis_job()
    with Context(devices=[0], rank=0, world=2) as ctx:
        r = _lib.JobVerifyResult()
        ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
        verdicts = (_lib.JobVerdict * 1)()
        assert ctx._lib.bm_job_verify_gpu(ctx.handle, ctypes.byref(job.struct), bytes(32), ref.sub_array([(1, 2, 3, 4)]), 1,
                                          verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
        assert bytes(r) == b"\x5a" * 32
    with Context(devices=[0], rank=0, world=1) as ctx:  # a group of one is a plain context
        assert ref.as_tuples(ctx.verify_submits(job, [(29, job.ntime, 2083236893, 1)], 0xffff << 208)[0]) == \
            [(GENESIS_HASH, 3)]
