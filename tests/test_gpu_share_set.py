"""bm_share_set_verify on a device set against hashlib plus a Python set
(tests/share_set_ref.py), never against the library itself, but where a test says
so: the CPU set as a second witness.  Every comparison is exact equality of every
verdict and of the result struct; the scenarios are the CPU set's
(tests/test_share_set_abi.py)."""
import ctypes
import io
import os
import random

import pytest

from conftest import GOLDEN, load_golden
from distributed_bitcoin_minter_amd import BtcMinerError, Job, PoolSession, ShareSet, _lib, pool_dedup
import pool_verify_ref as ref
import share_set_ref as sref

pytestmark = pytest.mark.gpu

JOB_PATH = os.path.join(GOLDEN, "stratum_genesis_job.json")
SESSIONS_PATH = os.path.join(GOLDEN, "stratum_genesis_sessions.json")
JOB = load_golden("stratum_genesis_job.json")
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
GENESIS_PARAMS = '["satoshi.1","genesis","001d","495fab29","7c2bac1d","00000000"]'
BLOCK_LINE = "Block %s %064x" % (GENESIS_PARAMS, GENESIS_HASH)


def device_set(ctx):
    return lambda capacity: ShareSet(ctx, capacity)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_one_wave_and_beyond(gpu_ctx, n):
    """Around the workgroup of 64 and beyond one: about a third of the entries
    repeat earlier ones, exactly the first occurrence is unflagged, and a canary
    verdict past n stays."""
    sref.batch_edges(device_set(gpu_ctx), n)


def test_contention(gpu_ctx):
    """One submission in all 64 lanes of the first workgroup and in lanes of the
    next two: only index 0 of the copies is unflagged; the same batch again is all
    duplicates, records nothing and leaves the count."""
    sref.contention(device_set(gpu_ctx))


def test_forced_collisions_and_wrap_around(gpu_ctx):
    """16 slots, home slots 14, 15, 15, 15, 0: the probe chain wraps past the table's
    end; a second call queries them in another order among new hashes of the same
    home slots; a third finds all of a full table."""
    sref.forced_collisions(device_set(gpu_ctx))


def test_capacity_edges(gpu_ctx):
    """Capacity 8 holding 5: three new fit, four do not, 65 exhaust the probes of
    the 16 slots: BM_EFULL with canaries intact, the count unchanged, and a follow-up
    batch that behaves as the Python set that never saw the refused one."""
    sref.capacity_edges(device_set(gpu_ctx))


def test_across_calls(gpu_ctx):
    """Three batches of 5,000 over 500 sessions on a set of 2^16: the device set
    against the Python reference, and against the CPU set as a second witness."""
    sref.across_calls(device_set(gpu_ctx), witness=ShareSet.cpu)


def test_key_is_the_hash(gpu_ctx):
    sref.key_is_the_hash(device_set(gpu_ctx))


def test_lifecycle(gpu_ctx):
    """clear() forgets, two sets on one context are independent, and a set survives
    a verify_pool_submits call and a search_header call on its context (they share
    the context's buffers and stream)."""
    rng = random.Random(31)
    job = ref.synthetic_job(rng, 45, 4, 4, 250, 2)
    sessions = ref.synthetic_sessions(rng, 4)
    big = ref.random_subs(rng, 4, 3000, 7)
    genesis = Job.from_notify(JOB["notify"], JOB["extranonce1"], JOB["extranonce2_size"])

    def between():
        verdicts, _ = gpu_ctx.verify_pool_submits(job, ref.session_array(sessions), ref.sub_array(big))
        assert (verdicts[0].value, verdicts[0].status) == ref.verdict(job, sessions, big[0])
        assert not any(v.status & sref.DUPLICATE for v in verdicts)
        assert gpu_ctx.search_header(genesis.header(29), 2083236608, 2083237119, 0xffff << 208) == (True, GENESIS_HASH, 2083236893)

    sref.lifecycle(device_set(gpu_ctx), between)


def test_refusals_on_a_device_set(gpu_ctx):
    """BM_EINVAL leaves a device set and the canaries alone; the context's own
    refusals hold for its sets."""
    job = Job.from_notify(JOB["notify"], JOB["extranonce1"], JOB["extranonce2_size"])
    sessions = [PoolSession(b"\xff\xff", 0xffff << 208)]
    good = [(29, job.ntime, 2083236893, 1, 0)]
    with ShareSet(gpu_ctx, 4) as s:
        assert (s.count, s.capacity) == (0, 4)
        model = sref.Model(4)
        assert sref.check(s, model, job, sessions, good)[0] == [(GENESIS_HASH, 3)]
        verdicts = (_lib.JobVerdict * 1)()
        ctypes.memset(verdicts, 0xA5, 40)
        r = _lib.ShareSetResult()
        ctypes.memset(ctypes.byref(r), 0x5A, 64)
        bad = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
        bad.extranonce1_len = 9
        f = gpu_ctx._lib.bm_share_set_verify
        ses, arr = ref.session_array(sessions), ref.sub_array(good)
        assert f(s.handle, ctypes.byref(bad), ses, 1, arr, 1, 0, ref.U32, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
        assert f(s.handle, ctypes.byref(job.struct), None, 1, arr, 1, 0, ref.U32, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
        assert f(s.handle, ctypes.byref(job.struct), ses, 1, arr, 1, 0, ref.U32, verdicts, None) == _lib.BM_EINVAL
        assert bytes(verdicts) == b"\xa5" * 40 and bytes(r) == b"\x5a" * 64 and s.count == 1
        assert sref.check(s, model, job, sessions, good * 2)[0] == [(GENESIS_HASH, 3 | 16)] * 2
        with pytest.raises(BtcMinerError) as e:
            s.verify(job, [PoolSession(b"\xff\xff", ref.U256)], [(i, 2, 3, 4, 0) for i in range(4)])
        assert e.value.status == _lib.BM_EFULL and s.count == 1


def run(ctx, text, *flags):
    out = io.StringIO()
    rc = pool_dedup.main([JOB_PATH, SESSIONS_PATH, "-", *flags], out=out, ctx=ctx, stdin=io.StringIO(text))
    return rc, out.getvalue().splitlines()


def test_pool_dedup_on_the_gpu(gpu_ctx):
    """The README's example, in one call on the set and across two."""
    want = [BLOCK_LINE, "Reject duplicate " + GENESIS_PARAMS, "Verified 2 Accepted 1 Blocks 1 Rejected 1 Duplicates 1"]
    text = GENESIS_PARAMS + "\n" + BLOCK_LINE + "\n"
    assert run(gpu_ctx, text) == (0, want)
    assert run(gpu_ctx, text, "--batch", "1") == (0, want)
    other = GENESIS_PARAMS.replace("satoshi.1", "hal.1")
    mixed = "\n".join([other, GENESIS_PARAMS, "hello", other, GENESIS_PARAMS, GENESIS_PARAMS]) + "\n"
    lines = ["Reject above-target " + other, BLOCK_LINE, "Reject malformed hello", "Reject above-target " + other,
             "Reject duplicate " + GENESIS_PARAMS, "Reject duplicate " + GENESIS_PARAMS,
             "Verified 6 Accepted 1 Blocks 1 Rejected 5 Duplicates 2"]
    assert run(gpu_ctx, mixed) == (0, lines)
    assert run(gpu_ctx, mixed, "--batch", "1") == (0, lines)
    assert run(gpu_ctx, mixed, "--batch", "4", "--capacity", "1") == (0, lines)
