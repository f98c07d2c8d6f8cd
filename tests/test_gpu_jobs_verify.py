"""bm_jobs_verify_gpu on a gfx950 device: jobs_verify_kernel behind the host
grouping, against hashlib (tests/jobs_verify_ref.py) over the same scenarios as the
CPU entry (tests/test_jobs_verify_abi.py), a witness against bm_pool_verify_gpu per
job, the CPU entry on a large batch, and context reuse."""
import ctypes
import random

import pytest

from conftest import load_golden
from distributed_bitcoin_minter_amd import Job, _lib, verify_jobs_submits_cpu
import jobs_verify_ref as jref
import pool_verify_ref as ref

pytestmark = pytest.mark.gpu

GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f


def gpu_call(ctx):
    f = ctx._lib.bm_jobs_verify_gpu
    return lambda *a: f(ctx.handle, *a)


@pytest.mark.parametrize("n", jref.BATCH_SIZES)
def test_round_robin_batches(gpu_ctx, n):
    """A kernel that took the job from lane 0, or from the first record of a
    64-stride block of the caller's batch, passes single-job batches and fails these."""
    jref.round_robin(gpu_call(gpu_ctx), n)


@pytest.mark.parametrize("counts", jref.PER_JOB_COUNTS)
def test_per_job_counts(gpu_ctx, counts):
    jref.per_job_counts(gpu_call(gpu_ctx), counts)


def test_all_on_the_last_job(gpu_ctx):
    jref.last_job_only(gpu_call(gpu_ctx))


def test_malformed_unused_job_is_refused(gpu_ctx):
    jref.malformed_unused_job(gpu_call(gpu_ctx))


def test_unknown_jobs_among_valid_entries(gpu_ctx):
    jref.unknown_jobs(gpu_call(gpu_ctx))


def test_no_jobs_and_unknown_sessions(gpu_ctx):
    jref.no_jobs_and_unknown_sessions(gpu_call(gpu_ctx))


def test_verdicts_do_not_depend_on_the_arrangement(gpu_ctx):
    jref.arrangement(gpu_call(gpu_ctx))


def test_empty_batch(gpu_ctx):
    jobs, sessions = jref.three_jobs()
    rc, out, r = jref.raw(gpu_call(gpu_ctx), jobs, sessions, [])
    assert rc == _lib.BM_OK and ref.result_tuple(r) == (0,) * 5 and bytes(out) == b"\xa5" * 40


def test_witness_against_the_single_job_entry(gpu_ctx):
    """For each job, the verdicts of its submissions equal bm_pool_verify_gpu's on that job alone."""
    jobs, sessions = jref.three_jobs()
    rng = random.Random(8000)
    subs = jref.job_subs(rng, jobs, len(sessions), [rng.randrange(3) for _ in range(300)])
    got, _ = gpu_ctx.verify_jobs_submits(jobs, sessions, jref.sub_array(subs))
    views = jref.session_views(jobs, sessions)
    for j, pj in enumerate(jobs):
        mine = [i for i, s in enumerate(subs) if s[5] == j]
        assert len(mine) > 64
        alone, _ = gpu_ctx.verify_pool_submits(pj.job, views[j], [subs[i][:5] for i in mine], pj.ntime_lo, pj.ntime_hi)
        assert [bytes(got[i]) for i in mine] == [bytes(v) for v in alone], j


def test_gpu_against_the_cpu_entry_and_hashlib(gpu_ctx):
    """5,000 submissions over 8 jobs and 500 sessions, with above-target and INVALID entries."""
    jobs, sessions, subs, want = jref.large_case()
    arr = jref.sub_array(subs)
    got, r = gpu_ctx.verify_jobs_submits(jobs, sessions, arr)
    cpu, rc = verify_jobs_submits_cpu(jobs, sessions, arr)
    assert bytes(got) == bytes(cpu) and bytes(r) == bytes(rc)
    assert ref.as_tuples(got) == want and ref.result_tuple(r) == ref.counts(want)


def test_context_reuse(gpu_ctx):
    """Interleaved with verify_pool_submits and search_header on one context: the buffers are shared."""
    jobs, sessions = jref.three_jobs()
    views = jref.session_views(jobs, sessions)
    gj = load_golden("stratum_genesis_job.json")
    genesis = Job.from_notify(gj["notify"], gj["extranonce1"], gj["extranonce2_size"])
    rng = random.Random(10000)
    call = gpu_call(gpu_ctx)
    for n in (200, 3, 129):
        subs = jref.job_subs(rng, jobs, len(sessions), [rng.randrange(4) for _ in range(n)])
        jref.check(call, jobs, sessions, subs)
        one = [s[:5] for s in subs if s[5] == 1]
        got, _ = gpu_ctx.verify_pool_submits(jobs[1].job, views[1], one, 5, 7)
        assert ref.as_tuples(got) == [ref.verdict(jobs[1].job, views[1], s, 5, 7) for s in one]
        assert gpu_ctx.search_header(genesis.header(29), 2083236608, 2083237119, 0xffff << 208) == (
            True, GENESIS_HASH, 2083236893)
        jref.check(call, jobs, sessions, subs[::-1])


def test_python_call_and_refusal_keep_the_context(gpu_ctx):
    jobs, sessions = jref.three_jobs()
    with pytest.raises(ValueError):
        gpu_ctx.verify_jobs_submits([jobs[0]] * 65, sessions, [(1, 2, 3, 4, 0, 0)])
    bad, _keep = _lib._jobs_array(jobs)
    bad[2].job.extranonce2_size = 0
    out = (_lib.JobVerdict * 1)()
    r = _lib.PoolVerifyResult()
    assert gpu_ctx._lib.bm_jobs_verify_gpu(gpu_ctx.handle, bad, 3, ref.session_array(sessions), 7,
                                           jref.sub_array([(1, 2, 3, 4, 0, 0)]), 1, out, ctypes.byref(r)) == _lib.BM_EINVAL
    v, r = gpu_ctx.verify_jobs_submits(jobs, sessions, [(1, 1000, 3, 4, 0, 0), (1, 2, 3, 4, 0, 3)])
    assert ref.as_tuples(v) == jref.verdicts(jobs, sessions, [(1, 1000, 3, 4, 0, 0), (1, 2, 3, 4, 0, 3)])
