"""bm_share_set_verify_jobs on a device set (gfx950): jobs_verify_kernel's verdicts
through the share set's four kernels, against hashlib and a Python set
(tests/jobs_verify_ref.py), the same scenarios as on a CPU set
(tests/test_jobs_verify_abi.py)."""
import ctypes

import pytest

from distributed_bitcoin_minter_amd import ShareSet, _lib
import jobs_verify_ref as jref
import pool_verify_ref as ref

pytestmark = pytest.mark.gpu


def device_set(ctx):
    return lambda capacity: ShareSet(ctx, capacity)


@pytest.mark.parametrize("scenario", [jref.set_across_batches, jref.set_identical_jobs, jref.set_repeat_across_groups,
                                      jref.set_full, jref.set_alternating], ids=lambda f: f.__name__)
def test_device_share_set(gpu_ctx, scenario):
    scenario(device_set(gpu_ctx))


def test_device_set_against_a_cpu_set_on_a_large_batch(gpu_ctx):
    """5,000 submissions over 8 jobs, fed twice: the second pass is all duplicates
    where eligible; a CPU set gives the same bytes."""
    jobs, sessions, subs, _want = jref.large_case()
    with ShareSet(gpu_ctx, 1 << 14) as s, ShareSet.cpu(1 << 14) as c:
        model = jref.Model(1 << 14)
        for _ in range(2):
            want, r = jref.set_check(s, model, jobs, sessions, list(subs))
            v, cr = c.verify_jobs(jobs, sessions, jref.sub_array(subs))
            assert ref.as_tuples(v) == want and jref.ss.result_tuple(cr) == r
        assert r[6] == 0 and r[5] == sum(1 for _, st in want if jref.ss.eligible(st)) > 1000


def test_refusals_on_a_device_set(gpu_ctx):
    jobs, sessions = jref.open_jobs()
    with ShareSet(gpu_ctx, 4) as s:
        f = gpu_ctx._lib.bm_share_set_verify_jobs
        bad, _keep = _lib._jobs_array(jobs)
        bad[1].job.nbranch = 33
        rc, out, r = jref.raw(lambda *a: f(s.handle, *a), (bad, 3), sessions, [(1, 2, 3, 4, 0, 0)],
                              result=_lib.ShareSetResult)
        assert rc == _lib.BM_EINVAL and bytes(out) == b"\xa5" * 80 and bytes(r) == b"\x5a" * 64 and s.count == 0
        r = _lib.ShareSetResult()
        assert f(s.handle, bad, 3, None, 0, None, 0, None, ctypes.byref(r)) == _lib.BM_EINVAL
        v, r = s.verify_jobs(jobs, sessions, [(1, 2, 3, 4, 0, 0), (1, 2, 3, 4, 0, 0)])
        assert [x.status for x in v] == [1, 17] and s.count == 1
