"""The reference and scenarios of verification over several jobs, shared by the CPU
and the GPU tests of bm_jobs_verify_cpu / bm_jobs_verify_gpu / bm_share_set_verify_jobs.
The reference is never the library: it is tests/pool_verify_ref.verdict (hashlib),
applied per submission with that submission's job and that job's window, plus a
Python set of hashes for the share set (tests/share_set_ref.Model).  A scenario
takes `call`, the C entry with everything before `jobs` bound, so the same cases run
on both entries; every comparison is exact equality of every verdict's (hash,
status, reserved) and of the result struct, with a canary verdict past n."""
import ctypes
import functools
import random

from distributed_bitcoin_minter_amd import PoolJob, PoolSession, _lib
import pool_verify_ref as ref
import share_set_ref as ss
from pool_verify_ref import U32, U256
from verify_ref import INVALID_VERDICT

DUPLICATE = ss.DUPLICATE
UNDECODABLE_NBITS = 0x1d80ffff  # the sign bit of the mantissa: no block target


def session_views(jobs, sessions):
    """Per job the session table as that job reads it: the first extranonce1_len
    bytes of every session's extranonce1."""
    return [[PoolSession(s.extranonce1[:len(pj.job.extranonce1)], s.target) for s in sessions] for pj in jobs]


def verdicts(jobs, sessions, subs):
    """[(hash, status)] of (extranonce2, ntime, nonce, version, session, job) tuples with hashlib."""
    views = session_views(jobs, sessions)
    return [INVALID_VERDICT if s[5] >= len(jobs) else
            ref.verdict(jobs[s[5]].job, views[s[5]], s[:5], jobs[s[5]].ntime_lo, jobs[s[5]].ntime_hi) for s in subs]


def sub_array(subs, junk=0xDEADBEEF):
    """The submissions as the C ABI takes them; `reserved` is junk, which must not count."""
    arr = (_lib.JobsSubmit * len(subs))()
    for a, (en2, ntime, nonce, version, session, job) in zip(arr, subs):
        a.extranonce2, a.ntime, a.nonce, a.version, a.session, a.job, a.reserved = en2, ntime, nonce, version, session, job, junk
    return arr


def raw(call, jobs, sessions, subs, n=None, result=_lib.PoolVerifyResult):
    """One call through the C ABI into canary-filled arrays, one verdict longer than
    the batch -> (status, verdicts, result).  jobs: PoolJob rows, or a ready
    (PoolJobStruct array, count) pair."""
    n = len(subs) if n is None else n
    out = (_lib.JobVerdict * (n + 1))()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    r = result()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    if len(jobs) == 2 and isinstance(jobs[0], ctypes.Array):
        jarr, njobs = jobs
    else:
        jarr, _keep = _lib._jobs_array(jobs)
        njobs = len(jarr)
    ses = ref.session_array(sessions)
    rc = call(jarr if njobs else None, njobs, ses if len(ses) else None, len(ses), sub_array(subs) if n else None, n, out,
              ctypes.byref(r))
    return rc, out, r


def check(call, jobs, sessions, subs, want=None):
    """One call; every verdict and the counts against hashlib.  Returns the expectation."""
    want = verdicts(jobs, sessions, subs) if want is None else want
    rc, out, r = raw(call, jobs, sessions, subs)
    n = len(subs)
    assert rc == _lib.BM_OK
    assert ref.as_tuples(out, n) == want
    assert ref.result_tuple(r) == ref.counts(want)
    assert bytes(out[n]) == b"\xa5" * 40
    return want


# ---- the three jobs that differ in everything wave-uniform -------------------------------

@functools.lru_cache(maxsize=None)
def three_jobs():
    """(jobs, sessions).  Job 0: the field (4 + 4 bytes) at byte 10 of a 40-byte
    coinbase: one tail block, j0 2, boff 2, no branch.  Job 1: 8 + 8 bytes at byte
    122 of 150, crossing the block edge at 128: one whole block before, two tail
    blocks, j0 14, boff 2, one branch entry, an nbits that does not decode.  Job 2:
    1 + 1 bytes at byte 33 of 170: three tail blocks, j0 8, boff 1, three branch
    entries.  Three different windows; seven sessions of 8-byte extranonce1 under
    the grid's targets."""
    rng = random.Random(0x10b5)
    jobs = (PoolJob(ref.synthetic_job(rng, 10, 4, 4, 40, 0), 1000, 2000),
            PoolJob(ref.synthetic_job(rng, 122, 8, 8, 150, 1, nbits=UNDECODABLE_NBITS), 5, 7),
            PoolJob(ref.synthetic_job(rng, 33, 1, 1, 170, 3), 0x7fffffff, 0xfffffffe))
    sessions = tuple(ref.synthetic_sessions(rng, 8))
    return jobs, sessions


def job_subs(rng, jobs, nsessions, assign):
    """One submission per entry of `assign` (a job index each, possibly past the
    table): a random extranonce2 that fits its job, the ntimes of a job cycling
    through lo - 1, lo, hi and hi + 1 of its window, adjacent submissions under
    different sessions."""
    seen = {}
    out = []
    for i, j in enumerate(assign):
        if j < len(jobs):
            pj = jobs[j]
            k = seen[j] = seen.get(j, -1) + 1
            ntime = (pj.ntime_lo - 1, pj.ntime_lo, pj.ntime_hi, pj.ntime_hi + 1)[k % 4] & U32
            en2 = rng.getrandbits(8 * pj.job.extranonce2_size)
        else:
            ntime, en2 = rng.getrandbits(32), rng.getrandbits(8)
        out.append((en2, ntime, rng.getrandbits(32), rng.getrandbits(32), i % nsessions, j))
    return out


def layouts_differ():
    """The three jobs are what their docstring says, by the host's own arithmetic restated."""
    jobs, _ = three_jobs()
    shape = []
    for pj in jobs:
        j = pj.job
        pos, total = len(j.coinb1), len(j.coinb1) + len(j.extranonce1) + j.extranonce2_size + len(j.coinb2)
        pre = pos // 64
        nb = (total + 9 + 63) // 64 - pre
        shape.append((nb, (pos % 64) // 4, pos % 4, len(j.extranonce1), j.extranonce2_size, len(j.branch)))
    assert shape == [(1, 2, 2, 4, 4, 0), (2, 14, 2, 8, 8, 1), (3, 8, 1, 1, 1, 3)]
    assert ref.block_target(jobs[1].job.nbits) is None and ref.block_target(jobs[0].job.nbits) is not None


BATCH_SIZES = (1, 2, 63, 64, 65, 129, 200)
PER_JOB_COUNTS = ((0, 1, 64), (65, 0, 1), (64, 65, 0), (1, 64, 65), (65, 65, 65), (64, 64, 64))


def round_robin(call, n):
    """Jobs assigned round-robin: every 64-stride block of the batch mixes all three
    jobs, and every group ends mid-wave."""
    jobs, sessions = three_jobs()
    rng = random.Random(2000 + n)
    subs = job_subs(rng, jobs, len(sessions), [i % 3 for i in range(n)])
    want = check(call, jobs, sessions, subs)
    if n >= 63:
        # each job saw its window's four edges, flagged outside and clear inside
        for j in range(3):
            flags = [bool(st & ref.NTIME) for (_, st), s in zip(want, subs) if s[5] == j][:4]
            assert flags == [True, False, False, True], j
        assert not any(st & ref.BLOCK for (_, st), s in zip(want, subs) if s[5] == 1)  # nbits does not decode
        assert {0, 1} <= {st & ref.SHARE for _, st in want}


def per_job_counts(call, counts):
    """Per-job counts of exactly 0, 1, 64 and 65, in a shuffled order."""
    jobs, sessions = three_jobs()
    rng = random.Random(3000 + sum(c * 67 ** k for k, c in enumerate(counts)))
    assign = [j for j, c in enumerate(counts) for _ in range(c)]
    rng.shuffle(assign)
    check(call, jobs, sessions, job_subs(rng, jobs, len(sessions), assign))


def last_job_only(call):
    jobs, sessions = three_jobs()
    rng = random.Random(4000)
    check(call, jobs, sessions, job_subs(rng, jobs, len(sessions), [2] * 65))


def malformed_unused_job(call):
    """A job no submission names is refused all the same: BM_EINVAL, canaries intact."""
    jobs, sessions = three_jobs()
    rng = random.Random(5000)
    subs = job_subs(rng, jobs, len(sessions), [0, 2] * 10)
    for kw in (dict(extranonce2_size=9), dict(extranonce1_len=0), dict(nbranch=33), dict(coinb2_len=1 << 16)):
        jarr, _keep = _lib._jobs_array(jobs)
        for k, v in kw.items():
            setattr(jarr[1].job, k, v)
        rc, out, r = raw(call, (jarr, 3), sessions, subs)
        assert rc == _lib.BM_EINVAL, kw
        assert bytes(out) == b"\xa5" * (40 * 21) and bytes(r) == b"\x5a" * 40, kw
    check(call, jobs, sessions, subs)  # and the entry still answers


def unknown_jobs(call):
    """job == njobs and job == 2^32 - 1 at index 0, at n - 1 and mid-batch, among valid entries."""
    jobs, sessions = three_jobs()
    rng = random.Random(6000)
    n = 130
    assign = [i % 3 for i in range(n)]
    assign[0], assign[n - 1], assign[64], assign[65], assign[70] = 3, U32, U32, 3, 3
    subs = job_subs(rng, jobs, len(sessions), assign)
    want = check(call, jobs, sessions, subs)
    assert [i for i, w in enumerate(want) if w == INVALID_VERDICT] == [0, 64, 65, 70, n - 1]


def no_jobs_and_unknown_sessions(call):
    """njobs == 0 with n = 65 (jobs NULL): every entry INVALID.  And an unknown job
    combined with an unknown session, beside each of the two alone."""
    jobs, sessions = three_jobs()
    rng = random.Random(7000)
    subs = job_subs(rng, jobs, len(sessions), [i % 3 for i in range(65)])
    want = check(call, (), sessions, subs)
    assert want == [INVALID_VERDICT] * 65
    assert check(call, (), (), subs) == [INVALID_VERDICT] * 65
    ns = len(sessions)
    both = [(1, 2, 3, 4, ns, 3), (1, 2, 3, 4, U32, U32), (1, 2, 3, 4, ns, 0), (1, 2, 3, 4, 0, 3), (1, 2, 3, 4, 0, 0)]
    want = check(call, jobs, sessions, subs[:30] + both + subs[30:])
    assert [w == INVALID_VERDICT for w in want[30:35]] == [True, True, True, True, False]


def arrangement(call):
    """The same multiset of submissions in two orders: the same verdict per submission."""
    jobs, sessions = three_jobs()
    rng = random.Random(9000)
    subs = job_subs(rng, jobs, len(sessions), [rng.randrange(4) for _ in range(150)])
    a = check(call, jobs, sessions, subs)
    order = list(range(len(subs)))
    rng.shuffle(order)
    b = check(call, jobs, sessions, [subs[i] for i in order])
    assert b == [a[i] for i in order]
    c = check(call, jobs, sessions, sorted(subs, key=lambda s: -s[5]))
    assert sorted(c) == sorted(a)


@functools.lru_cache(maxsize=None)
def large_case():
    """(jobs, sessions, subs, verdicts): 5,000 submissions over 8 jobs of different
    layouts and 500 sessions, with above-target and INVALID entries of all three kinds."""
    rng = random.Random(0x8000)
    jobs = []
    for k in range(8):
        size1, size2 = rng.choice((2, 4, 8)), rng.choice((2, 4, 8))
        pos = rng.randrange(0, 200)
        total = pos + size1 + size2 + rng.randrange(1, 150)
        lo = rng.getrandbits(31)
        jobs.append(PoolJob(ref.synthetic_job(rng, pos, size1, size2, total, k % 5), lo, lo + (1 << 31)))
    sessions = [PoolSession(rng.randbytes(8), rng.choice((U256, U256, 1 << 255, 1 << 254, 0))) for _ in range(500)]
    subs = []
    for _ in range(5000):
        j = rng.randrange(8)
        en2 = rng.getrandbits(8 * jobs[j].job.extranonce2_size)
        p = rng.random()
        if p < 0.01:
            j = rng.randrange(8, 1 << 32)
        elif p < 0.02:
            en2 |= 1 << 8 * jobs[j].job.extranonce2_size if jobs[j].job.extranonce2_size < 8 else 0
        subs.append((en2, rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32),
                     rng.randrange(500, 1 << 32) if 0.02 <= p < 0.03 else rng.randrange(500), j))
    want = verdicts(jobs, sessions, subs)
    assert {0, 1, 4, 8, 9} <= {st for _, st in want} and any(st & ref.BLOCK for _, st in want)
    return tuple(jobs), tuple(sessions), tuple(subs), want


# ---- the share set ------------------------------------------------------------------------

class Model(ss.Model):
    """share_set_ref.Model with a step over several jobs: the same Python set."""

    def verify_jobs(self, jobs, sessions, subs):
        plain = verdicts(jobs, sessions, subs)
        new = {h for h, st in plain if ss.eligible(st)} - self.seen
        if len(self.seen) + len(new) > self.capacity:
            return None
        want, recorded = [], 0
        for h, st in plain:
            if ss.eligible(st):
                if h in self.seen:
                    st |= DUPLICATE
                else:
                    self.seen.add(h)
                    recorded += 1
            want.append((h, st))
        dups = sum(1 for _, st in want if st & DUPLICATE)
        return want, ref.counts(want) + (dups, recorded, len(self.seen))


def set_check(share_set, model, jobs, sessions, subs):
    """One bm_share_set_verify_jobs call on the set and on the model; everything
    against the model.  Returns the model's answer (None for a refusal)."""
    before = share_set.count
    want = model.verify_jobs(jobs, sessions, subs)
    f = share_set._lib.bm_share_set_verify_jobs
    rc, out, r = raw(lambda *a: f(share_set.handle, *a), jobs, sessions, subs, result=_lib.ShareSetResult)
    n = len(subs)
    if want is None:
        assert rc == _lib.BM_EFULL
        assert bytes(out) == b"\xa5" * (40 * (n + 1)) and bytes(r) == b"\x5a" * 64
        assert share_set.count == before == len(model.seen)
        return None
    assert rc == _lib.BM_OK
    assert ref.as_tuples(out, n) == want[0]
    assert ss.result_tuple(r) == want[1]
    assert bytes(out[n]) == b"\xa5" * 40
    assert share_set.count == len(model.seen) == r.count
    return want


def open_jobs(seed=0x5e7):
    """(jobs, sessions): three_jobs' layouts with decodable nbits or none, no
    windows, and sessions under which every hash is a share."""
    rng = random.Random(seed)
    jobs = (PoolJob(ref.synthetic_job(rng, 10, 4, 4, 40, 0)), PoolJob(ref.synthetic_job(rng, 122, 8, 8, 150, 1)),
            PoolJob(ref.synthetic_job(rng, 33, 1, 1, 170, 3)))
    return jobs, [PoolSession(rng.randbytes(8), U256) for _ in range(5)]


def set_across_batches(make_set):
    """One hash under job 0 in one batch and again in the next; the same tuple under
    two different jobs: two hashes, both recorded."""
    jobs, sessions = open_jobs()
    t = (0x0102, 5, 6, 7, 1)
    with make_set(64) as s:
        model = Model(64)
        want, r = set_check(s, model, jobs, sessions, [t + (0,), (9, 9, 9, 9, 0, 2)])
        assert r[5:] == (0, 2, 2)
        want, r = set_check(s, model, jobs, sessions, [(8, 8, 8, 8, 0, 1), t + (0,)])
        assert [st & DUPLICATE for _, st in want] == [0, DUPLICATE] and r[5:] == (1, 1, 3)
        u = (0x01, 5, 6, 7, 2)  # fits every job's extranonce2
        want, r = set_check(s, model, jobs, sessions, [u + (0,), u + (1,), u + (2,)])
        assert len({h for h, _ in want}) == 3 and r[5:] == (0, 3, 6)
        want, r = set_check(s, model, jobs, sessions, [u + (2,), u + (1,), u + (0,), u + (3,)])
        assert [st for _, st in want][:3] == [1 | DUPLICATE] * 3 and want[3] == INVALID_VERDICT and r[5:] == (3, 0, 6)


def set_identical_jobs(make_set):
    """Two jobs[] entries with identical content: identical hashes, so the second is a duplicate."""
    jobs, sessions = open_jobs()
    twin = (jobs[1], jobs[0], PoolJob(jobs[1].job))
    t = (0x0a0b0c0d, 5, 6, 7, 3)
    with make_set(16) as s:
        want, r = set_check(s, Model(16), twin, sessions, [t + (2,), t + (1,), t + (0,)])
        assert want[0][0] == want[2][0] != want[1][0]
        assert [st & DUPLICATE for _, st in want] == [0, 0, DUPLICATE] and r[5:] == (1, 2, 2)


def set_repeat_across_groups(make_set):
    """A repeat inside one batch whose two copies land in different job groups (two
    identical jobs[] entries, so the hash is one): the lower caller index wins,
    whichever group is staged first."""
    jobs, sessions = open_jobs()
    twin = (jobs[0], jobs[2], PoolJob(jobs[0].job))
    rng = random.Random(77)
    t = (0x01020304, 5, 6, 7, 0)
    for first, second in ((0, 2), (2, 0)):
        subs = [(rng.getrandbits(8), rng.getrandbits(32), 1, 2, i % 5, 1) for i in range(140)]
        subs[3], subs[100] = t + (first,), t + (second,)   # job group `second` may be staged before group `first`
        subs[70] = t + (first,)                             # and a repeat inside the group, a workgroup later
        with make_set(256) as s:
            want, r = set_check(s, Model(256), twin, sessions, subs)
        dup = [i for i, (_, st) in enumerate(want) if st & DUPLICATE and subs[i][:4] == t[:4]]
        assert dup == [70, 100] and not want[3][1] & DUPLICATE and want[3][0] == want[100][0]


def set_full(make_set):
    """BM_EFULL on capacity 8 with canaries, then a follow-up batch against the model that never saw the refused one."""
    jobs, sessions = open_jobs()
    rng = random.Random(88)

    def fresh(j):
        return (rng.getrandbits(8), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), rng.randrange(5), j)

    old = [fresh(i % 3) for i in range(5)]
    refused = [fresh(i % 3) for i in range(4)]
    with make_set(8) as s:
        model = Model(8)
        _, r = set_check(s, model, jobs, sessions, old)
        assert r[5:] == (0, 5, 5)
        assert set_check(s, model, jobs, sessions, [old[1]] + refused) is None
        assert set_check(s, model, jobs, sessions, [fresh(i % 3) for i in range(70)]) is None
        want, r = set_check(s, model, jobs, sessions, [old[0], refused[0], fresh(1), refused[0], old[4], refused[3]])
        assert [bool(st & DUPLICATE) for _, st in want] == [True, False, False, True, True, False] and r[5:] == (3, 3, 8)
        assert set_check(s, model, jobs, sessions, [fresh(2)]) is None


def set_alternating(make_set):
    """A set fed alternately by verify and verify_jobs: one key space."""
    jobs, sessions = open_jobs()
    job0, view0 = jobs[0].job, session_views(jobs, sessions)[0]
    rng = random.Random(99)
    a = [(rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), i % 5) for i in range(70)]
    with make_set(512) as s:
        model = Model(512)
        ss.check(s, model, job0, view0, a[:40])
        want, r = set_check(s, model, jobs, sessions, [x + (0,) for x in a[20:60]] + [(1, 2, 3, 4, 0, 1)])
        assert r[5:] == (20, 21, 61)
        want, r = ss.check(s, model, job0, view0, a)
        assert r[5:] == (60, 10, 71)
        want, r = set_check(s, model, jobs, sessions, [x + (0,) for x in a] + [(1, 2, 3, 4, 0, 1)])
        assert r[5:] == (71, 0, 71)
