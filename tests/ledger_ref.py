"""The ledger's reference and scenarios, shared by the CPU and the GPU tests of
bm_ledger_verify_jobs: hashlib verdicts (tests/jobs_verify_ref.verdicts), the Python
set of tests/share_set_ref.Model and a dict of rows.  The library is never its own
reference.  A scenario takes make_ledger(rows) -> Ledger and make_set(capacity) ->
ShareSet, so the same cases run on the CPU entries and on a device ledger; every
comparison is exact equality of every verdict, of the result struct and of every
row of the ledger read back (untouched rows included), with a canary verdict past n
and, on a refusal, canaries all over."""
import ctypes
import random

from distributed_bitcoin_minter_amd import PoolJob, PoolSession, _lib
import jobs_verify_ref as jref
import pool_verify_ref as ref
from pool_verify_ref import U32, U256
from verify_ref import INVALID_VERDICT, U64

SHARE, BLOCK, INVALID, NTIME, DUPLICATE = ref.SHARE, ref.BLOCK, ref.INVALID, ref.NTIME, jref.DUPLICATE
ACCEPTED, BLOCKS, ABOVE, NTIME_W, DUPLICATES, INVALID_W, WORK, BEST = range(8)
EMPTY = (0,) * 7 + (U64,)
PEELS = (0, 1, 4, 64)
WIDE_NBITS = 0x2100ffff  # the block target 0xffff << 240: nearly every hash is a block


def classify(status):
    """The row word a submission of a known session counts in: the first rule that applies."""
    if status & INVALID:
        return INVALID_W
    if status & NTIME:
        return NTIME_W
    if status & DUPLICATE:
        return DUPLICATES
    if status & (SHARE | BLOCK):
        return ACCEPTED
    return ABOVE


class Model:
    """The specification, restated: a dict of rows, and share_set_ref's Python set
    when the ledger is fed through a share set."""

    def __init__(self, rows, capacity=None):
        self.nrows, self.rows = rows, {}
        self.set = jref.Model(capacity) if capacity else None

    def verify(self, jobs, sessions, subs, accounts=None, weights=None):
        """([(hash, status)], the eleven result fields), or None where the call must
        return BM_EFULL (the model is unchanged then)."""
        if self.set is not None:
            answer = self.set.verify_jobs(jobs, sessions, subs)
            if answer is None:
                return None
            want, counts = answer
        else:
            want = jref.verdicts(jobs, sessions, subs)
            counts = ref.counts(want) + (0, 0, 0)
        credited = unattributed = work = 0
        for sub, (h, st) in zip(subs, want):
            s = sub[4]
            if s >= len(sessions):
                unattributed += 1
                continue
            row = self.rows.setdefault(accounts[s] if accounts is not None else s, list(EMPTY))
            cls = classify(st)
            row[cls] += 1
            if cls == ACCEPTED:
                w = weights[s] if weights is not None else 1
                row[BLOCKS] += 1 if st & BLOCK else 0
                row[WORK] = (row[WORK] + w) & U64
                row[BEST] = min(row[BEST], h >> 192)
                credited += 1
                work = (work + w) & U64
        return want, counts + (credited, unattributed, work)

    def table(self):
        return [tuple(self.rows.get(i, EMPTY)) for i in range(self.nrows)]

    def drain(self, first, count):
        out = self.table()[first:first + count]
        for i in range(first, first + count):
            self.rows.pop(i, None)
        return out

    def classes(self):
        """Submissions counted in the rows, over all rows."""
        return sum(sum(r[k] for k in (ACCEPTED, ABOVE, NTIME_W, DUPLICATES, INVALID_W)) for r in self.rows.values())


def result_tuple(r):
    return tuple(getattr(r, f) for f, _ in _lib.LedgerResult._fields_)


def table(ledger):
    return [row.as_tuple() for row in ledger.read()]


def raw(ledger, share_set, jobs, sessions, subs, accounts=None, weights=None):
    """One call through the C ABI into canary-filled arrays -> (status, verdicts, result)."""
    nses = len(sessions)
    acc = (ctypes.c_uint32 * max(nses, 1))(*accounts) if accounts is not None else None
    wgt = (ctypes.c_uint64 * max(nses, 1))(*weights) if weights is not None else None
    f = ledger._lib.bm_ledger_verify_jobs
    sh = share_set.handle if share_set is not None else None
    return jref.raw(lambda *a: f(ledger.handle, sh, *a[:4], acc, wgt, *a[4:]), jobs, sessions, subs,
                    result=_lib.LedgerResult)


def check(ledger, model, jobs, sessions, subs, share_set=None, accounts=None, weights=None):
    """One call on the ledger and on the model; everything against the model,
    every row included.  Returns the model's answer (None for BM_EFULL)."""
    assert (share_set is None) == (model.set is None)
    before, count = table(ledger), share_set.count if share_set is not None else 0
    want = model.verify(jobs, sessions, subs, accounts, weights)
    rc, out, r = raw(ledger, share_set, jobs, sessions, subs, accounts, weights)
    n = len(subs)
    if want is None:
        assert rc == _lib.BM_EFULL
        assert bytes(out) == b"\xa5" * (40 * (n + 1)) and bytes(r) == b"\x5a" * 88
        assert table(ledger) == before == model.table() and share_set.count == count
        return None
    assert rc == _lib.BM_OK
    assert ref.as_tuples(out, n) == want[0]
    assert result_tuple(r) == want[1]
    assert bytes(out[n]) == b"\xa5" * 40
    assert table(ledger) == model.table()
    if share_set is not None:
        assert share_set.count == len(model.set.seen) == r.count
    return want


def refused(ledger, model, call, status=None):
    """call() -> (status, verdicts, result) must be refused with canaries intact and
    the ledger as the model has it."""
    rc, out, r = call()
    assert rc == (_lib.BM_EINVAL if status is None else status)
    assert bytes(out) == b"\xa5" * len(bytes(out)) and bytes(r) == b"\x5a" * 88
    assert table(ledger) == model.table()


def open_job(rng, nbits=ref.GRID_NBITS, lo=0, hi=U32):
    return PoolJob(ref.synthetic_job(rng, 45, 8, 4, 120, 1, nbits=nbits), lo, hi)


def open_sessions(rng, n):
    return [PoolSession(rng.randbytes(8), U256) for _ in range(n)]


def sub(rng, session, job=0):
    return (rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), session, job)


def pair(make_ledger, make_set, rows, capacity, peel=None):
    """[(ledger, model, set or None)]: one ledger fed through a set and one without."""
    out = []
    for with_set in (True, False):
        ledger = make_ledger(rows)
        if peel is not None:
            ledger.set_peel(peel)
        out.append((ledger, Model(rows, capacity if with_set else None), make_set(capacity) if with_set else None))
    return out


def close(triples):
    for ledger, _, share_set in triples:
        ledger.close()
        if share_set is not None:
            share_set.close()


# ---- scenarios ---------------------------------------------------------------------------

def batch_sizes(make_ledger, make_set, n):
    """n submissions round-robin over three jobs and seven sessions on four rows:
    the last wave of every job group is partial."""
    jobs, sessions = jref.three_jobs()
    rng = random.Random(100 + n)
    subs = jref.job_subs(rng, jobs, len(sessions), [i % 3 for i in range(n)])
    accounts = [0, 1, 2, 0, 1, 2, 3]
    weights = [rng.getrandbits(64) for _ in sessions]
    triples = pair(make_ledger, make_set, 4, 256)
    try:
        for ledger, model, share_set in triples:
            want, r = check(ledger, model, jobs, sessions, subs, share_set, accounts, weights)
            assert r[0] == n == model.classes() and r[9] == 0
    finally:
        close(triples)


def wave_shapes(make_ledger, make_set, peel):
    """One job, so lane k of the credit kernel is submission k.  Open targets: every
    hash is accepted and `best` is a real 64-bit min; random 64-bit weights, so
    `work` wraps.  The shapes accumulate in one ledger."""
    rng = random.Random(200)
    jobs = (open_job(rng),)
    sessions = open_sessions(rng, 70)
    weights = [rng.getrandbits(64) for _ in sessions]
    strays = [7] * 64
    strays[5], strays[20], strays[40], strays[63] = 1, 2, 3, 4
    shapes = [[3] * 64,                       # all 64 lanes of a wave on one row
              [i % 2 for i in range(64)],     # two rows alternating by lane
              list(range(64)),                # 64 distinct rows in one wave
              [10 + i % 5 for i in range(64)],  # exactly five rows: at peel 4 the fifth takes the per-lane path
              strays,                         # one row on 60 lanes and four strays
              [9] * 150,                      # one row across three workgroups
              [i % 69 for i in range(200)]]   # and rows that recur in later waves
    triples = pair(make_ledger, make_set, 70, 1024, peel)
    try:
        for ledger, model, share_set in triples:
            for shape in shapes:
                subs = [sub(rng, s) for s in shape]
                want, r = check(ledger, model, jobs, sessions, subs, share_set, None, weights)
                assert r[8] == len(shape) and all(st & SHARE for _, st in want)
            assert model.rows[9][ACCEPTED] >= 150 and len({row[BEST] for row in model.rows.values()}) > 60
    finally:
        close(triples)


def row_mapping(make_ledger, make_set):
    rng = random.Random(300)
    jobs = (open_job(rng),)
    sessions = open_sessions(rng, 6)
    triples = pair(make_ledger, make_set, 9, 256)
    try:
        for ledger, model, share_set in triples:
            # two sessions on one row, weights 3 and 2^40, interleaved in one wave: a per-submission sum
            accounts, weights = [4, 4, 0, 8, 1, 1], [3, 1 << 40, 7, 11, (1 << 63), (1 << 63) + 5]
            subs = [sub(rng, i % 2) for i in range(41)]
            check(ledger, model, jobs, sessions, subs, share_set, accounts, weights)
            assert model.rows[4][WORK] == 21 * 3 + 20 * (1 << 40)
            # weights 2^63 and 2^63 + 5 on one row: work wraps to 5; a session on the highest row
            want, r = check(ledger, model, jobs, sessions, [sub(rng, 4), sub(rng, 5), sub(rng, 3)], share_set, accounts,
                            weights)
            assert model.rows[1][WORK] == 5 and model.rows[8][ACCEPTED] == 1 and r[10] == 5 + 11
            # accounts NULL: the identity; weights NULL: one each
            before = model.rows[4][ACCEPTED]
            want, r = check(ledger, model, jobs, sessions, [sub(rng, 5 - i % 6) for i in range(70)], share_set)
            assert r[10] == 70 and model.rows[4][ACCEPTED] == before + 12 and model.rows[5][ACCEPTED] == 12
    finally:
        close(triples)
    # rows == 1: every session on row 0
    triples = pair(make_ledger, make_set, 1, 256)
    try:
        for ledger, model, share_set in triples:
            check(ledger, model, jobs, sessions, [sub(rng, i % 6) for i in range(67)], share_set, [0] * 6, [2] * 6)
            assert model.table() == [(67, model.rows[0][BLOCKS], 0, 0, 0, 0, 134, model.rows[0][BEST])]
            check(ledger, model, jobs, sessions[:1], [sub(rng, 0)], share_set)
    finally:
        close(triples)


def every_class(make_ledger, make_set):
    """One row receives every class in one wave; a second row only sees its own."""
    rng = random.Random(400)
    jobs = (open_job(rng, WIDE_NBITS), open_job(rng, ref.GRID_NBITS, 1000, 2000))
    en1 = rng.randbytes(8)
    sessions = [PoolSession(en1, U256), PoolSession(en1, 0), PoolSession(rng.randbytes(8), U256)]
    accounts, weights = [1, 1, 0], [5, 9, 1]
    earlier = (77, 1500, 1, 2, 0, 1)
    inside = (3, 1500, 4, 5, 0, 1)
    batch = [(1, 1, 1, 1, 0, 0),        # job 0, open target: SHARE | BLOCK
             (2, 1, 1, 1, 1, 0),        # job 0, target 0: BLOCK without SHARE
             (3, 1500, 1, 1, 1, 1),     # job 1, target 0: above target
             (4, 2001, 1, 1, 1, 1),     # NTIME alone
             (5, 999, 1, 1, 0, 1),      # NTIME with SHARE
             inside, inside,            # a duplicate from this batch (with a set)
             earlier,                   # a duplicate from an earlier call (with a set)
             (1 << 32, 1500, 1, 1, 0, 1),  # INVALID by extranonce2
             (6, 1500, 1, 1, 0, 2),     # INVALID by unknown job
             (7, 1500, 1, 1, 2, 1)]     # the other row: accepted
    triples = pair(make_ledger, make_set, 2, 64)
    try:
        for ledger, model, share_set in triples:
            check(ledger, model, jobs, sessions, [earlier], share_set, accounts, weights)
            want, r = check(ledger, model, jobs, sessions, batch * 5, share_set, accounts, weights)
            statuses = {st for _, st in want}
            assert {SHARE | BLOCK, BLOCK, 0, NTIME, NTIME | SHARE, INVALID} <= statuses
            row = model.rows[1]
            assert row[INVALID_W] == 10 and row[NTIME_W] == 10 and row[ABOVE] == 5 and row[BLOCKS] >= 2
            if share_set is not None:
                assert SHARE | DUPLICATE in statuses and row[DUPLICATES] == 9 + 5 + 4 + 4
            assert all(row[k] for k in (ACCEPTED, BLOCKS, ABOVE, NTIME_W, INVALID_W, WORK))
            assert model.rows[0][ACCEPTED] + model.rows[0][DUPLICATES] == 5
    finally:
        close(triples)


def unknown_sessions(make_ledger, make_set):
    """Unknown-session lanes first, last and in the middle of a wave: they touch no
    row, lead no round and count in `unattributed`; so does an unknown job with an
    unknown session, while an unknown job with a known session is that row's INVALID."""
    rng = random.Random(500)
    jobs = (open_job(rng),)
    sessions = open_sessions(rng, 3)
    subs = [sub(rng, i % 3) for i in range(130)]
    for i, s in ((0, 3), (31, U32), (63, 3), (64, 1 << 20), (100, 3), (129, U32)):
        subs[i] = subs[i][:4] + (s, 0)
    subs[70] = subs[70][:4] + (3, 1)    # unknown job, unknown session
    subs[71] = subs[71][:4] + (2, 1)    # unknown job, known session
    triples = pair(make_ledger, make_set, 3, 256)
    try:
        for ledger, model, share_set in triples:
            want, r = check(ledger, model, jobs, sessions, subs, share_set, [2, 1, 0], [1, 2, 3])
            assert r[9] == 7 and r[3] == 8 and model.classes() == 123 and model.rows[0][INVALID_W] == 1
            want, r = check(ledger, model, jobs, sessions, [s[:4] + (5, 0) for s in subs[:65]], share_set, [2, 1, 0])
            assert r[9] == 65 and r[8] == 0 and want == [INVALID_VERDICT] * 65
            want, r = check(ledger, model, jobs, (), subs[:3], share_set)  # no sessions at all
            assert r[9] == 3
    finally:
        close(triples)


def best_job():
    rng = random.Random(600)
    en1 = rng.randbytes(8)
    return (open_job(rng, jref.UNDECODABLE_NBITS),), [PoolSession(en1, U256), PoolSession(en1, 0), PoolSession(en1, U256)]


# Two submissions of best_job whose hashes agree in bytes 0..3 and differ in bytes 4..7 (found once by a
# birthday search over the nonce; the scenario asserts the property)
BEST_PAIR = ((1, 2, 50412, 3, 0, 0), (1, 2, 72446, 3, 0, 0))


def best(make_ledger, make_set):
    jobs, sessions = best_job()
    a, b = BEST_PAIR
    ha, hb = (h for h, _ in jref.verdicts(jobs, sessions, [a, b]))
    assert ha >> 224 == hb >> 224 and (ha >> 192) != (hb >> 192)
    lo, hi = (a, b) if ha < hb else (b, a)
    rng = random.Random(601)
    pool = sorted((sub(rng, 0) for _ in range(40)), key=lambda s: jref.verdicts(jobs, sessions, [s])[0][0])
    accounts = [0, 0, 1]
    triples = pair(make_ledger, make_set, 2, 256)
    try:
        for ledger, model, share_set in triples:
            # the two hashes that differ in bytes 4..7 only, the higher one first and in another lane
            check(ledger, model, jobs, sessions, [hi, lo], share_set, accounts)
            assert model.rows[0][BEST] == min(ha, hb) >> 192
            ledger.clear()
            model.rows.clear()
            check(ledger, model, jobs, sessions, pool[10:20], share_set, accounts)
            low = model.rows[0][BEST]
            # a later call with higher hashes leaves best
            check(ledger, model, jobs, sessions, pool[20:], share_set, accounts)
            assert model.rows[0][BEST] == low
            # a lower hash that is rejected (above target: session 1 has target 0) leaves best
            check(ledger, model, jobs, sessions, [pool[0][:4] + (1, 0)], share_set, accounts)
            assert model.rows[0][BEST] == low and model.rows[0][ABOVE] == 1
            # row 1 takes a low hash; with a set the same hash again on row 0 is a duplicate and leaves row 0's best
            check(ledger, model, jobs, sessions, [pool[1][:4] + (2, 0)], share_set, accounts)
            want, _ = check(ledger, model, jobs, sessions, [pool[1][:4] + (0, 0)], share_set, accounts)
            if share_set is not None:
                assert want[0][1] & DUPLICATE and model.rows[0][BEST] == low
            assert model.rows[1][BEST] < low
    finally:
        close(triples)


def accumulation(make_ledger, make_set, witness=None):
    """Three calls of 5,000 submissions (jobs_verify_ref.large_case: 8 jobs, 500
    sessions) on 37 accounts, in three orders, with a set and without one.
    witness(rows): a second ledger whose bytes must agree, fed through a CPU set."""
    jobs, sessions, subs, _ = jref.large_case()
    rng = random.Random(700)
    accounts = [s % 37 for s in range(500)]
    weights = [rng.getrandbits(64) for _ in range(500)]
    orders = [list(subs), list(subs[::-1]), sorted(subs)]
    from distributed_bitcoin_minter_amd import ShareSet
    triples = pair(make_ledger, make_set, 37, 1 << 14)
    try:
        for ledger, model, share_set in triples:
            other = witness(37) if witness else None
            other_set = ShareSet.cpu(1 << 14) if witness and share_set is not None else None
            try:
                unattributed = 0
                for batch in orders:
                    want, r = check(ledger, model, jobs, sessions, batch, share_set, accounts, weights)
                    unattributed += r[9]
                    if other is not None:
                        rc, v, wr = raw(other, other_set, jobs, sessions, batch, accounts, weights)
                        assert rc == _lib.BM_OK and ref.as_tuples(v, 5000) == want and result_tuple(wr) == r
                        assert table(other) == table(ledger)
                assert model.classes() + unattributed == 15000 and unattributed > 50
                assert all(model.rows[k][ACCEPTED] for k in range(37))
                if share_set is not None:
                    assert sum(row[DUPLICATES] for row in model.rows.values()) > 2000
            finally:
                if other is not None:
                    other.close()
                if other_set is not None:
                    other_set.close()
    finally:
        close(triples)


def drain_and_clear(make_ledger, make_set, between=None):
    """drain of a middle range returns what read returned, empties exactly that
    range and leaves its neighbours; clear empties all; two ledgers are
    independent.  between(): other calls on the ledger's context."""
    rng = random.Random(800)
    jobs = (open_job(rng),)
    sessions = open_sessions(rng, 10)
    with make_ledger(10) as a, make_ledger(4) as b:
        ma, mb = Model(10), Model(4)
        assert a.rows == 10 and b.rows == 4 and table(a) == [EMPTY] * 10
        check(a, ma, jobs, sessions, [sub(rng, i % 10) for i in range(90)], None, None, list(range(1, 11)))
        if between:
            between()
        check(b, mb, jobs, sessions, [sub(rng, i % 10) for i in range(50)], None, [i % 4 for i in range(10)])
        assert table(a) == ma.table()
        assert [r.as_tuple() for r in a.read(3, 4)] == ma.table()[3:7]
        assert [r.as_tuple() for r in a.drain(3, 4)] == ma.drain(3, 4)
        assert table(a) == ma.table() and table(a)[3:7] == [EMPTY] * 4 and EMPTY not in table(a)[:3] + table(a)[7:]
        assert len(a.drain(10, 0)) == 0 and len(a.read(0, 0)) == 0 and table(a) == ma.table()
        check(a, ma, jobs, sessions, [sub(rng, i % 10) for i in range(30)])
        if between:
            between()
        a.clear()
        ma.rows.clear()
        assert table(a) == [EMPTY] * 10 and table(b) == mb.table() != [EMPTY] * 4
        check(a, ma, jobs, sessions, [sub(rng, 9)])
        assert [r.as_tuple() for r in b.drain()] == mb.drain(0, 4) and table(b) == [EMPTY] * 4


def refusals(make_ledger, make_set, foreign_set=None):
    """Every refusal leaves the ledger byte-identical and the caller's arrays alone."""
    jobs, sessions = jref.open_jobs()
    rng = random.Random(900)

    def fresh(j, s=None):
        return (rng.getrandbits(8), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32),
                rng.randrange(5) if s is None else s, j)

    accounts = [0, 1, 2, 1, 0]
    with make_ledger(3) as ledger, make_set(8) as small:
        model = Model(3, 8)
        check(ledger, model, jobs, sessions, [fresh(i % 3) for i in range(5)], small, accounts, [1, 2, 3, 4, 5])
        # BM_EFULL from the capacity-8 set: the ledger and the set's count are unchanged
        assert check(ledger, model, jobs, sessions, [fresh(i % 3) for i in range(4)], small, accounts) is None
        assert check(ledger, model, jobs, sessions, [fresh(i % 3) for i in range(70)], small, accounts) is None
        one = [fresh(0)]
        # an account equal to rows (the last session's: every session is checked); identity with nsessions > rows
        refused(ledger, model, lambda: raw(ledger, small, jobs, sessions, one, [0, 1, 2, 1, 3]))
        refused(ledger, model, lambda: raw(ledger, None, jobs, sessions, one, [0, 1, 2, 1, U32]))
        refused(ledger, model, lambda: raw(ledger, small, jobs, sessions, one))
        refused(ledger, model, lambda: raw(ledger, None, jobs, sessions, one))
        # a malformed job that no submission names
        bad, _keep = _lib._jobs_array(jobs)
        bad[1].job.nbranch = 33
        refused(ledger, model, lambda: raw(ledger, small, (bad, 3), sessions, one, accounts))
        refused(ledger, model, lambda: raw(ledger, None, (bad, 3), sessions, one, accounts))
        # a set of the other kind
        if foreign_set is not None:
            with foreign_set(8) as other:
                refused(ledger, model, lambda: raw(ledger, other, jobs, sessions, one, accounts))
                assert other.count == 0
        # a NULL ledger, a NULL result
        f = ledger._lib.bm_ledger_verify_jobs
        r = _lib.LedgerResult()
        assert f(None, None, None, 0, None, 0, None, None, None, 0, None, ctypes.byref(r)) == _lib.BM_EINVAL
        assert f(ledger.handle, None, None, 0, None, 0, None, None, None, 0, None, None) == _lib.BM_EINVAL
        # a range past the end in read and drain; rounds = 65
        rows = (_lib.LedgerRow * 4)()
        ctypes.memset(rows, 0xA5, ctypes.sizeof(rows))
        lib = ledger._lib
        for first, count in ((0, 4), (3, 1), (4, 0), (2, 2), (U64, 2)):
            assert lib.bm_ledger_read(ledger.handle, first, count, rows) == _lib.BM_EINVAL, (first, count)
            assert lib.bm_ledger_drain(ledger.handle, first, count, rows) == _lib.BM_EINVAL, (first, count)
        assert lib.bm_ledger_read(ledger.handle, 0, 1, None) == _lib.BM_EINVAL
        assert bytes(rows) == b"\xa5" * 256
        assert lib.bm_ledger_set_peel(ledger.handle, 65) == _lib.BM_EINVAL
        assert lib.bm_ledger_set_peel(ledger.handle, 64) == _lib.BM_OK
        assert lib.bm_ledger_rows(ledger.handle, None) == _lib.BM_EINVAL
        assert table(ledger) == model.table() and small.count == 5
        # an empty batch is legal and changes nothing; and the ledger still answers
        rc, out, r = raw(ledger, small, jobs, sessions, [], accounts)
        assert rc == _lib.BM_OK and result_tuple(r) == (0,) * 7 + (5, 0, 0, 0) and table(ledger) == model.table()
        rc, out, r = raw(ledger, None, jobs, sessions, [], accounts)
        assert rc == _lib.BM_OK and result_tuple(r) == (0,) * 11
        want, r = check(ledger, model, jobs, sessions, [fresh(1), fresh(2), fresh(0)], small, accounts)
        assert r[6:9] == (3, 8, 3)


def creation():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.bm_ledger_create_cpu(0, ctypes.byref(h)) == _lib.BM_EINVAL
    assert lib.bm_ledger_create_cpu(_lib.BM_MAX_LEDGER_ROWS + 1, ctypes.byref(h)) == _lib.BM_EINVAL
    assert lib.bm_ledger_create_cpu(1, None) == _lib.BM_EINVAL and h.value is None
    lib.bm_ledger_destroy(None)
    assert lib.bm_ledger_clear(None) == _lib.BM_EINVAL


def agreement(make_ledger, make_set):
    """`verdicts` and the first eight result fields equal bm_share_set_verify_jobs's on
    a second, identical set."""
    jobs, sessions, subs, _ = jref.large_case()
    batches = [list(subs[:700]), list(subs[400:1100]), list(subs[:300]) * 2]
    with make_ledger(500) as ledger, make_set(4096) as a, make_set(4096) as b:
        f = b._lib.bm_share_set_verify_jobs
        for batch in batches:
            rc, out, r = raw(ledger, a, jobs, sessions, batch)
            rc2, out2, r2 = jref.raw(lambda *args: f(b.handle, *args), jobs, sessions, batch, result=_lib.ShareSetResult)
            assert rc == rc2 == _lib.BM_OK and bytes(out) == bytes(out2) and bytes(r)[:64] == bytes(r2)
            assert a.count == b.count
        assert r.duplicates >= 300
