"""The share set's reference and scenarios, shared by the CPU and the GPU tests of
bm_share_set_verify: hashlib (tests/pool_verify_ref.py's `verdict`) plus a Python
`set` of hashes, processed one submission at a time.  The library is never its own
reference.  A scenario takes make_set(capacity) -> ShareSet, so the same cases run
on a device set and on a CPU set; every comparison is exact equality of every
verdict's (hash, status, reserved) and of the result struct, with a canary verdict
past n and, on a refusal, canaries all over."""
import ctypes
import random

from distributed_bitcoin_minter_amd import PoolSession, _lib
import pool_verify_ref as ref
from pool_verify_ref import U32, U256

DUPLICATE = 16
SHARE, BLOCK, INVALID, NTIME = ref.SHARE, ref.BLOCK, ref.INVALID, ref.NTIME


def eligible(status):
    return bool(status & (SHARE | BLOCK)) and not status & INVALID


def home_slot(h, capacity):
    """The documented home slot of hash h (an int) in a device set of that capacity."""
    slots = 16
    while slots < 2 * capacity:
        slots *= 2
    return (h & U32) % slots


class Model:
    """The specification, restated: a Python set of hashes."""

    def __init__(self, capacity):
        self.capacity, self.seen = capacity, set()

    def verify(self, job, sessions, subs, lo=0, hi=U32):
        """([(hash, status)], result tuple), or None where the call must return
        BM_EFULL (the model is unchanged then)."""
        plain = [ref.verdict(job, sessions, s, lo, hi) for s in subs]
        new = {h for h, st in plain if eligible(st)} - self.seen
        if len(self.seen) + len(new) > self.capacity:
            return None
        want, recorded = [], 0
        for h, st in plain:
            if eligible(st):
                if h in self.seen:
                    st |= DUPLICATE
                else:
                    self.seen.add(h)
                    recorded += 1
            want.append((h, st))
        dups = sum(1 for _, st in want if st & DUPLICATE)
        return want, ref.counts(want) + (dups, recorded, len(self.seen))


def result_tuple(r):
    return r.n, r.shares, r.blocks, r.invalid, r.ntime, r.duplicates, r.recorded, r.count


def raw_verify(share_set, job, sessions, subs, lo=0, hi=U32):
    """One call through the C ABI into canary-filled arrays, one verdict longer
    than the batch -> (status, verdicts, result)."""
    n = len(subs)
    verdicts = (_lib.JobVerdict * (n + 1))()
    ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
    r = _lib.ShareSetResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    ses = ref.session_array(sessions)
    rc = share_set._lib.bm_share_set_verify(share_set.handle, ctypes.byref(job.struct), ses if len(ses) else None,
                                            len(ses), ref.sub_array(subs) if n else None, n, lo, hi, verdicts,
                                            ctypes.byref(r))
    return rc, verdicts, r


def check(share_set, model, job, sessions, subs, lo=0, hi=U32):
    """One call on the set and on the model; everything against the model.  Returns
    the model's answer (None for a refusal)."""
    before = share_set.count
    want = model.verify(job, sessions, subs, lo, hi)
    rc, verdicts, r = raw_verify(share_set, job, sessions, subs, lo, hi)
    n = len(subs)
    if want is None:
        assert rc == _lib.BM_EFULL
        assert bytes(verdicts) == b"\xa5" * (40 * (n + 1)) and bytes(r) == b"\x5a" * 64
        assert share_set.count == before == len(model.seen)
        return None
    assert rc == _lib.BM_OK
    assert ref.as_tuples(verdicts, n) == want[0]
    assert result_tuple(r) == want[1]
    assert bytes(verdicts[n]) == b"\xa5" * 40
    assert share_set.count == len(model.seen) == r.count and share_set.capacity == model.capacity
    return want


def open_sessions(rng, size1, n=7):
    """n sessions under which every hash is a share."""
    return [PoolSession(rng.randbytes(size1), U256) for _ in range(n)]


def fresh_sub(rng, size2, nsessions):
    return (rng.getrandbits(8 * size2), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32),
            rng.randrange(nsessions))


# ---- scenarios ---------------------------------------------------------------------------

def batch_edges(make_set, n):
    """n submissions, about a third of which repeat an earlier one: exactly the
    first occurrence is unflagged."""
    rng = random.Random(1000 + n)
    job = ref.synthetic_job(rng, 61, 8, 8, 130, 2)
    sessions = open_sessions(rng, 8)
    subs = []
    for i in range(n):
        subs.append(subs[rng.randrange(i)] if i and rng.random() < 1 / 3 else fresh_sub(rng, 8, 7))
    with make_set(256) as s:
        want, result = check(s, Model(256), job, sessions, subs)
    assert [bool(st & DUPLICATE) for _, st in want] == [sub in subs[:i] for i, sub in enumerate(subs)]
    assert result[6] == len(set(subs)) and result[5] == n - len(set(subs))
    if n > 60:
        assert result[5] > n // 6


def contention(make_set):
    """One submission in all 64 lanes of the first workgroup and in lanes of the
    second and third, among distinct others; then the same batch again."""
    rng = random.Random(2000)
    job = ref.synthetic_job(rng, 45, 4, 4, 250, 1)
    sessions = open_sessions(rng, 4)
    hot = fresh_sub(rng, 4, 7)
    subs = [fresh_sub(rng, 4, 7) for _ in range(192)]
    copies = list(range(64)) + [64, 69, 127, 129, 145, 190]
    for i in copies:
        subs[i] = hot
    with make_set(512) as s:
        model = Model(512)
        want, result = check(s, model, job, sessions, subs)
        assert [i for i, (_, st) in enumerate(want) if st & DUPLICATE] == copies[1:]
        assert result[5:] == (len(copies) - 1, 192 - len(copies) + 1, 192 - len(copies) + 1)
        again, result2 = check(s, model, job, sessions, subs)
        assert all(st & DUPLICATE for _, st in again)
        assert result2[5:] == (192, 0, result[7])


def forced_collisions(make_set):
    """Capacity 8, 16 slots: hashes whose home slots are 14, 15, 15, 15 and 0, so the
    probe chain wraps past the table's end; then queried in another order, mixed
    with new hashes of the same home slots."""
    rng = random.Random(3000)
    job = ref.synthetic_job(rng, 45, 4, 4, 120, 0)
    sessions = open_sessions(rng, 4, 3)
    by_home = {}
    for _ in range(300):
        sub = fresh_sub(rng, 4, 3)
        by_home.setdefault(home_slot(ref.verdict(job, sessions, sub)[0], 8), []).append(sub)
    assert len(by_home[15]) >= 4 and len(by_home[14]) >= 2 and len(by_home[0]) >= 2
    first = [by_home[14][0], by_home[15][0], by_home[15][1], by_home[15][2], by_home[0][0]]
    second = [first[4], by_home[15][3], first[2], by_home[14][1], first[0], first[3], by_home[0][1], first[1]]
    with make_set(8) as s:
        model = Model(8)
        _, r1 = check(s, model, job, sessions, first)
        assert r1[5:] == (0, 5, 5)
        want, r2 = check(s, model, job, sessions, second)
        assert [bool(st & DUPLICATE) for _, st in want] == [True, False, True, False, True, True, False, True]
        assert r2[5:] == (5, 3, 8)
        want, r3 = check(s, model, job, sessions, second[::-1] + first)  # a full table: every probe still ends
        assert all(st & DUPLICATE for _, st in want) and r3[5:] == (13, 0, 8)


def capacity_edges(make_set):
    """Capacity 8 holding 5: three new hashes fit, four do not, and neither do 65
    (which exhaust the probes of a 16-slot table).  A refusal leaves canaries, the
    count and every later answer as if it never happened."""
    rng = random.Random(4000)
    job = ref.synthetic_job(rng, 45, 4, 4, 120, 1)
    sessions = open_sessions(rng, 4, 3)
    old = [fresh_sub(rng, 4, 3) for _ in range(5)]
    new = [fresh_sub(rng, 4, 3) for _ in range(80)]

    def holding_five():
        s, model = make_set(8), Model(8)
        _, r = check(s, model, job, sessions, old)
        assert r[5:] == (0, 5, 5)
        return s, model

    # three new distinct hashes plus repeats: the set is full to the brim; then one more does not fit
    s, model = holding_five()
    with s:
        _, r = check(s, model, job, sessions, [new[0], old[1], new[1], new[0], old[4], new[2], new[1]])
        assert r[5:] == (4, 3, 8)
        assert check(s, model, job, sessions, [old[0], new[3]]) is None
        _, r = check(s, model, job, sessions, old + new[:3])
        assert r[5:] == (8, 0, 8)
    # four new, and 65 new: refused; the follow-up holds old hashes, hashes of the refused batch and new ones
    for refused in ([new[0], old[2], new[1], new[2], new[0], new[3]], new[10:75]):
        s, model = holding_five()
        with s:
            assert check(s, model, job, sessions, refused) is None
            want, r = check(s, model, job, sessions, [old[0], refused[0], new[79], old[3], refused[0], refused[-1]])
            assert [bool(st & DUPLICATE) for _, st in want] == [True, False, False, True, True, False]
            assert r[5:] == (3, 3, 8)
            assert check(s, model, job, sessions, refused) is None  # and the set still answers after it
            _, r = check(s, model, job, sessions, old)
            assert r[5:] == (5, 0, 8)


def across_calls(make_set, witness=None):
    """Capacity 2^16, three batches of 5,000 over 500 sessions: about 30 % repeat
    inside the batch and about 30 % repeat earlier batches; per-session targets put
    a part above target (ineligible: never flagged, however often they repeat);
    INVALID entries; an ntime window that leaves a part outside (eligible all the
    same).  witness(capacity): a second set whose bytes must agree."""
    rng = random.Random(5000)
    job = ref.synthetic_job(rng, 57, 5, 3, 300, 2)
    sessions = [PoolSession(rng.randbytes(5), rng.choice((U256, U256, 1 << 255, 1 << 254, 0))) for _ in range(500)]
    window = ref.GRID_WINDOW

    def one():
        if rng.random() < 0.03:  # INVALID of either kind
            return (rng.getrandbits(64) | 1 << 40, 1, 2, 3, 4) if rng.random() < 0.5 else (5, 6, 7, 8, rng.randrange(500, 1 << 32))
        return (rng.getrandbits(24), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), rng.randrange(500))

    earlier, statuses = [], set()
    repeated_rejects = 0
    with make_set(1 << 16) as s:
        model = Model(1 << 16)
        other = witness(1 << 16) if witness else None
        try:
            for _ in range(3):
                subs = []
                for i in range(5000):
                    p = rng.random()
                    if p < 0.3 and i:
                        subs.append(subs[rng.randrange(i)])
                    elif p < 0.6 and earlier:
                        subs.append(earlier[rng.randrange(len(earlier))])
                    else:
                        subs.append(one())
                want, r = check(s, model, job, sessions, subs, *window)
                assert r[5] > 500 and r[6] > 500 and r[3] > 50 and r[4] > 1000
                statuses |= {st for _, st in want}
                seen_subs = set(earlier)
                repeated_rejects += sum(1 for sub, (_, st) in zip(subs, want) if sub in seen_subs and not eligible(st))
                assert all(not st & DUPLICATE for _, st in want if not eligible(st))
                if other is not None:
                    rc, v, wr = raw_verify(other, job, sessions, subs, *window)
                    assert rc == _lib.BM_OK and ref.as_tuples(v, 5000) == want and result_tuple(wr) == r
                earlier += subs
        finally:
            if other is not None:
                other.close()
    assert repeated_rejects > 100
    # rejects, INVALID, shares and blocks inside and outside the window, plain and duplicate
    assert {0, 4, 8, 1, 9, 1 | 16, 9 | 16} <= statuses and any(st & BLOCK for st in statuses)


def key_is_the_hash(make_set):
    """Two sessions with the same extranonce1 and the same tuple: a duplicate; another
    extranonce1: not.  BLOCK without SHARE is eligible."""
    rng = random.Random(6000)
    job = ref.synthetic_job(rng, 10, 4, 4, 100, 0, nbits=0x2100ffff)  # the block target: 0xffff << 240
    en1 = rng.randbytes(4)
    sessions = [PoolSession(en1, U256), PoolSession(en1, U256), PoolSession(rng.randbytes(4), U256), PoolSession(en1, 0)]
    t = (0x01020304, 5, 6, 7)
    with make_set(16) as s:
        model = Model(16)
        want, r = check(s, model, job, sessions, [t + (0,), t + (1,), t + (2,)])
        assert [st for _, st in want] == [3, 3 | 16, 3] and want[0][0] == want[1][0] != want[2][0]
        # under target 0 the same hash is a block but no share: still eligible, still a duplicate
        u = (0x0a0b0c0d, 8, 9, 10)
        want, r = check(s, model, job, sessions, [u + (3,), u + (3,), t + (3,), u + (0,)])
        assert [st for _, st in want] == [2, 2 | 16, 2 | 16, 3 | 16] and r[5:] == (3, 1, 3)


def lifecycle(make_set, between=None):
    """clear() forgets; two sets are independent; an empty batch and an all-INVALID
    batch leave the set untouched.  between(): other calls on the set's context."""
    rng = random.Random(7000)
    job = ref.synthetic_job(rng, 45, 4, 4, 250, 2)
    sessions = open_sessions(rng, 4)
    subs = [fresh_sub(rng, 4, 7) for _ in range(100)]
    invalid = [(1 << 40, 1, 2, 3, 0), (5, 6, 7, 8, 7), (5, 6, 7, 8, U32)] * 30
    with make_set(300) as a, make_set(100) as b:
        ma, mb = Model(300), Model(100)
        check(a, ma, job, sessions, subs[:60])
        if between:
            between()
        check(b, mb, job, sessions, subs[40:])          # b has seen none of a's
        want, r = check(a, ma, job, sessions, subs)      # a remembers across b's call and the others'
        assert r[5:] == (60, 40, 100)
        want, r = check(a, ma, job, sessions, [])
        assert r == (0,) * 7 + (100,)
        want, r = check(a, ma, job, sessions, invalid)
        assert r[3] == 90 and r[5:] == (0, 0, 100) and all(w == ref.INVALID_VERDICT for w in want)
        a.clear()
        ma.seen.clear()
        assert a.count == 0 and a.capacity == 300 and b.count == 60
        if between:
            between()
        want, r = check(a, ma, job, sessions, subs[:10] + subs[:10])
        assert r[5:] == (10, 10, 10)
        want, r = check(b, mb, job, sessions, subs)
        assert r[5:] == (60, 40, 100)
        assert check(b, mb, job, sessions, [fresh_sub(rng, 4, 7)]) is None  # b is full; a is not
        check(a, ma, job, sessions, subs[5:15])
