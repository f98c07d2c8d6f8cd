"""The session table's reference and scenarios, shared by the CPU and the GPU tests
of bm_sessions_*: a pure-Python model -- big integers for the difficulty-to-target
function and the vardiff rule, tests/ledger_ref.Model (hashlib verdicts, a Python set,
a dict of rows) for the verify call.  The library is never its own reference; where a
scenario takes a `witness`, a CPU table runs beside a device table and every byte of
the two must agree as well.  Every comparison is exact equality.

The CPU table computes the rule with a 128-bit type and the device table in the 64-bit
words of bm_sessions_args.hpp, so the model is what judges both.  Two scenarios put
that arithmetic and the change list where small numbers never take them:
* wide_arithmetic: policies, difficulties, clocks and counts of every bit length up to
  64, with directed rows (directed_rows()) on the division's saturation edge, the step
  and range clamps, the band's edge with products above 2^64 and old * max_up around
  2^64.  It pins the high partial products and carries of mul_64x64, both branches of
  div_128by64 for divisors up to 2^64 - 1, the high words of le_128 and every clamp.
  The model alone counts, per class of CLASSES, the evaluated slots it sends through
  the rule and fails below 20 in any class;
* dense_changes: waves whose 64 lanes all change, one changed or one unchanged lane at
  a wave's first and last lane, a cap of zero, one short, and at a wave edge inside a
  longer list, and lists of 18 and 19 entries from five waves, either side of the
  host's switch between sorting the list and placing it by slot.
tests/test_sessions_arith.py runs trace()'s rule and directed_rows() against the
header itself, compiled for the host."""
import copy
import ctypes
import random

from distributed_bitcoin_minter_amd import PoolSession, _lib
import jobs_verify_ref as jref
import ledger_ref as lref
import pool_verify_ref as ref

U64 = (1 << 64) - 1
U32 = (1 << 32) - 1
DIFFICULTIES = (1, 2, 3, 0xffff, 0x10000, 1 << 32, (1 << 32) + 1, (1 << 53) - 1, 1 << 63, U64)
POLICY = dict(target_ms=1000, window_ms=9000, min_difficulty_fx=1, max_difficulty_fx=U64, burst=0, band_permille=100,
              max_up=4, max_down=4)


def target_fx(d):
    """T(d) = floor(0xffff * 2^240 / d)."""
    return (0xffff << 240) // d


def vardiff(p, now_ms, state):
    """The rule for one open slot -> (evaluated, new difficulty; the old one where unchanged)."""
    old, since, accepted, _ = state
    elapsed = now_ms - since if now_ms >= since else 0
    if not (elapsed >= p["window_ms"] or (p["burst"] != 0 and accepted >= p["burst"])):
        return False, old
    ideal = old * (min(accepted, U32) * p["target_ms"]) // max(elapsed, 1)
    new = min(max(ideal, max(1, old // p["max_down"])), min(old * p["max_up"], U64))
    new = min(max(new, p["min_difficulty_fx"]), p["max_difficulty_fx"])
    if abs(new - old) * 1000 <= old * p["band_permille"]:
        return True, old
    return True, new


class Model:
    """The specification, restated: a list of slots [extranonce1, difficulty, account]
    and of states [difficulty, since, accepted, retargets]."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.clear()

    def clear(self):
        self.count = 0
        self.slots = [[bytes(8), 0, 0] for _ in range(self.capacity)]
        self.states = [[0, 0, 0, 0] for _ in range(self.capacity)]

    def set(self, entries, now_ms, index=None):
        index = list(range(len(entries))) if index is None else index
        assert all(i < self.capacity for i in index)
        for i, (en1, fx, account) in zip(index, entries):
            self.slots[i] = [bytes(en1).ljust(8, b"\0"), fx, account]
            self.states[i] = [fx, now_ms, 0, 0]
            self.count = max(self.count, i + 1)

    def arrays(self, first=0, count=None):
        count = self.count - first if count is None else count
        rows = self.slots[first:first + count]
        return ([PoolSession(en1, target_fx(fx) if fx else 0) for en1, fx, _ in rows], [a for _, _, a in rows],
                [fx for _, fx, _ in rows])

    def snapshot(self):
        ses, acc, wgt = self.arrays(0, self.capacity)
        return (self.count, [(s.extranonce1, s.target) for s in ses], acc, wgt, [tuple(s) for s in self.states])

    def verify(self, jobs, subs, ledger_model=None, set_model=None):
        """ledger_ref.Model's answer over this table's arrays, or None for BM_EFULL;
        ledger_model None: a scratch ledger (with the persistent set_model, if any)."""
        sessions, accounts, weights = self.arrays()
        if ledger_model is None:
            ledger_model = lref.Model(max(accounts, default=0) + 1)
            ledger_model.set = set_model
        want = ledger_model.verify(jobs, sessions, subs, accounts, weights)
        if want is None:
            return None
        for sub, (_, st) in zip(subs, want[0]):
            if sub[4] < self.count and lref.classify(st) == lref.ACCEPTED:
                self.states[sub[4]][2] += 1
        return want

    def retarget(self, now_ms, p, cap):
        """(changes [(session, old, new, target)] or None for BM_EFULL, the five counts)."""
        changes, evaluated, n_open = [], [], 0
        for s in range(self.count):
            if self.states[s][0] == 0:
                continue
            n_open += 1
            ev, new = vardiff(p, now_ms, self.states[s])
            if ev:
                evaluated.append(s)
                if new != self.states[s][0]:
                    changes.append((s, self.states[s][0], new, target_fx(new)))
        counts = (n_open, len(evaluated), len(changes), sum(1 for c in changes if c[2] > c[1]),
                  sum(1 for c in changes if c[2] < c[1]))
        if len(changes) > cap:
            return None, counts
        for s in evaluated:
            self.states[s][1], self.states[s][2] = now_ms, 0
        for s, _, new, _ in changes:
            self.states[s][0] = self.slots[s][1] = new
            self.states[s][3] += 1
        return changes, counts


def snapshot(table):
    """Everything a table holds, over its whole capacity."""
    count, capacity = table.count, table.capacity
    ses, acc, wgt = table.get(0, capacity)
    return (count, [(bytes(s.extranonce1), int.from_bytes(bytes(s.target), "big")) for s in ses], acc, wgt,
            [s.as_tuple() for s in table.state(0, capacity)])


def raw_bytes(table):
    """The same as the bytes the C ABI returns."""
    capacity = table.capacity
    ses, acc, wgt = table.get(0, capacity)
    return bytes(ses), tuple(acc), tuple(wgt), bytes(table.state(0, capacity)), table.count


def raw_verify(table, ledger, share_set, jobs, subs):
    """One call through the C ABI into canary-filled arrays -> (status, verdicts, result)."""
    n = len(subs)
    out = (_lib.JobVerdict * (n + 1))()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    r = _lib.LedgerResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    if len(jobs) == 2 and isinstance(jobs[0], ctypes.Array):
        jarr, njobs = jobs
    else:
        jarr, _keep = _lib._jobs_array(jobs)
        njobs = len(jarr)
    rc = table._lib.bm_sessions_verify_jobs(table.handle, ledger.handle if ledger is not None else None,
                                            share_set.handle if share_set is not None else None,
                                            jarr if njobs else None, njobs, jref.sub_array(subs) if n else None, n, out,
                                            ctypes.byref(r))
    return rc, out, r


def raw_retarget(table, now_ms, p, cap):
    """One call into canary-filled arrays -> (status, changes as bytes, result)."""
    changes = (_lib.VardiffChange * (cap + 1))()
    ctypes.memset(changes, 0xA5, ctypes.sizeof(changes))
    r = _lib.VardiffResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    ps = _lib.VardiffPolicy(**p).struct
    rc = table._lib.bm_sessions_retarget(table.handle, now_ms, ctypes.byref(ps), changes, cap, ctypes.byref(r))
    return rc, changes, r


class Rig:
    """A table, its model and, optionally, a witness table (a CPU table beside a device
    table) with the ledgers and sets that go with each: every step runs on all of them
    and compares everything."""

    def __init__(self, make_table, capacity, witness=None, make_ledger=None, rows=0, make_set=None, set_capacity=0,
                 witness_ledger=None, witness_set=None):
        self.table, self.model = make_table(capacity), Model(capacity)
        self.other = witness(capacity) if witness else None
        self.ledger = make_ledger(rows) if make_ledger else None
        self.ledger_model = lref.Model(rows) if make_ledger else None
        self.set = make_set(set_capacity) if make_set else None
        self.set_model = jref.Model(set_capacity) if make_set else None
        if self.ledger_model is not None:
            self.ledger_model.set = self.set_model
        self.other_ledger = witness_ledger(rows) if witness and make_ledger else None
        self.other_set = witness_set(set_capacity) if witness and make_set else None

    def close(self):
        for obj in (self.table, self.other, self.ledger, self.set, self.other_ledger, self.other_set):
            if obj is not None:
                obj.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def same(self):
        assert snapshot(self.table) == self.model.snapshot()
        if self.other is not None:
            assert raw_bytes(self.table) == raw_bytes(self.other)
        if self.ledger is not None:
            assert lref.table(self.ledger) == self.ledger_model.table()
            if self.other_ledger is not None:
                assert bytes(self.ledger.read()) == bytes(self.other_ledger.read())
        if self.set is not None:
            assert self.set.count == len(self.set_model.seen)
            if self.other_set is not None:
                assert self.other_set.count == self.set.count

    def set_slots(self, entries, now_ms, index=None):
        self.table.set(entries, now_ms, index)
        self.model.set(entries, now_ms, index)
        if self.other is not None:
            self.other.set(entries, now_ms, index)
        self.same()

    def clear(self):
        self.table.clear()
        self.model.clear()
        if self.other is not None:
            self.other.clear()
        self.same()

    def verify(self, jobs, subs):
        """-> the model's answer, None for BM_EFULL (nothing has changed then)."""
        n = len(subs)
        want = self.model.verify(jobs, subs, self.ledger_model, self.set_model)
        rc, out, r = raw_verify(self.table, self.ledger, self.set, jobs, subs)
        if self.other is not None:
            rc2, out2, r2 = raw_verify(self.other, self.other_ledger, self.other_set, jobs, subs)
            assert rc2 == rc and bytes(out2) == bytes(out) and bytes(r2) == bytes(r)
        if want is None:
            assert rc == _lib.BM_EFULL
            assert bytes(out) == b"\xa5" * (40 * (n + 1)) and bytes(r) == b"\x5a" * 88
        else:
            assert rc == _lib.BM_OK
            assert ref.as_tuples(out, n) == want[0]
            assert lref.result_tuple(r) == want[1]
            assert bytes(out[n]) == b"\xa5" * 40
        self.same()
        return want

    def retarget(self, now_ms, p, cap):
        """-> (the model's changes, None for BM_EFULL, the counts)."""
        changes, counts = self.model.retarget(now_ms, p, cap)
        rc, got, r = raw_retarget(self.table, now_ms, p, cap)
        if self.other is not None:
            rc2, got2, r2 = raw_retarget(self.other, now_ms, p, cap)
            assert rc2 == rc and bytes(got2) == bytes(got) and bytes(r2) == bytes(r)
        assert r.as_tuple() == counts
        if changes is None:
            assert rc == _lib.BM_EFULL and bytes(got) == b"\xa5" * (56 * (cap + 1))
        else:
            assert rc == _lib.BM_OK
            assert [c.as_tuple() for c in got[:len(changes)]] == changes
            assert all(c.reserved == 0 for c in got[:len(changes)])
            assert bytes(got)[56 * len(changes):] == b"\xa5" * (56 * (cap + 1 - len(changes)))
        self.same()
        return changes, counts


# ---- scenarios ---------------------------------------------------------------------------

def block_job(rng, lo=0, hi=U32):
    """A job whose block target is 0xffff << 240: nearly every hash is a BLOCK, so a
    submission is accepted whatever its session's difficulty."""
    return lref.open_job(rng, lref.WIDE_NBITS, lo, hi)


def accepted_subs(rng, session, k, job=0):
    return [lref.sub(rng, session, job) for _ in range(k)]


def division(make_table, witness=None):
    """The listed difficulties through set and get."""
    rng = random.Random(11)
    with Rig(make_table, len(DIFFICULTIES) + 1, witness) as rig:
        rig.set_slots([(rng.randbytes(8), d, k) for k, d in enumerate(DIFFICULTIES)], 5)
        ses, acc, wgt = rig.table.get()
        assert [int.from_bytes(bytes(s.target), "big") for s in ses] == [(0xffff << 240) // d for d in DIFFICULTIES]
        assert int.from_bytes(bytes(ses[5].target), "big") == 0xffff << 208 and wgt == list(DIFFICULTIES)


def division_by_retarget(make_table, witness=None):
    """The listed difficulties as the NEW difficulty of a retarget (min = max = d pins
    it): the table's own division, against the big-integer quotient."""
    rng = random.Random(12)
    for d in DIFFICULTIES + tuple(rng.getrandbits(rng.randrange(1, 65)) | 1 for _ in range(6)):
        with Rig(make_table, 3, witness) as rig:
            old = 7 if d != 7 else 8
            rig.set_slots([(b"a" * 8, old, 0), (b"b" * 8, 0, 0), (b"c" * 8, old, 1)], 0)
            p = dict(POLICY, min_difficulty_fx=d, max_difficulty_fx=d, band_permille=0, window_ms=0)
            changes, counts = rig.retarget(1, p, 2)
            assert changes == [(0, old, d, (0xffff << 240) // d), (2, old, d, (0xffff << 240) // d)]
            assert counts == (2, 2, 2, 2 * (d > old), 2 * (d < old))


# (old, accepted, since_ms, the new difficulty or None where the slot is unchanged): retarget at NOW under POLICY
NOW = 20000
EDGES = [(10000, 11, 10000, None),        # ideal 11000: exactly on the upper band edge
         (10000, 11, 10001, 11001),       # one above it
         (10000, 9, 10000, None),         # ideal 9000: exactly on the lower band edge
         (10000, 9, 9999, 8999),          # one below it
         (10000, 100, 10000, 40000),      # ideal 100000: the max_up clamp
         (10000, 1, 10000, 2500),         # ideal 1000: the max_down clamp
         (10000, 0, 10000, 2500),         # accepted = 0: ideal 0
         (U64, 100, 10000, None),         # old * max_up saturates at 2^64 - 1 = old
         (U64, 0, 10000, U64 // 4),
         (1, 0, 10000, None),             # max(1, floor(1 / 4)) = 1
         (1, 30, 10000, 3),
         (10000, 50, 15000, "idle"),      # a window of 5000 < 9000 and no burst: not evaluated
         (1 << 63, 2, 10000, 1 << 61)]    # ideal 0.2 * 2^63 is below old / 4


def edge_cases(make_table, witness=None):
    rng = random.Random(13)
    jobs = (block_job(rng),)
    with Rig(make_table, 70, witness) as rig:
        # slots 0.., then the same cases again from slot 57 on, across the wave edge at 64
        for base in (0, 57):
            for k, (old, _, since, _) in enumerate(EDGES):
                rig.set_slots([(rng.randbytes(8), old, k)], since, [base + k])
        subs = [s for base in (0, 57) for k, e in enumerate(EDGES) for s in accepted_subs(rng, base + k, e[1])]
        want = rig.verify(jobs, subs)
        assert all(st & lref.BLOCK for _, st in want[0])
        expect = [(base + k, e[0], e[3], target_fx(e[3])) for base in (0, 57) for k, e in enumerate(EDGES)
                  if e[3] not in (None, "idle")]
        before = raw_bytes(rig.table)
        # one entry short: BM_EFULL, the exact counts, and the table, windows and counters included, as before
        changes, counts = rig.retarget(NOW, POLICY, len(expect) - 1)
        idle = sum(1 for e in EDGES if e[3] == "idle")
        assert changes is None and counts == (2 * len(EDGES), 2 * (len(EDGES) - idle), len(expect), 2 * 3, 2 * 5)
        assert raw_bytes(rig.table) == before
        changes, counts = rig.retarget(NOW, POLICY, len(expect))  # cap == changed
        assert changes == expect
        states = [s.as_tuple() for s in rig.table.state()]
        for base in (0, 57):
            for k, (old, accepted, since, new) in enumerate(EDGES):
                if new == "idle":
                    assert states[base + k] == (old, since, accepted, 0)
                else:
                    assert states[base + k] == (old if new is None else new, NOW, 0, 0 if new is None else 1)
        # a second step right away: no window has passed, nothing is evaluated
        assert rig.retarget(NOW + 1, POLICY, 0) == ([], (2 * len(EDGES), 0, 0, 0, 0))


def burst_and_clock(make_table, witness=None):
    """A burst with elapsed = 0 (D = 1), now_ms < since_ms with and without a burst,
    and the min and max clamps."""
    rng = random.Random(14)
    jobs = (block_job(rng),)
    p = dict(POLICY, burst=5)
    with Rig(make_table, 8, witness) as rig:
        rig.set_slots([(rng.randbytes(8), 10000, 0), (rng.randbytes(8), 10000, 0), (rng.randbytes(8), 0, 0),
                       (rng.randbytes(8), 10000, 0), (rng.randbytes(8), 10000, 0)], 5000)
        rig.verify(jobs, accepted_subs(rng, 0, 5) + accepted_subs(rng, 1, 4) + accepted_subs(rng, 3, 6) +
                   accepted_subs(rng, 2, 2) + accepted_subs(rng, 7, 1))
        assert [s.accepted for s in rig.table.state()] == [5, 4, 2, 6, 0]  # a closed slot tallies; slot 7 is past count
        # elapsed = 0: ideal = 10000 * 5000 / 1, cut by max_up; slot 1 has 4 < burst
        changes, counts = rig.retarget(5000, p, 8)
        assert changes == [(0, 10000, 40000, target_fx(40000)), (3, 10000, 40000, target_fx(40000))]
        assert counts == (4, 2, 2, 2, 0)
        # now_ms < since_ms: elapsed = 0, so no window is over; the burst still fires (slot 1 reaches 5)
        rig.verify(jobs, accepted_subs(rng, 1, 1))
        assert rig.retarget(4000, dict(POLICY), 8) == ([], (4, 0, 0, 0, 0))
        changes, counts = rig.retarget(4000, p, 8)
        assert changes == [(1, 10000, 40000, target_fx(40000))] and counts == (4, 1, 1, 1, 0)
        # the min clamp: everything is evaluated (window 0) with accepted = 0, ideal 0 -> old / 4, then [min, max]
        lo = dict(POLICY, window_ms=0, min_difficulty_fx=9500, max_difficulty_fx=20000, band_permille=0)
        changes, counts = rig.retarget(4000, lo, 8)
        assert [c[:3] for c in changes] == [(0, 40000, 10000), (1, 40000, 10000), (3, 40000, 10000), (4, 10000, 9500)]
        assert counts == (4, 4, 4, 0, 4)
        # the max clamp: a burst of 6 at elapsed = 0 asks for 4 * old
        rig.verify(jobs, accepted_subs(rng, 0, 6))
        hi = dict(POLICY, window_ms=10 ** 9, burst=5, band_permille=0, max_difficulty_fx=12000)
        changes, counts = rig.retarget(4000, hi, 8)
        assert changes == [(0, 10000, 12000, target_fx(12000))] and counts == (4, 1, 1, 1, 0)
        assert [s.retargets for s in rig.table.state()] == [3, 2, 0, 2, 1]


def set_semantics(make_table, witness=None):
    """Repeated indices (the later entry wins), closing a slot, count, never-set slots, clear."""
    rng = random.Random(15)
    with Rig(make_table, 300, witness) as rig:
        assert (rig.table.count, rig.table.capacity) == (0, 300)
        a, b, c = (rng.randbytes(8) for _ in range(3))
        rig.set_slots([(a, 5, 1), (b, 6, 2), (c, 7, 3), (a, 8, 4)], 100, [5, 129, 5, 5])
        assert rig.table.count == 130
        ses, acc, wgt = rig.table.get()
        assert (bytes(ses[5].extranonce1), acc[5], wgt[5]) == (a, 4, 8) and wgt[129] == 6 and wgt[0] == 0
        assert bytes(ses[4]) == bytes(40) and rig.table.state(4, 1)[0].as_tuple() == (0, 0, 0, 0)
        rig.set_slots([(b, 0, 9)], 200, [129])  # closes it: target zero, weight 0; count stays
        assert rig.table.count == 130 and bytes(rig.table.get(129, 1)[0][0].target) == bytes(32)
        assert rig.table.state(129, 1)[0].as_tuple() == (0, 200, 0, 0)
        rig.set_slots([(rng.randbytes(8), rng.getrandbits(64) | 1, rng.getrandbits(32)) for _ in range(299)], 7)
        rig.set_slots([(c, 1, 0)], 9, [299])
        assert rig.table.count == 300
        rig.set_slots([], 1)
        # an index at capacity: BM_EINVAL, nothing changes, the entries before it included
        idx = (ctypes.c_uint32 * 2)(3, 300)
        init = (_lib.SessionInit * 2)()
        init[0].difficulty_fx = init[1].difficulty_fx = 77
        assert rig.table._lib.bm_sessions_set(rig.table.handle, idx, 2, init, 1) == _lib.BM_EINVAL
        if rig.other is not None:
            assert rig.other._lib.bm_sessions_set(rig.other.handle, idx, 2, init, 1) == _lib.BM_EINVAL
        rig.same()
        rig.table.clear()
        rig.model.clear()
        if rig.other is not None:
            rig.other.clear()
        rig.same()
        assert rig.table.count == 0
        rig.set_slots([(a, 3, 0)], 1, [2])
        assert rig.table.count == 3


GPU_SLOTS = (0, 5, 63, 64, 129, 299)


def sequence(make_table, make_ledger, make_set, witness=None, witness_ledger=None, witness_set=None, between=None):
    """Capacity 300, open slots at 0, 5, 63, 64, 129 and 299 with closed slots in
    between, three jobs, batches of about 200 with unknown sessions and jobs, repeats,
    ntime rejects and above-target rejects: set, verify x3, retarget (first one entry
    short: BM_EFULL), verify, retarget.  between(): other calls on the table's context."""
    rng = random.Random(16)
    jobs3, _ = jref.three_jobs()
    jobs = (jobs3[0], jobs3[2], block_job(rng, 1000, 2000))  # 0- and 3-entry branches, and a job that accepts
    for with_ledger, with_set in ((True, True), (True, False), (False, True), (False, False)):
        with Rig(make_table, 300, witness, make_ledger if with_ledger else None, 7, make_set if with_set else None, 1024,
                 witness_ledger, witness_set) as rig:
            fx = {0: 1, 5: 1, 63: 1 << 20, 64: 1 << 40, 129: U64, 299: 1 << 33}
            rig.set_slots([(rng.randbytes(8), fx[s], s % 7) for s in GPU_SLOTS], 1000, list(GPU_SLOTS))
            rig.set_slots([(rng.randbytes(8), 0, 6)], 1000, [200])
            pool = list(GPU_SLOTS) + [1, 200, 300, U32]  # a never-set slot, a closed one, two unknown sessions

            def batch(n):
                subs = jref.job_subs(rng, jobs, 1, [(0, 1, 2, 2, 2, 3)[i % 6] for i in range(n)])
                subs = [s[:4] + (pool[rng.randrange(len(pool))], s[5]) for s in subs]
                for i in range(10, n, 9):
                    subs[i] = subs[i - 7]  # a repeat: a duplicate where it is eligible
                return subs

            total = 0
            for k in range(3):
                want = rig.verify(jobs, batch(200 + k))
                total += want[1][8]
                if between:
                    between()
                    rig.same()
            statuses = {st for _, st in want[0]}
            assert lref.INVALID in statuses and 0 in statuses and any(st & lref.NTIME for st in statuses)
            assert with_set == any(st & lref.DUPLICATE for st in statuses)
            assert sum(s.accepted for s in rig.table.state()) == total > 50
            p = dict(POLICY, window_ms=5000, band_permille=0)
            changes, counts = copy.deepcopy(rig.model).retarget(8000, p, 300)
            short = len(changes) - 1
            assert len(changes) >= 3 and changes[0][0] < 64 <= changes[-1][0]  # the list straddles waves
            before = raw_bytes(rig.table)
            assert rig.retarget(8000, p, short)[0] is None and raw_bytes(rig.table) == before
            assert rig.retarget(8000, p, short + 1)[0] == changes
            rig.verify(jobs, batch(190))
            rig.retarget(14000, p, 300)


def contention(make_table, make_set, witness=None, witness_set=None):
    """130 copies of one accepted submission on one session: with a set 129 are
    duplicates and one tallies, without one all 130 tally."""
    rng = random.Random(17)
    jobs = (block_job(rng),)
    one = lref.sub(rng, 64)
    for with_set in (True, False):
        with Rig(make_table, 300, witness, None, 0, make_set if with_set else None, 256, None, witness_set) as rig:
            rig.set_slots([(rng.randbytes(8), 1 << 32, 0)], 0, [64])
            want = rig.verify(jobs, [one] * 130)
            assert want[1][8] == (1 if with_set else 130) and want[1][5] == (129 if with_set else 0)
            assert rig.table.state(64, 1)[0].accepted == (1 if with_set else 130)


def trace(p, now_ms, state):
    """The rule's intermediate values for one evaluated slot, in big integers: what the
    directed rows are found by and the coverage classes are read from.  `ideal` is the
    true quotient, 2^64 or more where the table saturates it."""
    old, since, accepted, _ = state
    D = max(now_ms - since if now_ms >= since else 0, 1)
    N = min(accepted, U32) * p["target_ms"]
    lo, hi = max(1, old // p["max_down"]), min(old * p["max_up"], U64)
    ideal = old * N // D
    cut = min(max(ideal, lo), hi)
    new = min(max(cut, p["min_difficulty_fx"]), p["max_difficulty_fx"])
    held = abs(new - old) * 1000 <= old * p["band_permille"]
    assert vardiff(dict(p, window_ms=0), now_ms, state) == (True, old if held else new)
    return dict(old=old, N=N, D=D, P=old * N, lo=lo, hi=hi, ideal=ideal, cut=cut, new=new, held=held)


CLASSES = ("both high words", "P.hi >= D", "0 < P.hi < D", "0 < P.hi < D, D >= 2^63", "inside [lo, hi]", "cut by lo",
           "cut by hi", "cut by min", "cut by max", "old * max_up >= 2^64", "band product >= 2^64", "raised", "lowered",
           "held by the band")


def classes(p, t):
    """The coverage classes of CLASSES an evaluated slot falls in, from its trace."""
    p_hi = t["P"] >> 64
    diff = abs(t["new"] - t["old"])
    is_in = {"both high words": t["old"] >> 32 and t["N"] >> 32,
             "P.hi >= D": p_hi >= t["D"],
             "0 < P.hi < D": 0 < p_hi < t["D"],
             "0 < P.hi < D, D >= 2^63": 0 < p_hi < t["D"] and t["D"] >> 63,
             "inside [lo, hi]": t["lo"] < t["ideal"] < t["hi"],
             "cut by lo": t["ideal"] < t["lo"],
             "cut by hi": t["ideal"] > t["hi"],
             "cut by min": t["cut"] < p["min_difficulty_fx"],
             "cut by max": t["cut"] > p["max_difficulty_fx"],
             "old * max_up >= 2^64": t["old"] * p["max_up"] >> 64,
             "band product >= 2^64": diff * 1000 >> 64 or t["old"] * p["band_permille"] >> 64,
             "raised": not t["held"] and t["new"] > t["old"],
             "lowered": not t["held"] and t["new"] < t["old"],
             "held by the band": t["held"] and diff != 0}
    return [c for c in CLASSES if is_in[c]]


def find(p, want, olds, accepteds, elapseds):
    """The first (old, accepted, elapsed) of the grid whose trace `want` accepts: a
    directed row computed by the model."""
    for old in olds:
        for accepted in accepteds:
            for elapsed in elapseds:
                if want(trace(p, elapsed, (old, 0, accepted, 0))):
                    return old, accepted, elapsed
    raise AssertionError("no such row in the grid")


# The policies of the directed rows of wide_arithmetic, one per round from the first on.
# 0: the division's and the band's edges; 1 and 2: old * max_up around 2^64 where 2^64
# (2^62 * 4) and 2^64 + 1 (67280421310721 * 274177) factor; 3: a [min, max] in mid-range.
DIRECTED = (dict(target_ms=990, window_ms=0, min_difficulty_fx=50, max_difficulty_fx=U64, burst=0, band_permille=100,
                 max_up=3, max_down=5),
            dict(target_ms=U32, window_ms=0, min_difficulty_fx=1, max_difficulty_fx=U64, burst=0, band_permille=0,
                 max_up=4, max_down=2),
            dict(target_ms=U32, window_ms=0, min_difficulty_fx=1, max_difficulty_fx=U64, burst=0, band_permille=0,
                 max_up=274177, max_down=2),
            dict(target_ms=U32, window_ms=0, min_difficulty_fx=10 ** 6, max_difficulty_fx=10 ** 12, burst=0,
                 band_permille=0, max_up=2, max_down=2))


def directed_rows(k):
    """[(old, accepted, elapsed)] under DIRECTED[k], in the style of EDGES; each row's
    claim is asserted on the model's trace."""
    p, rows = DIRECTED[k], []

    def row(old, accepted, elapsed, claim):
        assert claim(trace(p, elapsed, (old, 0, accepted, 0))), (k, old, accepted, elapsed)
        rows.append((old, accepted, elapsed))

    if k == 0:
        # P = 2^63 * 2 * 990 = 990 * 2^64: P.hi against D = 989, 990, 991
        for e in (989, 990, 991):
            row(1 << 63, 2, e, lambda t: (t["P"] >> 64) - t["D"] == 990 - e)
        for delta in (-1, 0, 1):  # the ideal one below, on and one above each of lo, hi and min
            rows.append(find(p, lambda t: t["ideal"] - t["lo"] == delta, range(5000, 5010), (1,), range(4900, 5000)))
            rows.append(find(p, lambda t: t["ideal"] - t["hi"] == delta, range(100, 120), (1, 2), range(300, 700)))
            rows.append(find(p, lambda t: t["lo"] < t["ideal"] < t["hi"] and t["ideal"] - p["min_difficulty_fx"] == delta,
                             range(200, 240), (1,), range(3000, 5000)))
        row(U64 - 1, 1, 990, lambda t: t["ideal"] == U64 - 1)  # one below max, then on it; (1 << 63, 2, 990) is one above
        row(U64, 1, 990, lambda t: t["ideal"] == t["hi"] == U64)
        # the band's edge with both products above 2^64: diff * 1000 == old * 100 lowered (ideal = 0.9 old) and
        # raised (ideal = 1.1 old), and the nearest values on each side
        q = 2 * 10 ** 17
        row(10 * q, 1, 1100, lambda t: t["held"] and (t["old"] - t["new"]) * 1000 == t["old"] * 100 >= 1 << 64)
        row(10 * q - 1, 1, 1100, lambda t: not t["held"] and (t["old"] - t["new"]) * 1000 - t["old"] * 100 == 100)
        row(10 * q + 1, 1, 1100, lambda t: not t["held"] and (t["old"] - t["new"]) * 1000 - t["old"] * 100 == 900)
        row(10 * q, 1, 900, lambda t: t["held"] and (t["new"] - t["old"]) * 1000 == t["old"] * 100 >= 1 << 64)
        row(10 * q + 1, 1, 900, lambda t: t["held"] and t["old"] * 100 - (t["new"] - t["old"]) * 1000 == 100)
        row(10 * q, 1, 899, lambda t: not t["held"] and t["new"] > t["old"])
        for delta in (-1, 0, 1):  # old * 3 = 2^64 - 4, 2^64 - 1, 2^64 + 2
            row(U64 // 3 + delta, 6, 1, lambda t: t["old"] * 3 == (1 << 64) - 1 + 3 * delta and t["new"] == t["hi"])
    elif k == 1:
        for delta in (-1, 0, 1):  # old * 4 = 2^64 - 4, 2^64, 2^64 + 4
            row((1 << 62) + delta, 1, 0, lambda t: t["old"] * 4 == (1 << 64) + 4 * delta and t["new"] == t["hi"])
    elif k == 2:
        for delta in (-1, 0, 1):  # old * 274177 = 2^64 + 1 and 274177 either side
            row(67280421310721 + delta, 1, 0,
                lambda t: t["old"] * 274177 == (1 << 64) + 1 + 274177 * delta and t["new"] == t["hi"])
    else:
        for delta in (-1, 0, 1):  # elapsed = target_ms and one accepted: the ideal is old itself
            row(p["min_difficulty_fx"] + delta, 1, U32, lambda t: t["ideal"] - p["min_difficulty_fx"] == delta)
            row(p["max_difficulty_fx"] + delta, 1, U32, lambda t: t["ideal"] - p["max_difficulty_fx"] == delta)
    return rows


WIDE_ROUNDS, WIDE_SLOTS, WIDE_FLOOR = 48, 300, 20
FORMS = ("zero", "one", "thousands", "wide", "top", "negative")


def random_bits(rng, lo, hi):
    """A value whose bit length is uniform in lo..hi."""
    bits = rng.randrange(lo, hi + 1)
    return (1 << (bits - 1)) | rng.getrandbits(bits - 1)


def wide_round(rng, r):
    """One round of wide_arithmetic as data: (policy, now_ms, [(entries, since_ms,
    index)] -- one per set call --, submissions)."""
    if r < len(DIRECTED):
        p = dict(DIRECTED[r])
    else:
        factor = lambda: rng.choice((1, 2, 4, random_bits(rng, 1, 32), U32))
        lo, hi = sorted((random_bits(rng, 1, 64), random_bits(rng, 1, 64)))
        p = dict(target_ms=U32 if r % 4 == 1 else random_bits(rng, 1, 32), window_ms=0, burst=0,
                 band_permille=rng.choice((0, 1, 100, 999, 1000)), max_up=factor(), max_down=factor(),
                 min_difficulty_fx=lo if r % 2 else 1, max_difficulty_fx=hi if r % 2 else U64)
        if r in (10, 25, 40):  # the burst side of the rule: no window ever ends
            p.update(window_ms=U64, burst=rng.randrange(1, 7))
    # five of the six forms of `elapsed`, one per set call; now_ms = 2^64 - 1 where none is negative
    forms = [f for k, f in enumerate(FORMS) if k != r % len(FORMS)]
    rng.shuffle(forms)
    now_ms = U64 if "negative" not in forms else (3 << 62) + rng.getrandbits(61)
    since = {"zero": now_ms, "one": now_ms - 1, "thousands": now_ms - rng.randrange(1000, 20000),
             "wide": now_ms - random_bits(rng, 33, 63), "top": rng.randrange(1000),
             "negative": min(U64, now_ms + random_bits(rng, 1, 40))}
    # about one slot in ten is closed, and one at each wave edge, on the side that alternates with the round
    edge = (63, 128, 191, 256) if r % 2 else (64, 127, 192, 255)
    sets, accepted = [], {}
    for g, form in enumerate(forms):
        index = [s for s in range(WIDE_SLOTS) if (s + r) % len(forms) == g]
        entries = []
        for s in index:
            old = 0 if s % 10 == r % 10 or s in edge else random_bits(rng, 1, 64)
            # slot % 7 accepted submissions; a part of the slots of a high `old` get two or more (N can pass 2^32)
            accepted[s] = max(s % 7, 2) if old >> 32 and s % 2 else s % 7
            entries.append((rng.randbytes(8), old, s % 5))
        sets.append((entries, since[form], index))
    if r < len(DIRECTED):  # the directed rows, across the wave edge at 64: a set call per distinct `elapsed`
        by_since = {}
        for s, (old, k, elapsed) in enumerate(directed_rows(r), 64 - 9):
            accepted[s] = k
            by_since.setdefault(now_ms - elapsed, []).append((s, (rng.randbytes(8), old, s % 5)))
        sets += [([e for _, e in rows], at, [s for s, _ in rows]) for at, rows in by_since.items()]
    subs = [sub for s in range(WIDE_SLOTS) for sub in accepted_subs(rng, s, accepted[s])]
    return p, now_ms, sets, subs


def wide_arithmetic(make_table, witness=None):
    """The vardiff rule at full width: 48 rounds on one table of 300 slots, each with a
    policy, difficulties and clocks of random bit lengths up to 64 (target_ms up to
    2^32 - 1, elapsed from 0 to above 2^63 and negative), about a tenth of the slots
    closed around the wave edges, one verify and one retarget; the first rounds carry
    the directed rows of directed_rows().  The model alone first runs every round and
    counts the evaluated slots per class of CLASSES: fewer than 20 in any is a failure
    of the scenario, before a table is looked at.  -> the counts."""
    rng = random.Random(19)
    jobs = (block_job(rng),)
    rounds = [wide_round(rng, r) for r in range(WIDE_ROUNDS)]
    model, cover = Model(WIDE_SLOTS), dict.fromkeys(CLASSES, 0)
    for p, now_ms, sets, subs in rounds:
        model.clear()
        for entries, since_ms, index in sets:
            model.set(entries, since_ms, index)
        model.verify(jobs, subs)
        for state in model.states:
            if state[0] and vardiff(p, now_ms, state)[0]:
                for c in classes(p, trace(p, now_ms, state)):
                    cover[c] += 1
        model.retarget(now_ms, p, WIDE_SLOTS)
    assert all(n >= WIDE_FLOOR for n in cover.values()), cover
    with Rig(make_table, WIDE_SLOTS, witness) as rig:
        for p, now_ms, sets, subs in rounds:
            rig.clear()
            for entries, since_ms, index in sets:
                rig.set_slots(entries, since_ms, index)
            rig.verify(jobs, subs)
            changes, counts = rig.retarget(now_ms, p, WIDE_SLOTS)
            assert changes is not None and counts[0] == sum(1 for s in rig.model.states if s[0])
    return cover


def dense_changes(make_table, witness=None):
    """Full waves of changed lanes and both orderings of the change list: 300 open slots,
    window 0, band 0 and nothing accepted, so every slot with old >= 2 is lowered to
    max(1, old / 4) and a slot with old = 1 is evaluated and unchanged."""
    rng = random.Random(20)
    n = WIDE_SLOTS
    p = dict(POLICY, window_ms=0, band_permille=0)

    def fill(rig, changed, now_ms):
        """Every slot anew: its own difficulty (the slot's number in bits 2..11 of 12 to 64) where it is to change, else 1."""
        olds = [(rng.getrandbits(rng.randrange(53)) << 12) | ((s + 1) << 2) | rng.getrandbits(2) if s in changed else 1
                for s in range(n)]
        rig.set_slots([(rng.randbytes(8), old, s % 3) for s, old in enumerate(olds)], now_ms)
        return [(s, old, old // 4, target_fx(old // 4)) for s, old in enumerate(olds) if s in changed]

    def full(rig, now_ms, cap, changed):
        """BM_EFULL with the exact counts, and the table byte for byte as before (the Rig checks the canaries)."""
        before = raw_bytes(rig.table)
        assert rig.retarget(now_ms, p, cap) == (None, (n, n, changed, 0, changed))
        assert raw_bytes(rig.table) == before

    with Rig(make_table, n, witness) as rig:
        # every lane of every wave changed: the cap one short, zero, at the first wave's edge; then the whole list
        expect = fill(rig, set(range(n)), 0)
        for cap in (n - 1, 0, 64):
            full(rig, 1, cap, n)
        assert rig.retarget(1, p, n) == (expect, (n, n, n, 0, n))
        assert len({c[3] for c in expect}) == n
        assert [s.as_tuple() for s in rig.table.state()] == [(c[2], 1, 0, 1) for c in expect]
        # nothing changed: an empty list fits a cap of zero
        fill(rig, set(), 2)
        assert rig.retarget(3, p, 0) == ([], (n, n, 0, 0, 0))
        # one changed lane among unchanged ones, at the end and at the start of a wave
        for k, lane in enumerate((63, 0, 64)):
            expect = fill(rig, {lane}, 4 + k)
            full(rig, 10 + k, 0, 1)
            assert rig.retarget(10 + k, p, 1) == (expect, (n, n, 1, 0, 1))
        # and the complement: every lane changed but that one
        for k, lane in enumerate((63, 0, 64)):
            expect = fill(rig, set(range(n)) - {lane}, 20 + k)
            full(rig, 30 + k, n - 2, n - 1)
            assert rig.retarget(30 + k, p, n - 1) == (expect, (n, n, n - 1, 0, n - 1))
        # the host's two orderings of a list from all five waves: 18 * 16 < 300 sorts, 19 * 16 >= 300 places by slot
        spread = [0, 63, 64, 255, 256, 299, 5, 31, 62, 65, 100, 127, 128, 170, 191, 192, 230, 270, 290]
        for k in (18, 19):
            assert {s // 64 for s in spread[:k]} == set(range(5)) and len(set(spread[:k])) == k
            expect = fill(rig, set(spread[:k]), 40 + k)
            full(rig, 70 + k, k - 1, k)
            assert rig.retarget(70 + k, p, k) == (expect, (n, n, k, 0, k))
            assert [c[0] for c in expect] == sorted(spread[:k])


def refusals(make_table, make_ledger, make_set, foreign_ledger=None, foreign_set=None):
    """Every refusal leaves the table, the ledger, the set and the caller's arrays alone."""
    rng = random.Random(18)
    jobs = (block_job(rng),)
    with Rig(make_table, 4, None, make_ledger, 3, make_set, 8) as rig:
        rig.set_slots([(rng.randbytes(8), 1, 0), (rng.randbytes(8), 1, 2)], 0)
        rig.verify(jobs, accepted_subs(rng, 0, 5))
        assert rig.verify(jobs, accepted_subs(rng, 1, 4)) is None  # BM_EFULL from the capacity-8 set
        one = accepted_subs(rng, 0, 1)

        def refused(call, status=_lib.BM_EINVAL):
            rc, out, r = call()
            assert rc == status and bytes(out) == b"\xa5" * len(bytes(out)) and bytes(r) == b"\x5a" * len(bytes(r))
            rig.same()

        lib, h = rig.table._lib, rig.table.handle
        # an account equal to the ledger's rows, on a slot no submission names; fine without a ledger
        rig.set_slots([(rng.randbytes(8), 1, 3)], 0, [3])
        refused(lambda: raw_verify(rig.table, rig.ledger, rig.set, jobs, one))
        refused(lambda: raw_verify(rig.table, rig.ledger, None, jobs, one))
        rig.set_slots([(rng.randbytes(8), 1, 1)], 0, [3])
        bad, _keep = _lib._jobs_array(jobs)
        bad[0].job.nbranch = 33
        refused(lambda: raw_verify(rig.table, rig.ledger, rig.set, (bad, 1), one))
        refused(lambda: raw_verify(rig.table, None, None, (bad, 1), one))
        if foreign_ledger is not None:
            with foreign_ledger(3) as other, foreign_set(8) as other_set:
                refused(lambda: raw_verify(rig.table, other, None, jobs, one))
                refused(lambda: raw_verify(rig.table, None, other_set, jobs, one))
                refused(lambda: raw_verify(rig.table, rig.ledger, other_set, jobs, one))
                assert other_set.count == 0 and lref.table(other) == [lref.EMPTY] * 3
        r = _lib.LedgerResult()
        assert lib.bm_sessions_verify_jobs(None, None, None, None, 0, None, 0, None, ctypes.byref(r)) == _lib.BM_EINVAL
        assert lib.bm_sessions_verify_jobs(h, None, None, None, 0, None, 0, None, None) == _lib.BM_EINVAL
        # retarget: every bad policy, NULL pointers, with untouched outputs
        for bad_p in (dict(target_ms=0), dict(target_ms=1 << 32), dict(min_difficulty_fx=0),
                      dict(min_difficulty_fx=5, max_difficulty_fx=4), dict(max_up=0), dict(max_down=0),
                      dict(band_permille=1001)):
            refused(lambda: raw_retarget(rig.table, 10 ** 6, dict(POLICY, **bad_p), 4))
        ps = _lib.VardiffPolicy(**POLICY).struct
        vr, ch = _lib.VardiffResult(), (_lib.VardiffChange * 4)()
        f = lib.bm_sessions_retarget
        assert f(None, 1, ctypes.byref(ps), ch, 4, ctypes.byref(vr)) == _lib.BM_EINVAL
        assert f(h, 1, None, ch, 4, ctypes.byref(vr)) == _lib.BM_EINVAL
        assert f(h, 1, ctypes.byref(ps), None, 4, ctypes.byref(vr)) == _lib.BM_EINVAL
        assert f(h, 1, ctypes.byref(ps), ch, 4, None) == _lib.BM_EINVAL
        # get, set, count
        ses = (_lib.PoolSessionStruct * 5)()
        ctypes.memset(ses, 0xA5, ctypes.sizeof(ses))
        for first, count in ((0, 5), (4, 1), (5, 0), (U64, 2)):
            assert lib.bm_sessions_get(h, first, count, ses, None, None, None) == _lib.BM_EINVAL, (first, count)
        assert lib.bm_sessions_get(None, 0, 1, ses, None, None, None) == _lib.BM_EINVAL
        assert bytes(ses) == b"\xa5" * 200
        assert lib.bm_sessions_get(h, 4, 0, None, None, None, None) == _lib.BM_OK
        assert lib.bm_sessions_get(h, 0, 4, None, None, None, None) == _lib.BM_OK
        assert lib.bm_sessions_set(h, None, 1, None, 0) == _lib.BM_EINVAL
        assert lib.bm_sessions_set(None, None, 0, None, 0) == _lib.BM_EINVAL
        assert lib.bm_sessions_set(h, None, 5, (_lib.SessionInit * 5)(), 0) == _lib.BM_EINVAL
        assert lib.bm_sessions_count(h, None, None) == _lib.BM_EINVAL and lib.bm_sessions_clear(None) == _lib.BM_EINVAL
        c = ctypes.c_uint64(0)
        assert lib.bm_sessions_count(None, ctypes.byref(c), None) == _lib.BM_EINVAL
        rig.same()
        # an empty batch is legal and changes nothing; and the table still answers
        rc, out, r = raw_verify(rig.table, rig.ledger, rig.set, jobs, [])
        assert rc == _lib.BM_OK and lref.result_tuple(r) == (0,) * 7 + (5, 0, 0, 0)
        rig.same()
        assert rig.verify(jobs, accepted_subs(rng, 1, 3))[1][6:9] == (3, 8, 3)


def creation():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.bm_sessions_create_cpu(0, ctypes.byref(h)) == _lib.BM_EINVAL
    assert lib.bm_sessions_create_cpu(_lib.BM_MAX_POOL_SESSIONS + 1, ctypes.byref(h)) == _lib.BM_EINVAL
    assert lib.bm_sessions_create_cpu(1, None) == _lib.BM_EINVAL and h.value is None
    lib.bm_sessions_destroy(None)
