"""The pool verifier's reference and cases, shared by the CPU and the GPU tests of
bm_pool_verify_cpu / bm_pool_verify_gpu: hashlib only, in the manner of
tests/verify_ref.py.  A verdict is rebuilt here from the job's pieces and the
submission's session (coinbase under the session's extranonce1, branch fold,
field order, the session's own target, the ntime window); neither entry of the
library is the other's reference.  Every grid is built once per process and left
unchanged."""
import functools
import random
import struct

from distributed_bitcoin_minter_amd import Job, PoolSession, _lib
from verify_ref import BLOCK, INVALID, INVALID_VERDICT, SHARE, U32, U64, U256, block_target, sha256d

NTIME = 8

# the field's (extranonce1 || extranonce2) byte offset in the coinbase mod 64, each
# with 0 and 2 whole blocks before it, the two sizes, and the coinbase's total
# length mod 64
OFFSETS = (0, 1, 3, 47, 48, 49, 56, 60, 61, 63)
BLOCKS_BEFORE = (0, 2)
SIZES1 = (1, 4, 8)
SIZES2 = (1, 4, 8)
LENGTHS = (55, 56, 63, 0, 1)
PER_JOB = 65
SESSIONS_PER_JOB = 7
GRID_NBITS = 0x2000ffff       # the block target 0xffff << 232: about one hash in 256
# per-session share targets: the extremes, about a half, about a quarter, and below the block target
GRID_TARGETS = (1 << 255, 1 << 254, U256, 0, 1 << 255, 0xffff << 200, 1 << 253)
GRID_WINDOW = (1 << 30, 3 << 30)  # about half of the random ntimes lie inside


def verdict(job, sessions, sub, lo=0, hi=U32):
    """(hash, status) of (extranonce2, ntime, nonce, version, session) with hashlib."""
    en2, ntime, nonce, version, s = sub
    if s >= len(sessions) or en2 >> (8 * job.extranonce2_size):
        return INVALID_VERDICT
    ses = sessions[s]
    assert len(ses.extranonce1) == len(job.extranonce1)
    root = sha256d(job.coinb1 + ses.extranonce1 + en2.to_bytes(job.extranonce2_size, "big") + job.coinb2)
    for entry in job.branch:
        root = sha256d(root + entry)
    header = struct.pack("<I", version) + job.prevhash + root + struct.pack("<III", ntime, job.nbits, nonce)
    h = int.from_bytes(sha256d(header), "little")
    bt = block_target(job.nbits)
    return h, ((SHARE if h <= ses.target else 0) | (BLOCK if bt is not None and h <= bt else 0)
               | (NTIME if ntime < lo or ntime > hi else 0))


def synthetic_job(rng, pos, size1, size2, total, depth, nbits=GRID_NBITS):
    """A job of random bytes whose field (size1 + size2 bytes) starts at byte pos
    of a coinbase of total bytes, under a branch of depth entries.  Its own
    extranonce1 is random too: only its length may count."""
    return Job(rng.randbytes(pos), rng.randbytes(size1), size2, rng.randbytes(total - pos - size1 - size2),
               [rng.randbytes(32) for _ in range(depth)], rng.randbytes(32), rng.getrandbits(32), nbits,
               rng.getrandbits(32))


def synthetic_sessions(rng, size1, targets=GRID_TARGETS):
    """One session per target: extranonce1 all 0x00, all 0xFF, then random."""
    en1s = [bytes(size1), b"\xff" * size1] + [rng.randbytes(size1) for _ in range(len(targets) - 2)]
    return [PoolSession(e, t) for e, t in zip(en1s, targets)]


def random_subs(rng, size2, n, nsessions):
    """n submissions: extranonce2's ends first, then random values of it;
    adjacent submissions use different sessions."""
    top = (1 << (8 * size2)) - 1
    en2s = ([0, top] + [rng.getrandbits(8 * size2) for _ in range(n - 2)])[:n]
    start = rng.randrange(nsessions)
    step = 3 if nsessions % 3 else 1  # coprime to the table's size: every session is used
    return [(e, rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), (start + i * step) % nsessions)
            for i, e in enumerate(en2s)]


def layout_total(pos, size, length):
    """The shortest coinbase that holds the field at pos and has that length mod 64."""
    total = pos + size
    return total + (length - total) % 64


@functools.lru_cache(maxsize=None)
def layout_grid():
    """((label, job, sessions, subs, verdicts), ...) over OFFSETS x BLOCKS_BEFORE x
    SIZES1 x SIZES2 x LENGTHS: 900 jobs x 65 submissions over 7 sessions, the
    branch depth cycling through 0..2, under GRID_WINDOW."""
    rng = random.Random(0x5eed0002)
    out = []
    for off in OFFSETS:
        for pre in BLOCKS_BEFORE:
            for size1 in SIZES1:
                for size2 in SIZES2:
                    for length in LENGTHS:
                        pos = 64 * pre + off
                        job = synthetic_job(rng, pos, size1, size2, layout_total(pos, size1 + size2, length),
                                            len(out) % 3)
                        sessions = synthetic_sessions(rng, size1)
                        subs = random_subs(rng, size2, PER_JOB, len(sessions))
                        want = [verdict(job, sessions, s, *GRID_WINDOW) for s in subs]
                        out.append(((off, pre, size1, size2, length), job, sessions, subs, want))
    return tuple(out)


def ladder_case():
    """(job, sessions, subs, verdicts): one hashed submission with hash H under 29
    sessions that differ in their target only: H - 1, H, H + 1, the two extremes,
    and per 32-bit word k one above with the lower words zero, one below with the
    lower words all ones, and bit 31 of word k flipped."""
    rng = random.Random(11)
    job = synthetic_job(rng, 45, 4, 4, 120, 1)
    en1 = rng.randbytes(4)
    sub = (0x01020304, 5, 6, 7)
    H, status = verdict(job, [PoolSession(en1, 0)], sub + (0,))
    assert status == 0
    words = [(H >> (32 * k)) & U32 for k in range(8)]
    assert all(0 < w < U32 for w in words)  # every rung exists for this hash
    rungs = [(H - 1, False), (H, True), (H + 1, True), (0, False), (U256, True)]
    for k in range(8):
        rungs.append((((H >> (32 * k)) + 1) << (32 * k), True))
        rungs.append(((((H >> (32 * k)) - 1) << (32 * k)) | ((1 << (32 * k)) - 1), False))
        rungs.append((H ^ (1 << (32 * k + 31)), not words[k] >> 31))
    assert len(rungs) == 29 and all((H <= t) == s for t, s in rungs)
    sessions = [PoolSession(en1, t) for t, _ in rungs]
    subs = [sub + (s,) for s in range(len(sessions))]
    return job, sessions, subs, [(H, 1 if is_set else 0) for _, is_set in rungs]


def window_cases():
    """[(lo, hi, subs over two sessions, NTIME expected per submission)]."""
    def subs(ntimes):
        return [(7, t, 9, 10, i % 2) for i, t in enumerate(ntimes)]
    return [(1000, 2000, subs([999, 1000, 2000, 2001]), [True, False, False, True]),
            (0, U32, subs([0, 1, U32 - 1, U32]), [False] * 4),
            (0, 5, subs([0, 5, 6]), [False, False, True]),
            (5, U32, subs([4, 5, U32]), [True, False, False]),
            (2000, 1000, subs([999, 1000, 1500, 2000, 2001]), [True] * 5),   # lo > hi: every entry flagged
            (7, 7, subs([6, 7, 8]), [True, False, True])]


def invalid_case():
    """(job, three sessions, 70 submissions): session == nsessions, 2^32 - 1 and
    past the table, an extranonce2 that does not fit, and valid ones between."""
    rng = random.Random(14)
    job = synthetic_job(rng, 70, 2, 2, 150, 1)
    sessions = [PoolSession(rng.randbytes(2), U256) for _ in range(3)]
    subs = [(5, 6, 7, 8, 3), (0xffff, 1, 2, 3, 2), (5, 6, 7, 8, U32), (0x10000, 1, 2, 3, 0), (U64, 1, 2, 3, 1),
            (5, 6, 7, 8, 0), (1 << 63, 1, 2, 3, 7)] * 10
    return job, sessions, subs


def sub_array(subs):
    arr = (_lib.PoolSubmit * len(subs))()
    for a, (en2, ntime, nonce, version, session) in zip(arr, subs):
        a.extranonce2, a.ntime, a.nonce, a.version, a.session = en2, ntime, nonce, version, session
    return arr


def session_array(sessions, junk=0xA5):
    """The sessions as the C ABI takes them; the bytes of extranonce1 past the
    job's size are junk, which must not count."""
    arr = (_lib.PoolSessionStruct * len(sessions))()
    for a, s in zip(arr, sessions):
        a.extranonce1[:] = list(s.extranonce1) + [junk] * (8 - len(s.extranonce1))
        a.target[:] = list(s.target.to_bytes(32, "big"))
    return arr


def as_tuples(verdicts, n=None):
    """[(hash, status)] of a JobVerdict array; reserved must be 0."""
    rows = verdicts[:len(verdicts) if n is None else n]
    assert all(v.reserved == 0 for v in rows)
    return [(v.value, v.status) for v in rows]


def counts(want):
    return (len(want),) + tuple(sum(1 for _, s in want if s & flag) for flag in (SHARE, BLOCK, INVALID, NTIME))


def result_tuple(r):
    return r.n, r.shares, r.blocks, r.invalid, r.ntime
