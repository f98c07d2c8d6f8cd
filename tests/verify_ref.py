"""The share verifier's reference and cases, shared by the CPU and the GPU tests
of bm_job_verify_cpu / bm_job_verify_gpu: hashlib only.  A verdict is rebuilt
here from the job's pieces (coinbase, branch fold, field order); neither entry
of the library is the other's reference.  Every grid is built once per process
and left unchanged."""
import functools
import hashlib
import random
import struct

from distributed_bitcoin_minter_amd import Job, _lib

U32 = (1 << 32) - 1
U64 = (1 << 64) - 1
U256 = (1 << 256) - 1
SHARE, BLOCK, INVALID = 1, 2, 4
INVALID_VERDICT = (U256, INVALID)

# extranonce2's byte offset in the coinbase mod 64 (each with 0 and 2 whole
# blocks before it), its size, and the coinbase's total length mod 64
OFFSETS = (0, 1, 3, 56, 57, 60, 61, 63)
BLOCKS_BEFORE = (0, 2)
SIZES = (1, 2, 4, 7, 8)
LENGTHS = (55, 56, 63, 0, 1)
PER_JOB = 65
GRID_TARGET = 1 << 255        # about half of the hashes are shares
GRID_NBITS = 0x2000ffff       # the block target 0xffff << 232: about one hash in 256


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def block_target(nbits):
    """Bitcoin's compact target restated (None: negative or over 256 bits)."""
    mant, exp = nbits & 0x7fffff, nbits >> 24
    if nbits & 0x800000:
        return None
    t = mant >> (8 * (3 - exp)) if exp < 3 else mant << (8 * (exp - 3))
    return t if t <= U256 else None


def verdict(job, target, sub):
    """(hash, status) of (extranonce2, ntime, nonce, version) with hashlib."""
    en2, ntime, nonce, version = sub
    if en2 >> (8 * job.extranonce2_size):
        return INVALID_VERDICT
    root = sha256d(job.coinb1 + job.extranonce1 + en2.to_bytes(job.extranonce2_size, "big") + job.coinb2)
    for entry in job.branch:
        root = sha256d(root + entry)
    header = struct.pack("<I", version) + job.prevhash + root + struct.pack("<III", ntime, job.nbits, nonce)
    h = int.from_bytes(sha256d(header), "little")
    bt = block_target(job.nbits)
    return h, (SHARE if h <= target else 0) | (BLOCK if bt is not None and h <= bt else 0)


def synthetic_job(rng, pos, size, total, depth, nbits=GRID_NBITS):
    """A job of random bytes whose extranonce2 (size bytes) starts at byte pos
    of a coinbase of total bytes, under a branch of depth entries."""
    en1_len = min(pos, 4)
    return Job(rng.randbytes(pos - en1_len), rng.randbytes(en1_len), size, rng.randbytes(total - pos - size),
               [rng.randbytes(32) for _ in range(depth)], rng.randbytes(32), rng.getrandbits(32), nbits,
               rng.getrandbits(32))


def random_subs(rng, size, n):
    """n submissions: the field's ends first, then random values of it."""
    top = (1 << (8 * size)) - 1
    en2s = [0, top] + [rng.getrandbits(8 * size) for _ in range(n - 2)]
    return [(e, rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32)) for e in en2s[:n]]


def layout_total(pos, size, length):
    """The shortest coinbase that holds extranonce2 at pos and has that length mod 64."""
    total = pos + size
    return total + (length - total) % 64


@functools.lru_cache(maxsize=None)
def layout_grid():
    """((label, job, subs, verdicts), ...) over OFFSETS x BLOCKS_BEFORE x SIZES x
    LENGTHS: 400 jobs x 65 submissions, the branch depth cycling through 0..2."""
    rng = random.Random(0x5eed0001)
    out = []
    for off in OFFSETS:
        for pre in BLOCKS_BEFORE:
            for size in SIZES:
                for length in LENGTHS:
                    pos = 64 * pre + off
                    job = synthetic_job(rng, pos, size, layout_total(pos, size, length), len(out) % 3)
                    subs = random_subs(rng, size, PER_JOB)
                    out.append(((off, pre, size, length), job, subs, [verdict(job, GRID_TARGET, s) for s in subs]))
    return tuple(out)


def sub_array(subs):
    arr = (_lib.JobSubmit * len(subs))()
    for a, (en2, ntime, nonce, version) in zip(arr, subs):
        a.extranonce2, a.ntime, a.nonce, a.version = en2, ntime, nonce, version
        a.reserved = 0xDEADBEEF  # ignored
    return arr


def as_tuples(verdicts, n=None):
    """[(hash, status)] of a JobVerdict array; reserved must be 0."""
    rows = verdicts[:len(verdicts) if n is None else n]
    assert all(v.reserved == 0 for v in rows)
    return [(v.value, v.status) for v in rows]


def counts(want):
    return (len(want), sum(1 for _, s in want if s & SHARE), sum(1 for _, s in want if s & BLOCK),
            sum(1 for _, s in want if s & INVALID))


def result_tuple(r):
    return r.n, r.shares, r.blocks, r.invalid
