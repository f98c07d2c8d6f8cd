"""bm_search_header_hits_gpu on the GPU against hashlib: every nonce of a range
with H(n) <= target, and the range's best share.

H(n) = sha256d(header[0:76] || le32(n)) as a little-endian 256-bit integer.
Every CPU window stays at or below 2^17 nonces, computed once per window and
shared (with tests/test_gpu_header.py's, whose windows these are).  Every
comparison is on the whole list."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, U64
from distributed_bitcoin_minter_amd import Context, _lib
from test_gpu_header import GENESIS, GOLDEN, H, window

pytestmark = pytest.mark.gpu

U32 = (1 << 32) - 1
U256 = (1 << 256) - 1
LOW = (0, 65535)
TOP = (2 ** 32 - 2 ** 16, U32)
CAP = 65536


def zero_bits(z):
    return (1 << (256 - z)) - 1


def expect(header, lo, hi, target, cap=CAP):
    """What search_header_hits must return, from hashlib."""
    w = window(header, lo, hi)
    hits = [(h, n) for h, n in w if h <= target]
    _, n = min((h >> 192, n) for h, n in w)
    return len(hits), hits if len(hits) <= cap else None, (H(header, n), n)


def check(ctx, header, lo, hi, target, single=None):
    """The enumeration against hashlib and, with `single` (a one-device
    context), against the header search: hits[0] is what search_header finds
    at the same target, the best share its answer at target 0."""
    want = expect(header, lo, hi, target)
    got = ctx.search_header_hits(header, lo, hi, target, CAP)
    assert got == want, (lo, hi, hex(target), got[0], want[0])
    assert ctx.search_header_hits(header, lo, hi, target, 0)[0] == want[0]  # count mode
    if single is not None:
        first = single.search_header(header, lo, hi, target)
        assert first == ((True,) + want[1][0] if want[1] else (False,) + want[2])
        assert single.search_header(header, lo, hi, 0) == (False,) + want[2]
    return want


# ---- 1. densities --------------------------------------------------------------

@pytest.mark.parametrize("win,counts", [(LOW, (65536, 4138, 231, 13, 1)), (TOP, (65536, 4075, 275, 11, 1))],
                         ids=["low", "top"])
def test_densities(gpu_ctx, win, counts):
    for z, count in zip((0, 4, 8, 12, 16), counts):
        want = check(gpu_ctx, GENESIS, *win, zero_bits(z), single=gpu_ctx)
        assert want[0] == count, (z, want[0])
    # nothing wraps past 2^32-1: the window, and nothing else, was scanned
    gpu_ctx.search_header_hits(GENESIS, *win, zero_bits(12), CAP)
    st = gpu_ctx.last_stats()
    assert st.nonces == 65536 and st.launches == 1 and st.launch[0].nonces == 65536


# ---- 2. the exact 256-bit compare ------------------------------------------------

def test_kth_smallest_targets(gpu_ctx):
    by_hash = sorted(window(GENESIS, *LOW))
    for k in (1, 2, 10, 100):
        assert check(gpu_ctx, GENESIS, *LOW, by_hash[k - 1][0], single=gpu_ctx)[0] == k
    assert check(gpu_ctx, GENESIS, *LOW, by_hash[0][0] - 1, single=gpu_ctx)[0] == 0


def test_hot_path_boundary(gpu_ctx):
    """T = H(n) with only its top 32 bits kept: the top words are equal and
    the low words decide."""
    w = window(GENESIS, *LOW)
    for n in (0, 4200, 8603, 30001, 65535):
        T = (w[n][0] >> 224) << 224
        want = check(gpu_ctx, GENESIS, *LOW, T, single=gpu_ctx)
        assert (w[n][0], n) not in want[1]  # H(n) itself has low bits set


def test_extreme_targets(gpu_ctx):
    assert check(gpu_ctx, GENESIS, *LOW, 0, single=gpu_ctx)[0] == 0
    assert check(gpu_ctx, GENESIS, *LOW, U256, single=gpu_ctx)[0] == 65536


# ---- 3. task and chunk edges -----------------------------------------------------

def test_single_nonces_and_a_short_range(gpu_ctx):
    for n in (0, 255, 256, 8603, U32):
        h = H(GENESIS, n)
        assert gpu_ctx.search_header_hits(GENESIS, n, n, h) == (1, [(h, n)], (h, n))
        assert gpu_ctx.search_header_hits(GENESIS, n, n, h - 1) == (0, [], (h, n))
        assert gpu_ctx.search_header_hits(GENESIS, n, n, U256) == (1, [(h, n)], (h, n))
    # tasks of 256 nonces over-cover [777, 1000]: nothing outside it counts
    assert check(gpu_ctx, GENESIS, 777, 1000, U256)[0] == 224
    check(gpu_ctx, GENESIS, 777, 1000, sorted(window(GENESIS, 777, 1000))[3][0])


def _random_cases():
    rng = random.Random(0x5A4E)
    cases = []
    for i in range(26):
        header = GENESIS if i < 6 else bytes(rng.getrandbits(8) for _ in range(80))
        length = [1, 2, 255, 256, 257, 70000][i] if i < 6 else rng.randint(1, 70000)
        lo = rng.choice([0, U32 - length + 1]) if i % 7 == 6 else rng.randint(0, U32 - length + 1)
        cases.append((header, lo, lo + length - 1, rng.random()))
    return cases


@pytest.mark.parametrize("case", _random_cases(), ids=lambda c: f"{c[1]}+{c[2] - c[1] + 1}")
def test_random_ranges(gpu_ctx, case):
    header, lo, hi, pick = case
    by_hash = sorted(window(header, lo, hi))
    T = by_hash[int(pick * min(len(by_hash), 50))][0]  # one of the window's own 50 smallest hashes
    check(gpu_ctx, header, lo, hi, T)
    assert check(gpu_ctx, header, lo, hi, U256)[0] == hi - lo + 1
    assert gpu_ctx.last_stats().nonces == hi - lo + 1


# ---- 4. all or nothing -----------------------------------------------------------

def _raw(ctx, header, lo, hi, target, buf, cap, out):
    return ctx._lib.bm_search_header_hits_gpu(ctx.handle, header, lo, hi, target, buf, cap,
                                              ctypes.byref(out) if out is not None else None)


def test_all_or_nothing(gpu_ctx):
    lo, hi, ones = 0, 9999, b"\xff" * 32
    want = expect(GENESIS, *LOW, U256)
    assert gpu_ctx.search_header_hits(GENESIS, lo, hi, U256, 10000) == (10000, want[1][:10000], min(
        want[1][:10000], key=lambda s: (s[0] >> 192, s[1])))
    cap = 9999
    buf = (_lib.HeaderHit * (cap + 2))()
    ctypes.memset(buf, 0xA5, ctypes.sizeof(buf))
    before = bytes(buf)
    r = _lib.HeaderHitsResult()
    assert _raw(gpu_ctx, GENESIS, lo, hi, ones, buf, cap, r) == _lib.BM_OK
    assert (r.count, r.stored, r.reserved) == (10000, 0, 0) and bytes(buf) == before
    best = (int.from_bytes(bytes(r.hash), "big"), r.nonce)
    r = _lib.HeaderHitsResult()
    assert _raw(gpu_ctx, GENESIS, lo, hi, ones, None, 0, r) == _lib.BM_OK  # count mode
    assert (r.count, r.stored) == (10000, 0) and (int.from_bytes(bytes(r.hash), "big"), r.nonce) == best
    # an empty range leaves the buffer alone
    assert _raw(gpu_ctx, GENESIS, 5, 4, ones, buf, cap, r) == _lib.BM_OK
    assert (bytes(r.hash), r.nonce, r.reserved, r.count, r.stored) == (ones, U32, 0, 0, 0) and bytes(buf) == before
    assert gpu_ctx.search_header_hits(GENESIS, U32, 0, U256) == (0, [], (U256, U32))
    # count == cap exactly, with the reserved words zero
    assert _raw(gpu_ctx, GENESIS, lo, hi, ones, buf, 10000, r) == _lib.BM_OK
    assert (r.count, r.stored) == (10000, 10000)
    assert [(int.from_bytes(bytes(e.hash), "big"), e.nonce, e.reserved) for e in buf[:10000]] == [
        (h, n, 0) for h, n in want[1][:10000]]
    assert bytes(buf)[10000 * 40:] == before[10000 * 40:]


def test_bad_arguments_on_a_live_context(gpu_ctx):
    r = _lib.HeaderHitsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    before = bytes(r)
    buf = (_lib.HeaderHit * 4)()
    tgt = bytes(32)
    assert _raw(gpu_ctx, None, 0, 1, tgt, buf, 4, r) == _lib.BM_EINVAL
    assert _raw(gpu_ctx, GENESIS, 0, 1, None, buf, 4, r) == _lib.BM_EINVAL
    assert _raw(gpu_ctx, GENESIS, 0, 1, tgt, buf, 4, None) == _lib.BM_EINVAL
    assert _raw(gpu_ctx, GENESIS, 0, 1, tgt, None, 4, r) == _lib.BM_EINVAL
    assert _raw(gpu_ctx, GENESIS, 0, 1, tgt, buf, _lib.BM_MAX_HEADER_HITS + 1, r) == _lib.BM_EINVAL
    assert gpu_ctx._lib.bm_search_header_hits_gpu(None, GENESIS, 0, 1, tgt, buf, 4, ctypes.byref(r)) == _lib.BM_EINVAL
    assert bytes(r) == before and bytes(buf) == bytes(ctypes.sizeof(buf))


# ---- 6. independence from scheduling ---------------------------------------------

SCHED_CASES = [(0, 65535, zero_bits(4)), (0, 65535, 0)]  # one dense, one with no hit

_CHILD = r"""
import json, sys
from distributed_bitcoin_minter_amd import Context
header = bytes.fromhex(sys.argv[1])
cases = json.loads(sys.argv[2])
with Context(num_gpus=1) as ctx:
    out = [ctx.search_header_hits(header, lo, hi, int(t, 16), 65536) for lo, hi, t in cases]
print(json.dumps([[c, [[format(h, "x"), n] for h, n in hits], [format(b[0], "x"), b[1]]] for c, hits, b in out]))
"""


def test_scheduling_does_not_matter(gpu_ctx):
    want = [expect(GENESIS, lo, hi, T) for lo, hi, T in SCHED_CASES]
    assert want[0][0] == 4138 and want[1][0] == 0
    gpu_ctx.set_blocks_per_cu(1)
    try:
        assert [gpu_ctx.search_header_hits(GENESIS, lo, hi, T, CAP) for lo, hi, T in SCHED_CASES] == want
    finally:
        gpu_ctx.set_blocks_per_cu(0)
    env = dict(os.environ, PYTHONPATH=ROOT, BTCMINER_CHUNK="10", BTCMINER_STREAMS="1")
    cases = json.dumps([[lo, hi, format(T, "x")] for lo, hi, T in SCHED_CASES])
    r = subprocess.run([sys.executable, "-c", _CHILD, GENESIS.hex(), cases], capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr
    got = [(c, [(int(h, 16), n) for h, n in hits], (int(b[0], 16), b[1])) for c, hits, b in json.loads(r.stdout)]
    assert got == want


# ---- 7. several devices on one GPU -----------------------------------------------

MULTI = (393216, 393216 + 3 * 2 ** 15 - 1)


@pytest.mark.parametrize("ndev", [2, 3])
def test_multi_device_on_one_gpu(gpu_ctx, ndev):
    lo, hi = MULTI
    w = window(GENESIS, lo, hi)
    pieces = _lib.split_range(lo, hi, ndev)
    with Context(devices=[0] * ndev) as ctx:
        def same(a, b, T):
            want = expect(GENESIS, a, b, T)
            assert ctx.search_header_hits(GENESIS, a, b, T, CAP) == want
            assert gpu_ctx.search_header_hits(GENESIS, a, b, T, CAP) == want
            return want

        # hits in every piece
        T = sorted(w)[300][0]
        want = same(lo, hi, T)
        assert all(any(a <= n <= b for _, n in want[1]) for a, b in pieces)
        st = ctx.last_stats()
        assert st.launches == ndev and st.combine_used == _lib.BM_COMBINED_HOST and st.nonces == hi - lo + 1
        # in one piece only: the last piece's minimum, when no earlier piece reaches it
        for k, (a, b) in enumerate(pieces):
            T = min(h for h, n in w if a <= n <= b)
            want = same(lo, hi, T)
            if all(a <= n <= b for _, n in want[1]):
                break
        else:
            pytest.fail("no target leaves hits in one piece only")
        # in none
        assert same(lo, hi, 0)[0] == 0
        ctx.set_split([1, 5, 2][:ndev])
        same(lo, hi, sorted(w)[300][0])
        assert ctx.last_stats().launches == ndev
        # a range shorter than the device count leaves a device empty
        same(8603, 8603, U256)
        assert ctx.last_stats().launches == 1


# ---- 8. shared buffers -----------------------------------------------------------

def test_enumerations_share_one_buffer():
    """The two enumerations use one counter and one buffer per device, which
    grows between them; the searches around them are unaffected."""
    msg_hits = [(int.from_bytes(hashlib.sha256(b"bradfitz %d" % n).digest()[:8], "big"), n) for n in range(10000)]
    with Context(num_gpus=1) as ctx:
        assert ctx.search_header_hits(GENESIS, *LOW, zero_bits(12), 16) == expect(GENESIS, *LOW, zero_bits(12), 16)
        assert ctx.search_hits(b"bradfitz", 0, 9999, U64, cap=10000) == (10000, msg_hits, min(msg_hits))
        assert ctx.search_header_hits(GENESIS, *LOW, U256, 65536) == expect(GENESIS, *LOW, U256)
        assert ctx.search_header(GENESIS, *LOW, zero_bits(12)) == (True, H(GENESIS, 4200), 4200)
        assert ctx.search(b"bradfitz", 0, 9999) == (1419516646206828, 9898)
        # count > cap with a smaller cap than the buffer now holds
        assert ctx.search_header_hits(GENESIS, *LOW, zero_bits(12), 12) == (13, None, (H(GENESIS, 8603), 8603))


# ---- 9. failure paths ------------------------------------------------------------

def test_failed_call_leaves_out_hits_and_context_alone(gpu_ctx):
    r = _lib.HeaderHitsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    buf = (_lib.HeaderHit * 64)()
    ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
    before = bytes(r), bytes(buf)
    gpu_ctx.search_header(GENESIS, *LOW, 0)
    dispatched = gpu_ctx.last_target_stats().nonces_dispatched
    gpu_ctx.set_test_fault(0)
    try:
        rc = _raw(gpu_ctx, GENESIS, 0, 65535, zero_bits(12).to_bytes(32, "big"), buf, 64, r)
        assert rc == _lib.BM_EINTERNAL
        assert (bytes(r), bytes(buf)) == before
    finally:
        gpu_ctx.set_test_fault(-1)
    assert gpu_ctx.last_target_stats().nonces_dispatched == dispatched == 65536  # not this call's to touch
    assert gpu_ctx.search(b"bradfitz", 0, 9999) == (1419516646206828, 9898)
    assert gpu_ctx.search_header(GENESIS, *LOW, zero_bits(12)) == (True, H(GENESIS, 4200), 4200)
    assert gpu_ctx.search_header_hits(GENESIS, *LOW, zero_bits(12)) == expect(GENESIS, *LOW, zero_bits(12))


def test_rank_context_is_refused():
    with Context(devices=[0], rank=1, world=2) as ctx:
        with pytest.raises(_lib.BtcMinerError) as ei:
            ctx.search_header_hits(GENESIS, 0, 1000, 0)
        assert ei.value.status == _lib.BM_EINVAL
    with Context(devices=[0], rank=0, world=1) as ctx:  # a group of one is a single device
        assert ctx.search_header_hits(GENESIS, *LOW, zero_bits(12)) == expect(GENESIS, *LOW, zero_bits(12))


# ---- 10. CLI ---------------------------------------------------------------------

def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.header_shares", *args],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_header_shares_cli():
    ntime = int.from_bytes(GENESIS[68:72], "little")
    want = expect(GENESIS, *LOW, zero_bits(12))
    lines = _cli(GENESIS.hex(), "--zero-bits", "12", "0", "65535")
    assert lines[:-1] == [f"Share {h:064x} {ntime} {n}" for h, n in want[1]]
    assert len(lines) == 14 and lines[0].split()[3] == "4200"
    assert lines[-1] == f"Shares 13 Best {want[2][0]:064x} {ntime} {want[2][1]}"


def test_header_shares_cli_prints_the_block():
    g = next(g for g in GOLDEN["headers"] if g["name"] == "genesis")
    ntime = int.from_bytes(GENESIS[68:72], "little")
    lo, hi = g["nonce"] - 30000, g["nonce"] + 30000
    want = expect(GENESIS, lo, hi, zero_bits(12))
    lines = _cli(GENESIS.hex(), "--zero-bits", "12", str(lo), str(hi))
    block = f"Block {g['hash']} {ntime} {g['nonce']}"
    assert lines[:-1] == [("Block" if n == g["nonce"] else "Share") + f" {h:064x} {ntime} {n}" for h, n in want[1]]
    assert block in lines and lines[-1] == f"Shares {want[0]} Best {g['hash']} {ntime} {g['nonce']}"
