"""bm_search_hits_gpu on the GPU: every nonce of a range whose hash is <=
target, each exactly once and in ascending order, with the exact count and
the range's minimum.  Every expected list comes from the CPU oracle over the
whole window (or, for the one whole-range case, from the target search's
walk and the committed golden); every comparison is on the full list, so a
duplicate, an omission or an out-of-range nonce fails it."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden
from distributed_bitcoin_minter_amd import Context, _lib, plan_segments

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1
T58 = (1 << 58) - 1  # about one hit per 64 nonces
T54 = (1 << 54) - 1  # about one hit per 1,024 nonces


def window(oracle, msg, lo, hi):
    """[(hash, nonce)] of the whole window, ascending nonces (oracle_hash_many)."""
    f = oracle.lib.oracle_hash_many
    f.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                  ctypes.POINTER(ctypes.c_uint64)]
    f.restype = None
    n = hi - lo + 1
    nonces = (ctypes.c_uint64 * n)(*range(lo, hi + 1))
    out = (ctypes.c_uint64 * n)()
    f(msg, len(msg), nonces, n, out)
    return list(zip(out, range(lo, hi + 1)))


def expect(hs, T):
    """The full answer for a window: (count, hits, min)."""
    hits = [(h, n) for h, n in hs if h <= T]
    return len(hits), hits, min(hs)


def check(ctx, hs, msg, T, cap=4096):
    """One call over the whole window hs against the oracle's list."""
    lo, hi = hs[0][1], hs[-1][1]
    count, hits, low = expect(hs, T)
    got = ctx.search_hits(msg, lo, hi, T, cap)
    want = (count, hits if count <= cap else None, low)
    assert got == want, (lo, hi, T, cap, got[0], count)
    assert ctx.last_stats().nonces == hi - lo + 1
    return got


def raw(ctx, msg, lo, hi, T, cap, fill=(0xAAAA, 0xBBBB)):
    """The C call itself on a pre-filled buffer of cap + 2 entries:
    (status, (hash, nonce, count, stored), buffer as a list)."""
    out = _lib.HitsResult(11, 22, 33, 44)
    buf = (_lib.Result * (cap + 2))(*[_lib.Result(*fill) for _ in range(cap + 2)])
    rc = ctx._lib.bm_search_hits_gpu(ctx.handle, msg, len(msg), lo, hi, T, buf, cap, ctypes.byref(out))
    return rc, (out.hash, out.nonce, out.count, out.stored), [(e.hash, e.nonce) for e in buf]


# ---- 1. known answer ---------------------------------------------------------

def test_known_answer(gpu_ctx, oracle):
    msg, T = b"bradfitz", 1419516646206828
    hs = window(oracle, msg, 0, 9999)
    assert min(hs) == (T, 9898) == oracle.search(msg, 0, 9999)
    assert gpu_ctx.search_hits(msg, 0, 9999, T) == (1, [(T, 9898)], (T, 9898))
    assert gpu_ctx.last_stats().nonces == 10000
    assert gpu_ctx.search_hits(msg, 0, 9999, T - 1) == (0, [], (T, 9898))
    # every nonce a hit
    assert gpu_ctx.search_hits(msg, 0, 9999, U64, cap=10000) == (10000, hs, (T, 9898))
    # one entry short: the exact count, nothing stored, the buffer as it was
    fill = (0xAAAA, 0xBBBB)
    rc, out, buf = raw(gpu_ctx, msg, 0, 9999, U64, 9999, fill)
    assert rc == _lib.BM_OK and out == (T, 9898, 10000, 0)
    assert buf == [fill] * 10001
    assert gpu_ctx.search_hits(msg, 0, 9999, U64, cap=9999) == (10000, None, (T, 9898))
    # count mode: NULL and 0
    o = _lib.HitsResult()
    assert gpu_ctx._lib.bm_search_hits_gpu(gpu_ctx.handle, msg, len(msg), 0, 9999, U64, None, 0,
                                           ctypes.byref(o)) == _lib.BM_OK
    assert (o.hash, o.nonce, o.count, o.stored) == (T, 9898, 10000, 0)
    assert gpu_ctx.search_hits(msg, 0, 9999, T, cap=0) == (1, None, (T, 9898))
    assert gpu_ctx.search_hits(msg, 0, 9999, T - 1, cap=0) == (0, [], (T, 9898))
    # empty range
    rc, out, buf = raw(gpu_ctx, msg, 5, 4, U64, 4, fill)
    assert rc == _lib.BM_OK and out == (U64, U64, 0, 0) and buf == [fill] * 6
    assert gpu_ctx.search_hits(msg, 5, 4, U64) == (0, [], (U64, U64))
    # the argument errors on a live context
    assert raw(gpu_ctx, msg, 0, 9, U64, 0)[0] == _lib.BM_OK
    o = _lib.HitsResult(1, 2, 3, 4)
    assert gpu_ctx._lib.bm_search_hits_gpu(gpu_ctx.handle, msg, len(msg), 0, 9, U64, None, 1,
                                           ctypes.byref(o)) == _lib.BM_EINVAL
    assert (o.hash, o.nonce, o.count, o.stored) == (1, 2, 3, 4)


# ---- 2. every layout ---------------------------------------------------------

def _layout_cases():
    """One (msg, lower, upper, max_windows) per kernel layout (nbv, p), derived
    with the CPU planner as tests/test_gpu_target.py does."""
    want = {(1, p) for p in range(64)} | {(2, p) for p in range(17)}
    found = {}
    for mw in (64, 0):
        for L in range(0, 128):
            msg = bytes((97 + (i * 7) % 26) for i in range(L))
            for D in range(1, 21):
                lo = 0 if D == 1 else 10 ** (D - 1)
                top = U64 if D == 20 else 10 ** D - 1
                for start in (lo, lo + 123_457 if D > 7 else lo, max(lo, top - 3000)):
                    hi = min(start + 3000, top)
                    for s in plan_segments(msg, start, hi, max_windows=mw):
                        key = (s.nbv, s.p)
                        if key in want and key not in found:
                            found[key] = (msg, s.nonce_base + s.vlo, s.nonce_base + s.vhi, mw)
            if len(found) == len(want):
                return found
    return found


_LAYOUTS = _layout_cases()


def test_hits_layout_table_complete():
    assert len(_LAYOUTS) == 64 + 17
    assert all(hi - lo + 1 <= 3001 for _m, lo, hi, _w in _LAYOUTS.values())


@pytest.mark.parametrize("key", sorted(_LAYOUTS))
def test_every_layout(gpu_ctx, oracle, key):
    msg, lo, hi, mw = _LAYOUTS[key]
    hs = window(oracle, msg, lo, hi)
    ranked = sorted(h for h, _ in hs)
    targets = [ranked[0], ranked[min(9, len(ranked) - 1)], T58, U64]
    gpu_ctx.set_max_windows(mw)
    try:
        for td in (0, 2):
            gpu_ctx.set_task_digits(td)
            for T in targets:
                check(gpu_ctx, hs, msg, T)
                st = gpu_ctx.last_stats()
                assert any((st.launch[i].nbv, st.launch[i].p) == key for i in range(st.recorded)), (td, T)
    finally:
        gpu_ctx.set_max_windows(64)
        gpu_ctx.set_task_digits(0)


# ---- 3. digit-count boundaries -----------------------------------------------

def _boundary_cases():
    """(msg, lower, upper) for D = 1..20: 100,000 nonces around 10^D (D = 20:
    the last 100,000 nonces), random printable messages of 0..130 bytes."""
    rng = random.Random(20261)
    cases = []
    for D in range(1, 21):
        msg = bytes(rng.randrange(32, 127) for _ in range(rng.randint(0, 130)))
        if D < 20:
            cases.append((msg, max(0, 10 ** D - 50_000), 10 ** D + 49_999))
        else:
            cases.append((msg, 2 ** 64 - 100_000, 2 ** 64 - 1))
    return cases


@pytest.mark.parametrize("D", range(1, 21))
def test_digit_count_boundaries(gpu_ctx, oracle, D):
    msg, lo, hi = _boundary_cases()[D - 1]
    hs = window(oracle, msg, lo, hi)
    gpu_ctx.set_task_digits(2 if D % 2 else 0)
    try:
        count, _hits, _low = check(gpu_ctx, hs, msg, T54)
    finally:
        gpu_ctx.set_task_digits(0)
    print("D", D, "len", len(msg), "hits", count)
    assert count > 0


# ---- 4. clipping -------------------------------------------------------------

def test_clipping(gpu_ctx, oracle):
    msg, base = b"clip the range", 1_234_000
    T, n0 = min(window(oracle, msg, base, base + 9999))
    above, below = window(oracle, msg, n0 + 1, n0 + 5000), window(oracle, msg, n0 - 5000, n0 - 1)
    # neither neighbour range holds a hit of its own, so neither may report n0
    assert expect(above, T)[0] == 0 and expect(below, T)[0] == 0
    assert check(gpu_ctx, above, msg, T)[:2] == (0, [])
    assert check(gpu_ctx, below, msg, T)[:2] == (0, [])
    assert gpu_ctx.search_hits(msg, n0, n0, T) == (1, [(T, n0)], (T, n0))
    assert gpu_ctx.search_hits(msg, n0, n0, T - 1) == (0, [], (T, n0))
    # every nonce a hit: exactly the range, not the tasks that cover it
    check(gpu_ctx, above, msg, U64, cap=5000)
    check(gpu_ctx, below, msg, U64, cap=5000)


# ---- 5. top of the range -----------------------------------------------------

def test_top_of_range(gpu_ctx, oracle):
    c3 = next(c for c in load_golden("full_range.json")["cases"] if c["config"] == "C3")
    msg = bytes.fromhex(c3["msg_hex"])
    assert len(msg) == 120
    hs = window(oracle, msg, U64 - 4999, U64)
    count, hits, _low = check(gpu_ctx, hs, msg, U64, cap=5000)
    assert count == 5000 and hits[-1] == (oracle.hash(msg, U64), U64)
    second = sorted(h for h, _ in hs)[1]
    assert check(gpu_ctx, hs, msg, second)[0] == 2
    # the last nonce alone
    h_last = oracle.hash(msg, U64)
    assert gpu_ctx.search_hits(msg, U64, U64, h_last) == (1, [(h_last, U64)], (h_last, U64))
    assert gpu_ctx.search_hits(msg, U64, U64, h_last - 1) == (0, [], (h_last, U64))


# ---- 6. padding-block layouts ------------------------------------------------

@pytest.mark.parametrize("blocks", [0, 1, 3, 16])
def test_padding_block_layouts(gpu_ctx, oracle, blocks):
    """"msg nonce" ends at byte 64 * blocks + P with P >= 55: the generic
    kernel runs these in hits mode, whatever the number of prefix blocks."""
    digits = 7
    L = 64 * blocks + 58 - 1 - digits  # the last digit lands on byte P = 57
    msg = bytes(65 + (i * 11) % 26 for i in range(L))
    lo, hi = 1_000_000, 1_004_000
    segs = plan_segments(msg, lo, hi)
    assert [(s.nbv, s.p, s.pad_block) for s in segs] == [(1, 57, 1)]
    hs = window(oracle, msg, lo, hi)
    third = sorted(h for h, _ in hs)[2]
    for T in (third, T58):
        check(gpu_ctx, hs, msg, T)
        st = gpu_ctx.last_stats()
        assert [(st.launch[i].p, st.launch[i].pad_block) for i in range(st.recorded)] == [(57, 1)]  # generic
    assert gpu_ctx.search(msg, lo, hi) == min(hs)


# ---- 7. capacity -------------------------------------------------------------

def test_capacity(gpu_ctx, oracle):
    """cap 1, then 4096, then 1 on one range: the device buffer grows and is
    reused, nothing stale comes back, stored and count are right each time."""
    msg, lo, hi = b"capacity", 500_000, 559_999
    hs = window(oracle, msg, lo, hi)
    count, hits, low = expect(hs, T54)
    assert count > 8
    fill = (0xC0FFEE, 0xF00D)
    with Context(num_gpus=1) as ctx:  # a fresh context: its buffer starts small
        for cap in (1, 4096, 1):
            rc, out, buf = raw(ctx, msg, lo, hi, T54, cap, fill)
            assert rc == _lib.BM_OK
            if cap >= count:
                assert out == low + (count, count)
                assert buf[:count] == hits and buf[count:] == [fill] * (cap + 2 - count)
            else:
                assert out == low + (count, 0)
                assert buf == [fill] * (cap + 2)
        # after the full buffer: a sparser call returns its own entries only
        tenth = sorted(h for h, _ in hs)[9]
        check(ctx, hs, msg, tenth)
        sub = hs[1000:3000]
        check(ctx, sub, msg, T54)
        # exactly cap hits fit; one fewer slot does not
        n = expect(sub, T58)[0]
        assert n > 2
        check(ctx, sub, msg, T58, cap=n)
        check(ctx, sub, msg, T58, cap=n - 1)
        check(ctx, sub, msg, sorted(h for h, _ in sub)[0], cap=1)


# ---- 8. multi-slot -----------------------------------------------------------

def test_multi_slot(gpu_ctx, oracle):
    msg = b"three slots"
    small = window(oracle, msg, 0, 30_000)
    big = window(oracle, msg, 0, 300_000)
    one = gpu_ctx.search_hits(msg, 0, 300_000, T54)
    assert one == expect(big, T54)[:2] + (min(big),)
    with Context(devices=[0, 0, 0]) as ctx:
        for shares in (None, [1, 5, 2]):
            ctx.set_split(shares)
            pieces = _lib.split_range(0, 30_000, 3, shares)
            assert all(p is not None for p in pieces)
            # every nonce once across the piece boundaries
            assert ctx.search_hits(msg, 0, 30_000, U64, cap=30_001) == (30_001, small, min(small))
            assert ctx.last_stats().combine_used == _lib.BM_COMBINED_HOST
            assert ctx.search_hits(msg, 0, 30_000, U64, cap=30_000) == (30_001, None, min(small))
            assert ctx.search_hits(msg, 0, 300_000, T54) == one
            st = ctx.last_stats()
            assert st.combine_used == _lib.BM_COMBINED_HOST and st.devices == 3 and st.nonces == 300_001
            assert ctx.get_split() == (shares or [])  # balance did not learn


# ---- 9. isolation ------------------------------------------------------------

def test_isolation(gpu_ctx, oracle):
    msg, lo, hi = b"isolation", 99_000, 119_000
    hs = window(oracle, msg, lo, hi)
    count, hits, low = expect(hs, T54)
    assert count > 2
    first = hits[0]
    fill = (0xAAAA, 0xBBBB)
    check(gpu_ctx, hs, msg, T54)
    try:
        for fault, (a, b) in ((0, (lo, hi)), (1, (0, hi))):  # before any launch; with one in flight
            gpu_ctx.set_test_fault(fault)
            rc, out, buf = raw(gpu_ctx, msg, a, b, T54, 64, fill)
            assert rc == _lib.BM_EINTERNAL
            assert out == (11, 22, 33, 44) and buf == [fill] * 66
    finally:
        gpu_ctx.set_test_fault(-1)
    check(gpu_ctx, hs, msg, T54)
    assert gpu_ctx.search(msg, lo, hi) == low
    assert gpu_ctx.search_target(msg, lo, hi, T54) == (True,) + first
    # alternating: the hit counter and the target's hit word do not interfere
    for _ in range(3):
        check(gpu_ctx, hs, msg, T54)
        assert gpu_ctx.search_target(msg, lo, hi, T54) == (True,) + first
        assert gpu_ctx.search_target(msg, lo, hi, low[0] - 1) == (False,) + low
        check(gpu_ctx, hs, msg, low[0] - 1)
        check(gpu_ctx, hs, msg, U64, cap=hi - lo + 1)
        assert gpu_ctx.search(msg, lo, hi) == low


# ---- 10. rank contexts -------------------------------------------------------

def test_rank_context(oracle):
    msg, lo, hi = b"ranks", 0, 20_000
    hs = window(oracle, msg, lo, hi)
    with Context(devices=[0], rank=1, world=2) as ctx:
        with pytest.raises(_lib.BtcMinerError) as ei:
            ctx.search_hits(msg, lo, hi, T54)
        assert ei.value.status == _lib.BM_EINVAL
        a, b = _lib.split_range(lo, hi, 2)[1]
        assert ctx.search(msg, lo, hi) == min(hs[a - lo:b - lo + 1])
    # a group of one is a single device
    with Context(devices=[0], rank=0, world=1) as ctx:
        check(ctx, hs, msg, T54)


# ---- 11. whole range ---------------------------------------------------------

@pytest.mark.parametrize("cfg", ["C2"])
def test_whole_range(gpu_ctx, oracle, cfg):
    """bradfitz over [0, 2^32-1] at 24 zero bits: the tail launch, both
    streams and the ten digit segments.  The CPU cannot list these hits (about
    256: binomial, sigma 16), so the list is compared with the target search's
    walk from each hit + 1, a path already pinned to the oracle."""
    c2 = next(c for c in load_golden("full_range.json")["cases"] if c["config"] == cfg)
    msg, lo, hi = bytes.fromhex(c2["msg_hex"]), c2["lower"], c2["upper"]
    golden = (c2["hash"], c2["nonce"])
    assert (msg, lo, hi, golden) == (b"bradfitz", 0, 2 ** 32 - 1, (5256245051, 1626825724))
    T = (1 << 40) - 1
    count, hits, low = gpu_ctx.search_hits(msg, lo, hi, T, cap=4096)
    assert gpu_ctx.last_stats().nonces == 2 ** 32
    print("hits", count)
    assert low == golden
    assert hits is not None and count == len(hits)
    assert 256 - 6 * 16 <= count <= 256 + 6 * 16, count
    walk, at = [], lo
    while at <= hi:
        found, h, n = gpu_ctx.search_target(msg, at, hi, T)
        if not found:
            break
        walk.append((h, n))
        at = n + 1
    assert hits == walk
    for h, n in hits:
        assert h == oracle.hash(msg, n) <= T
    # the minimum as the target: the first hit is the golden nonce
    count, hits, low = gpu_ctx.search_hits(msg, lo, hi, golden[0], cap=4096)
    assert count == len(hits) >= 1 and hits[0] == golden == low
    assert all(h == golden[0] for h, _ in hits)


# ---- 12. CLI -----------------------------------------------------------------

def test_shares_cli(oracle):
    """shares bradfitz 16 0 199999 against the oracle's list."""
    hs = window(oracle, b"bradfitz", 0, 199_999)
    count, hits, low = expect(hs, (1 << 48) - 1)
    assert count == 4 and {91989, 98985, 103006} < {n for _, n in hits}
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.shares", "bradfitz", "16", "0",
                        "199999"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr
    want = "".join(f"Share {h} {n}\n" for h, n in hits) + f"Shares 4 Min {low[0]} {low[1]}\n"
    assert r.stdout == want
