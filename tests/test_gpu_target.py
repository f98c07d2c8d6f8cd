"""bm_search_target_gpu on the GPU: the first nonce whose hash is <= target
(the smallest one, whatever the timing), or bm_search_gpu's answer when
there is none.  Every expected value comes from the CPU oracle or from the
committed goldens."""
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
T54 = 1 << 54  # about one hit per 1,024 nonces


def first_hit(oracle, msg, lo, hi, T):
    """First n in [lo, hi] with oracle.hash(msg, n) <= T, else None."""
    for n in range(lo, hi + 1):
        if oracle.hash(msg, n) <= T:
            return n
    return None


def window(oracle, msg, lo, hi):
    """[(hash, nonce)] of the whole window, ascending nonces."""
    return [(oracle.hash(msg, n), n) for n in range(lo, hi + 1)]


def kth_target(hs, k):
    """(T, expected nonce): T = the k-th smallest hash of the window; the
    answer is the smallest nonce among the hashes <= T."""
    T = sorted(h for h, _ in hs)[k - 1]
    return T, min(n for h, n in hs if h <= T)


def check_found(ctx, oracle, msg, lo, hi, T, nonce):
    got = ctx.search_target(msg, lo, hi, T)
    assert got == (True, oracle.hash(msg, nonce), nonce), (got, lo, hi, T)
    ts = ctx.last_target_stats()
    assert nonce - lo + 1 <= ts.nonces_dispatched <= hi - lo + 1
    return got


def check_not_found(ctx, msg, lo, hi, T, want):
    got = ctx.search_target(msg, lo, hi, T)
    assert got == (False,) + tuple(want), (got, lo, hi, T)
    assert ctx.last_target_stats().nonces_dispatched == hi - lo + 1


# ---- 1. known answer ---------------------------------------------------------

def test_known_answer(gpu_ctx, oracle):
    msg, T = b"bradfitz", 1419516646206828
    assert oracle.search(msg, 0, 9999) == (T, 9898)
    assert gpu_ctx.search_target(msg, 0, 9999, T) == (True, T, 9898)
    assert gpu_ctx.search_target(msg, 0, 9999, T - 1) == (False,) + gpu_ctx.search(msg, 0, 9999) == (False, T, 9898)
    assert gpu_ctx.search_target(msg, 0, 9999, U64) == (True, oracle.hash(msg, 0), 0)
    assert gpu_ctx.search_target(msg, 4321, 9999, U64) == (True, oracle.hash(msg, 4321), 4321)
    assert gpu_ctx.search_target(msg, 0, 9999, 0) == (False, T, 9898)
    # empty range
    assert gpu_ctx.search_target(msg, 5, 4, U64) == (False, U64, U64)
    assert gpu_ctx.last_target_stats().nonces_dispatched == 0


# ---- 2. every layout ---------------------------------------------------------

def _layout_cases():
    """One (msg, lower, upper, max_windows) per kernel layout (nbv, p), as
    tests/test_gpu_parity.py derives them with the CPU planner."""
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


def test_target_layout_table_complete():
    assert len(_LAYOUTS) == 64 + 17


@pytest.mark.parametrize("key", sorted(_LAYOUTS))
def test_every_layout(gpu_ctx, oracle, key):
    msg, lo, hi, mw = _LAYOUTS[key]
    hs = window(oracle, msg, lo, hi)
    low = min(hs)
    assert low == oracle.search(msg, lo, hi)
    gpu_ctx.set_max_windows(mw)
    try:
        for td in (0, 2):
            gpu_ctx.set_task_digits(td)
            for k in (1, 3, 10):
                if k > len(hs):
                    continue
                T, nonce = kth_target(hs, k)
                check_found(gpu_ctx, oracle, msg, lo, hi, T, nonce)
                st = gpu_ctx.last_stats()
                assert any((st.launch[i].nbv, st.launch[i].p) == key for i in range(st.recorded)), (td, k)
            if low[0] > 0:
                check_not_found(gpu_ctx, msg, lo, hi, low[0] - 1, low)
    finally:
        gpu_ctx.set_max_windows(64)
        gpu_ctx.set_task_digits(0)


# ---- 3. many racing hits -----------------------------------------------------

def _racing_cases():
    """40 (msg, lower, upper): message lengths 0..130, lowers over 1- to
    20-digit nonces, every other one placed just below a power of ten so the
    10^6 range crosses a digit-count boundary.  Seed chosen (with the oracle)
    so that every case has a hit at T54 within its first 20,000 nonces."""
    rng = random.Random(20260)
    cases = []
    for k in range(40):
        msg = bytes(rng.randrange(32, 127) for _ in range(rng.randint(0, 130)))
        D = 1 + k % 20
        dlo = 0 if D == 1 else 10 ** (D - 1)
        dhi = U64 - 10 ** 6 if D == 20 else 10 ** D - 1
        if k >= 20 and D < 20:
            lower = max(dlo, 10 ** D - rng.randint(1, 500_000))
        else:
            lower = rng.randint(dlo, dhi)
        cases.append((msg, lower, min(U64, lower + 10 ** 6)))
    return cases


def test_many_racing_hits(gpu_ctx, oracle):
    for i, (msg, lo, hi) in enumerate(_racing_cases()):
        want = first_hit(oracle, msg, lo, min(hi, lo + 19_999), T54)
        assert want is not None, ("choose another seed", i)
        gpu_ctx.set_task_digits(2 if i % 2 else 0)
        try:
            check_found(gpu_ctx, oracle, msg, lo, hi, T54, want)
        finally:
            gpu_ctx.set_task_digits(0)


# ---- 4. clipping -------------------------------------------------------------

def test_clipping(gpu_ctx, oracle):
    msg, base = b"clip the range", 1_234_000
    hs = window(oracle, msg, base, base + 9999)
    T, n0 = min(hs)
    assert sum(1 for h, _ in hs if h <= T) == 1
    lo_a, hi_a = n0 + 1, n0 + 5000
    lo_b, hi_b = n0 - 5000, n0 - 1
    min_a, min_b = oracle.search(msg, lo_a, hi_a), oracle.search(msg, lo_b, hi_b)
    # neither neighbour range holds a hit of its own, so neither may report n0
    assert min_a[0] > T and min_b[0] > T
    check_not_found(gpu_ctx, msg, lo_a, hi_a, T, min_a)
    check_not_found(gpu_ctx, msg, lo_b, hi_b, T, min_b)
    assert gpu_ctx.search_target(msg, n0, n0, T) == (True, T, n0)
    assert gpu_ctx.last_target_stats().nonces_dispatched == 1


# ---- 5. top of the range -----------------------------------------------------

def test_top_of_range(gpu_ctx, oracle):
    c3 = next(c for c in load_golden("full_range.json")["cases"] if c["config"] == "C3")
    msg = bytes.fromhex(c3["msg_hex"])
    assert len(msg) == 120
    lo, hi = U64 - 4999, U64
    hs = window(oracle, msg, lo, hi)
    T, nonce = kth_target(hs, 2)
    check_found(gpu_ctx, oracle, msg, lo, hi, T, nonce)
    low = min(hs)
    check_not_found(gpu_ctx, msg, lo, hi, low[0] - 1, low)
    # the last nonce itself: the only hit when the range is that nonce alone
    h_last = oracle.hash(msg, U64)
    assert gpu_ctx.search_target(msg, U64, U64, h_last) == (True, h_last, U64)
    assert gpu_ctx.search_target(msg, U64, U64, h_last - 1) == (False, h_last, U64)


# ---- 6. padding-block layouts ------------------------------------------------

@pytest.mark.parametrize("blocks", [0, 1, 3, 16])
def test_padding_block_layouts(gpu_ctx, oracle, blocks):
    """"msg nonce" ends at byte 64 * blocks + P with P >= 55: the generic
    kernel runs these in target mode, whatever the number of prefix blocks."""
    digits = 7
    L = 64 * blocks + 58 - 1 - digits  # the last digit lands on byte P = 57
    msg = bytes(65 + (i * 11) % 26 for i in range(L))
    lo, hi = 1_000_000, 1_004_000
    segs = plan_segments(msg, lo, hi)
    assert [(s.nbv, s.p, s.pad_block) for s in segs] == [(1, 57, 1)]
    hs = window(oracle, msg, lo, hi)
    T, nonce = kth_target(hs, 3)
    check_found(gpu_ctx, oracle, msg, lo, hi, T, nonce)
    st = gpu_ctx.last_stats()
    assert [(st.launch[i].p, st.launch[i].pad_block) for i in range(st.recorded)] == [(57, 1)]  # generic
    low = min(hs)
    check_not_found(gpu_ctx, msg, lo, hi, low[0] - 1, low)


# ---- 7. early exit is real ---------------------------------------------------

@pytest.mark.parametrize("cfg", ["C2"])
def test_early_exit_is_real(gpu_ctx, cfg):
    """bradfitz over [0, 2^32-1] with T = the committed minimum: found at
    the golden nonce (by the tie rule the first nonce at or below the minimum)
    after dispatching less than half the range.  Upper bound: the hit lies at
    0.379 of the range; the slack after it is at most one chunk per resident
    wave, 256 CUs x 4 SIMDs x <= 8 waves x 6,400 nonces = 52 M, plus the 16.8 M
    tail launch: well under 2^31."""
    c2 = next(c for c in load_golden("full_range.json")["cases"] if c["config"] == cfg)
    msg = bytes.fromhex(c2["msg_hex"])
    assert (msg, c2["lower"], c2["upper"], c2["hash"], c2["nonce"]) == (b"bradfitz", 0, 2 ** 32 - 1, 5256245051,
                                                                        1626825724)
    assert gpu_ctx.search_target(msg, 0, 2 ** 32 - 1, 5256245051) == (True, 5256245051, 1626825724)
    d = gpu_ctx.last_target_stats().nonces_dispatched
    print("dispatched", d)
    assert 1_626_825_725 <= d < 2 ** 31, d
    assert gpu_ctx.search_target(msg, 0, 2 ** 32 - 1, 5256245050) == (False, 5256245051, 1626825724)
    assert gpu_ctx.last_target_stats().nonces_dispatched == 2 ** 32


# ---- 8. multi-slot -----------------------------------------------------------

def test_multi_slot(gpu_ctx, oracle):
    msg = b"three slots"
    lo, hi = 0, 300_000
    # a) T54: hits in all three pieces
    pieces = _lib.split_range(lo, hi, 3)
    for a, b in pieces:
        assert first_hit(oracle, msg, a, min(b, a + 19_999), T54) is not None
    want_a = first_hit(oracle, msg, lo, hi, T54)
    # b) the only hits lie in the last piece: T = the minimum of the last
    # piece, a range chosen so that the first two pieces stay above it
    lo_b, hi_b = 800_000, 1_100_000
    pieces_b = _lib.split_range(lo_b, hi_b, 3)
    mins = [oracle.search(msg, a, b, threads=8) for a, b in pieces_b]
    T_b, want_b = mins[2]
    assert mins[0][0] > T_b and mins[1][0] > T_b
    with Context(devices=[0, 0, 0]) as ctx:
        for shares in (None, [1, 5, 2]):
            ctx.set_split(shares)
            assert ctx.search_target(msg, lo, hi, T54) == (True, oracle.hash(msg, want_a), want_a)
            ts = ctx.last_target_stats()
            assert ts.devices == 3 and sum(ts.dev_dispatched[:3]) == ts.nonces_dispatched >= want_a + 1
            assert ctx.search_target(msg, lo_b, hi_b, T_b) == (True, T_b, want_b)
            assert ctx.search_target(msg, lo_b, hi_b, T_b - 1) == (False,) + oracle.search(msg, lo_b, hi_b, threads=8)
            assert ctx.last_target_stats().nonces_dispatched == hi_b - lo_b + 1
            assert ctx.last_stats().combine_used == _lib.BM_COMBINED_HOST
    assert gpu_ctx.search_target(msg, lo, hi, T54) == (True, oracle.hash(msg, want_a), want_a)
    assert gpu_ctx.search_target(msg, lo_b, hi_b, T_b) == (True, T_b, want_b)


# ---- 9. isolation ------------------------------------------------------------

def test_isolation(gpu_ctx, oracle):
    msg, lo, hi = b"isolation", 99_000, 119_000
    want = first_hit(oracle, msg, lo, hi, T54)
    assert want is not None
    low = oracle.search(msg, lo, hi, threads=8)
    check_found(gpu_ctx, oracle, msg, lo, hi, T54, want)
    assert gpu_ctx.search(msg, lo, hi) == low
    # a failed call: out untouched, the context usable
    lib = gpu_ctx._lib
    r = _lib.TargetResult(11, 22, 33, 44)
    gpu_ctx.set_test_fault(0)
    try:
        rc = lib.bm_search_target_gpu(gpu_ctx.handle, msg, len(msg), lo, hi, T54, ctypes.byref(r))
        assert rc == _lib.BM_EINTERNAL
        assert (r.hash, r.nonce, r.found, r.reserved) == (11, 22, 33, 44)
        assert gpu_ctx.last_target_stats().nonces_dispatched == 0
        gpu_ctx.set_test_fault(1)  # after one launch is in flight
        with pytest.raises(_lib.BtcMinerError) as ei:
            gpu_ctx.search_target(msg, 0, hi, T54)
        assert ei.value.status == _lib.BM_EINTERNAL
    finally:
        gpu_ctx.set_test_fault(-1)
    check_found(gpu_ctx, oracle, msg, lo, hi, T54, want)
    assert gpu_ctx.search(msg, lo, hi) == low


def test_rank_context_is_refused(oracle):
    msg, lo, hi = b"ranks", 0, 20_000
    with Context(devices=[0], rank=1, world=2) as ctx:
        with pytest.raises(_lib.BtcMinerError) as ei:
            ctx.search_target(msg, lo, hi, T54)
        assert ei.value.status == _lib.BM_EINVAL
        a, b = _lib.split_range(lo, hi, 2)[1]
        assert ctx.search(msg, lo, hi) == oracle.search(msg, a, b)
    # a group of one is a single device
    with Context(devices=[0], rank=0, world=1) as ctx:
        want = first_hit(oracle, msg, lo, hi, T54)
        assert want is not None
        assert ctx.search_target(msg, lo, hi, T54) == (True, oracle.hash(msg, want), want)


# ---- 10. CLI -----------------------------------------------------------------

def test_pow_cli(oracle):
    """pow bradfitz 16 0 99999 against the oracle's first hit (2^-16 per
    nonce over 10^5 nonces: the oracle confirms one exists)."""
    want = first_hit(oracle, b"bradfitz", 0, 99_999, (1 << 48) - 1)
    assert want is not None
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.pow", "bradfitz", "16", "0", "99999"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout == f"Found {oracle.hash(b'bradfitz', want)} {want}\n"
