"""bm_search_header_versions_hits_gpu on the GPU against hashlib, never against
the library itself.

H(i, n) = sha256d(le32(versions[i]) || header[4:76] || le32(n)) as a
little-endian 256-bit integer.  The call lists every pair (n, i) of the range
with H(i, n) <= target, ascending by (n, i), counts them exactly, and returns
the best share, the pair minimising (H >> 192, n, i).  The windows, version
lists and hashlib columns are tests/test_gpu_header_versions.py's (at most 2^16
nonces x 9 versions per window, computed once and shared); the counts asserted
beside the full lists were computed with hashlib."""
import ctypes
import functools
import io
import json
import os
import struct
import subprocess
import sys

import pytest

from conftest import ROOT
from distributed_bitcoin_minter_amd import Context, _lib, bits_to_target, version_shares
from test_gpu_header_compare import VERSION_NONCES, ladder
from test_gpu_header_versions import (GEN, GENESIS, GOLDEN, LOW, MULTI, MULTI_VERSIONS, NVERS, VERS4, VERS9, H,
                                      _other_cases, column, pairs, smallest)

pytestmark = pytest.mark.gpu

U32 = (1 << 32) - 1
U256 = (1 << 256) - 1
TOP = (2 ** 32 - 2 ** 16, U32)
CAP = 65536
MAX_CAP = _lib.BM_MAX_HEADER_HITS
ZBITS = (4, 8, 12, 16)
# pairs of LOW under VERS9[:nver] at 4, 8, 12 and 16 leading zero bits (hashlib)
LOW_COUNTS = {1: (4070, 240, 16, 0), 2: (8045, 482, 24, 0), 3: (12183, 713, 37, 1), 4: (16175, 957, 58, 2),
              5: (20220, 1192, 72, 2), 7: (28463, 1684, 103, 2), 9: (36567, 2160, 131, 3)}
TOP_COUNTS = (16195, 1087, 52, 6)      # TOP under VERS9[:4]
MULTI_COUNTS = (18563, 1185, 69, 7)    # MULTI under MULTI_VERSIONS


def zero_bits(z):
    return (1 << (256 - z)) - 1


def groups_of(nver):
    return nver // 4 + (nver % 4) // 2 + nver % 2


@functools.lru_cache(maxsize=None)
def best_of(versions, lo, hi, header=GENESIS):
    """The window's best share (h, n, i): the minimum of (h >> 192, n, i)."""
    return min(pairs(versions, lo, hi, header), key=lambda s: (s[0] >> 192, s[1], s[2]))


def expect(versions, lo, hi, target, cap=CAP, header=GENESIS):
    """What Context.search_header_versions_hits must return, from hashlib."""
    if lo > hi:
        return (0, [], (U256, U32, 0))
    hits = [s for s in pairs(versions, lo, hi, header) if s[0] <= target]  # pairs ascend in (n, i)
    return (len(hits), hits if len(hits) <= cap else None, best_of(tuple(versions), lo, hi, header))


def with_version(version, header=GENESIS):
    return struct.pack("<I", version) + header[4:]


def _raw(ctx, header, versions, lo, hi, target, buf, cap, out):
    arr = (ctypes.c_uint32 * len(versions))(*versions)
    return ctx._lib.bm_search_header_versions_hits_gpu(ctx.handle, header, arr, len(versions), lo, hi, target, buf,
                                                       cap, ctypes.byref(out) if out is not None else None)


# ---- 1. densities, every group shape ---------------------------------------------

@pytest.mark.parametrize("nver", NVERS)
def test_densities(gpu_ctx, nver):
    vs = VERS9[:nver]
    for z, count in zip(ZBITS, LOW_COUNTS[nver]):
        want = expect(vs, *LOW, zero_bits(z))
        assert want[0] == count and want[1] is not None, (nver, z)
        assert gpu_ctx.search_header_versions_hits(GENESIS, vs, *LOW, zero_bits(z), CAP) == want, (nver, z)
        st = gpu_ctx.last_stats()
        assert st.launches == groups_of(nver) and st.nonces == 65536 * nver
        assert sum(st.launch[k].nonces for k in range(st.launches)) == 65536 * nver
        # count mode
        assert gpu_ctx.search_header_versions_hits(GENESIS, vs, *LOW, zero_bits(z), 0) == (count, None if count else [],
                                                                                           want[2]), (nver, z)
    # z = 0: every pair of the window, in (n, i) order
    want = expect(vs, *LOW, U256, 65536 * nver)
    assert want[0] == 65536 * nver == len(want[1])
    assert gpu_ctx.search_header_versions_hits(GENESIS, vs, *LOW, zero_bits(0), 65536 * nver) == want
    assert gpu_ctx.last_stats().nonces == 65536 * nver


def test_order_inside_a_nonce(gpu_ctx):
    """The per-version split of nver = 4, and the nonces that hit under two or
    more of the four versions: there the order inside a nonce shows."""
    vs = VERS9[:4]
    count, hits, _ = gpu_ctx.search_header_versions_hits(GENESIS, vs, *LOW, zero_bits(8), CAP)
    assert [sum(1 for _, _, i in hits if i == k) for k in range(4)] == [240, 242, 231, 244]
    assert len({n for (_, n, _), (_, m, _) in zip(hits, hits[1:]) if n == m}) == 8
    count, hits, _ = gpu_ctx.search_header_versions_hits(GENESIS, vs, *LOW, zero_bits(4), CAP)
    assert len({n for (_, n, _), (_, m, _) in zip(hits, hits[1:]) if n == m}) == 1375
    assert all((a[1], a[2]) < (b[1], b[2]) for a, b in zip(hits, hits[1:]))
    assert hits == expect(vs, *LOW, zero_bits(4))[1]


# ---- 2. the top of the nonce space -----------------------------------------------

def test_top_window(gpu_ctx):
    assert tuple(GOLDEN["genesis_windows"]["top"]["range"]) == TOP
    vs = VERS9[:4]
    for z, count in zip(ZBITS, TOP_COUNTS):
        want = expect(vs, *TOP, zero_bits(z))
        assert want[0] == count
        assert gpu_ctx.search_header_versions_hits(GENESIS, vs, *TOP, zero_bits(z), CAP) == want, z
        # no wrap past 2^32-1: the whole window, and nothing else, is scanned
        assert gpu_ctx.last_stats().nonces == 4 * 65536


# ---- 3. the exact compare --------------------------------------------------------

def test_kth_smallest_targets(gpu_ctx):
    by_hash = smallest(VERS4, *LOW)
    assert len({h for h, _, _ in by_hash}) == len(by_hash)
    for k in (1, 2, 10, 100):
        want = expect(VERS4, *LOW, by_hash[k - 1][0])
        assert want[0] == k and sorted(want[1]) == sorted(by_hash[:k])
        assert gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, by_hash[k - 1][0]) == want, k
    hmin = by_hash[0]
    assert best_of(VERS4, *LOW) == hmin
    assert gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, hmin[0] - 1) == (0, [], hmin)


def test_hot_path_boundary(gpu_ctx):
    """T = a pair's hash with only its top 32 bits kept: that hash's top word
    equals the target's, so the filter lets it through and the full compare
    decides."""
    cols = [column(v, *LOW) for v in VERS4]
    for n, i in ((0, 0), (4200, 2), (8603, 1), (30001, 3), (65535, 2)):
        T = (cols[i][n] >> 224) << 224
        want = expect(VERS4, *LOW, T, MAX_CAP)
        assert (cols[i][n], n, i) not in want[1]
        assert gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, T, MAX_CAP) == want, (n, i)


def test_extreme_targets(gpu_ctx):
    best = best_of(VERS4, *LOW)
    assert gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, 0) == (0, [], best)
    assert gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, bytes(32)) == (0, [], best)
    want = expect(VERS4, *LOW, U256, 4 * 65536)
    assert gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, U256, 4 * 65536) == want
    assert gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, b"\xff" * 32, 0) == (4 * 65536, None, best)


@pytest.mark.parametrize("n", VERSION_NONCES)
@pytest.mark.parametrize("nver", [4, 2, 1])
def test_single_nonce_ladder(gpu_ctx, nver, n):
    """The compare ladder (tests/test_gpu_header_compare.py) of every slot's own
    hash over [n, n], the others' hashes standing where they fall.  In an
    enumeration every slot's compare shows in the list on its own, so every
    slot of every kernel (M = 4, 2, 1) decides at every rung."""
    vs = VERS4[:nver]
    hs = [H(v, n) for v in vs]
    _, bi = min((h >> 192, i) for i, h in enumerate(hs))
    for slot in range(nver):
        for name, k, T in ladder(hs[slot]):
            hits = [(h, n, i) for i, h in enumerate(hs) if h <= T]
            assert ((hs[slot], n, slot) in hits) == (T >= hs[slot])
            want = (len(hits), hits, (hs[bi], n, bi))
            assert gpu_ctx.search_header_versions_hits(GENESIS, vs, n, n, T, nver) == want, (slot, name, k)
            assert gpu_ctx.search_header_versions_hits(GENESIS, vs, n, n, T, 0)[0] == len(hits), (slot, name, k)
        assert gpu_ctx.last_stats().launches == 1


# ---- 4. agreement with the older calls on the same context -------------------------

def test_agrees_with_the_older_calls(gpu_ctx):
    for z in (8, 12):
        T = zero_bits(z)
        count, hits, best = gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, T, CAP)
        assert count == len(hits) > 0
        assert gpu_ctx.search_header_versions(GENESIS, VERS4, *LOW, T) == (True,) + hits[0]
        assert gpu_ctx.search_header_versions(GENESIS, VERS4, *LOW, 0) == (False,) + best
        for i, v in enumerate(VERS4):
            c, one, b = gpu_ctx.search_header_hits(with_version(v), *LOW, T, CAP)
            assert [(h, n) for h, n, k in hits if k == i] == one and c == len(one)
            assert (best[0] >> 192, best[1]) <= (b[0] >> 192, b[1])


# ---- 5. edges, for M = 4, 2, 1 -----------------------------------------------------

@pytest.mark.parametrize("nver", [4, 2, 1])
def test_edges_every_kernel(gpu_ctx, nver):
    vs = VERS4[:nver]
    assert gpu_ctx.search_header_versions_hits(GENESIS, vs, 5, 4, U256) == (0, [], (U256, U32, 0))
    assert gpu_ctx.last_stats().launches == 0
    assert gpu_ctx.search_header_versions_hits(GENESIS, vs, U32, 0, U256) == (0, [], (U256, U32, 0))
    for n in (0, 255, 256, U32):
        hs = [H(v, n) for v in vs]
        _, bi = min((h >> 192, i) for i, h in enumerate(hs))
        best = (hs[bi], n, bi)
        every = [(h, n, i) for i, h in enumerate(hs)]
        assert gpu_ctx.search_header_versions_hits(GENESIS, vs, n, n, U256) == (nver, every, best), n
        st = gpu_ctx.last_stats()
        assert st.launches == 1 and st.nonces == nver
        i = hs.index(min(hs))
        assert gpu_ctx.search_header_versions_hits(GENESIS, vs, n, n, min(hs)) == (1, [(hs[i], n, i)], best), n
        assert gpu_ctx.search_header_versions_hits(GENESIS, vs, n, n, min(hs) - 1) == (0, [], best), n
    # tasks are 256 nonces: what a task covers beyond the range is clipped
    want = expect(vs, 777, 1000, U256)
    assert want[0] == 224 * nver
    assert gpu_ctx.search_header_versions_hits(GENESIS, vs, 777, 1000, U256) == want
    assert gpu_ctx.last_stats().nonces == 224 * nver


def test_repeated_version(gpu_ctx):
    v, n = VERS4[1], 4200
    h = H(v, n)
    assert gpu_ctx.search_header_versions_hits(GENESIS, [v, v], n, n, h) == (2, [(h, n, 0), (h, n, 1)], (h, n, 0))
    assert gpu_ctx.search_header_versions_hits(GENESIS, [v, v], n, n, h - 1) == (0, [], (h, n, 0))
    vs = (VERS4[0], v, v, VERS4[2], v)
    want = expect(vs, 0, 4095, zero_bits(6))
    assert any(a[1] == b[1] and a[0] == b[0] and (a[2], b[2]) == (1, 2) for a, b in zip(want[1], want[1][1:]))
    assert gpu_ctx.search_header_versions_hits(GENESIS, vs, 0, 4095, zero_bits(6)) == want


@pytest.mark.parametrize("case", _other_cases(), ids=lambda c: f"{c[0][:2].hex()}-{len(c[1])}v-{c[2]}+{c[3] - c[2] + 1}")
def test_other_headers(gpu_ctx, case):
    """The shared schedule words come from header bytes 64..75: here they take
    other values than the genesis block's (random, all-zero and all-ones
    headers, ranges of at most 2^13 nonces)."""
    header, vs, lo, hi, pick = case
    nver, length = len(vs), hi - lo + 1
    assert length <= 2 ** 13
    by_hash = smallest(vs, lo, hi, 50, header)
    T = by_hash[int(pick * min(len(by_hash), 50))][0]  # one of the window's own 50 smallest pair hashes
    want = expect(vs, lo, hi, T, CAP, header)
    assert 1 <= want[0] <= 50 and want[2] == by_hash[0]
    assert gpu_ctx.search_header_versions_hits(header, vs, lo, hi, T) == want
    assert gpu_ctx.search_header_versions_hits(header, vs, lo, hi, zero_bits(3)) == expect(vs, lo, hi, zero_bits(3),
                                                                                            CAP, header)
    assert gpu_ctx.search_header_versions_hits(header, vs, lo, hi, by_hash[0][0] - 1) == (0, [], by_hash[0])
    st = gpu_ctx.last_stats()
    assert st.nonces == length * nver and st.launches == groups_of(nver)


def test_sixty_four_versions(gpu_ctx):
    vs = _lib.roll_versions(1, 64)
    every = [(H(v, n), n, i) for n in range(256) for i, v in enumerate(vs)]
    best = min(every, key=lambda s: (s[0] >> 192, s[1], s[2]))
    got = gpu_ctx.search_header_versions_hits(GENESIS, vs, 0, 255, U256)
    assert got[0] == 16384 and got == (16384, every, best)
    assert all((a[1], a[2]) < (b[1], b[2]) for a, b in zip(got[1], got[1][1:]))
    st = gpu_ctx.last_stats()
    assert st.launches == 16 and st.nonces == 16384


# ---- 6. all or nothing -------------------------------------------------------------

def test_all_or_nothing(gpu_ctx):
    vs, (lo, hi), T = VERS9[:6], LOW, zero_bits(8)
    want = expect(vs, lo, hi, T)
    count = want[0]
    assert LOW_COUNTS[5][1] < count < LOW_COUNTS[7][1]  # groups 4 + 2, hits in both
    tgt = T.to_bytes(32, "big")
    buf = (_lib.HeaderVersionHit * (count + 2))()
    ctypes.memset(buf, 0xA5, ctypes.sizeof(buf))
    before = bytes(buf)
    r = _lib.HeaderVersionsHitsResult()
    assert _raw(gpu_ctx, GENESIS, vs, lo, hi, tgt, buf, count - 1, r) == _lib.BM_OK
    assert (r.count, r.stored, r.reserved) == (count, 0, 0) and bytes(buf) == before
    best = (int.from_bytes(bytes(r.hash), "big"), r.nonce, r.version_index)
    assert best == want[2] and r.version == vs[r.version_index]
    assert gpu_ctx.search_header_versions_hits(GENESIS, vs, lo, hi, T, count - 1) == (count, None, want[2])
    r = _lib.HeaderVersionsHitsResult()
    assert _raw(gpu_ctx, GENESIS, vs, lo, hi, tgt, None, 0, r) == _lib.BM_OK  # count mode
    assert (r.count, r.stored) == (count, 0)
    assert (int.from_bytes(bytes(r.hash), "big"), r.nonce, r.version_index) == best
    # an empty range leaves the buffer alone
    assert _raw(gpu_ctx, GENESIS, vs, 5, 4, tgt, buf, count, r) == _lib.BM_OK
    assert (bytes(r.hash), r.nonce, r.version_index, r.version, r.reserved, r.count, r.stored) == \
        (b"\xff" * 32, U32, 0, vs[0], 0, 0, 0) and bytes(buf) == before
    # count == cap exactly, with the reserved words zero and the versions filled in
    assert _raw(gpu_ctx, GENESIS, vs, lo, hi, tgt, buf, count, r) == _lib.BM_OK
    assert (r.count, r.stored) == (count, count)
    assert [(int.from_bytes(bytes(e.hash), "big"), e.nonce, e.version_index, e.version, e.reserved)
            for e in buf[:count]] == [(h, n, i, vs[i], 0) for h, n, i in want[1]]
    assert bytes(buf)[count * 48:] == before[count * 48:]


def test_bad_arguments_on_a_live_context(gpu_ctx):
    r = _lib.HeaderVersionsHitsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    before = bytes(r)
    buf = (_lib.HeaderVersionHit * 4)()
    tgt = bytes(32)
    f = gpu_ctx._lib.bm_search_header_versions_hits_gpu
    arr = (ctypes.c_uint32 * 65)(*range(65))
    h, out = gpu_ctx.handle, ctypes.byref(r)
    assert f(None, GENESIS, arr, 4, 0, 1, tgt, buf, 4, out) == _lib.BM_EINVAL
    assert f(h, None, arr, 4, 0, 1, tgt, buf, 4, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, None, 4, 0, 1, tgt, buf, 4, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 4, 0, 1, None, buf, 4, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 4, 0, 1, tgt, buf, 4, None) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 0, 0, 1, tgt, buf, 4, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 65, 0, 1, tgt, buf, 4, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 4, 0, 1, tgt, None, 4, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 4, 0, 1, tgt, buf, MAX_CAP + 1, out) == _lib.BM_EINVAL
    assert bytes(r) == before and bytes(buf) == bytes(ctypes.sizeof(buf))


# ---- 7. the counter is shared by a device's launches and zeroed once ----------------

def test_counter_is_shared_and_zeroed_once(gpu_ctx):
    vs, T = VERS9[:6], zero_bits(8)
    want = expect(vs, *LOW, T)
    assert any(i < 4 for _, _, i in want[1]) and any(i >= 4 for _, _, i in want[1])  # hits in both groups
    for _ in range(3):
        assert gpu_ctx.search_header_versions_hits(GENESIS, vs, *LOW, T, CAP) == want
        assert gpu_ctx.last_stats().launches == 2
    assert gpu_ctx.search_header_versions_hits(GENESIS, vs, *LOW, T, 0) == (want[0], None, want[2])
    assert gpu_ctx.search_header_versions_hits(GENESIS, vs, *LOW, T, want[0]) == want


# ---- 8. independence from grouping and scheduling ----------------------------------

_CHILD = r"""
import json, sys
from distributed_bitcoin_minter_amd import Context
header = bytes.fromhex(sys.argv[1])
cases = json.loads(sys.argv[2])
with Context(num_gpus=1) as ctx:
    out = [ctx.search_header_versions_hits(header, vs, lo, hi, int(t, 16), cap) for vs, lo, hi, t, cap in cases]
print(json.dumps([[c, None if hits is None else [[format(h, "x"), n, i] for h, n, i in hits],
                   [format(b[0], "x"), b[1], b[2]]] for c, hits, b in out]))
"""


def _case_table():
    """(versions, lo, hi, target, cap)"""
    cases = []
    for nver in (7, 4, 3, 1):
        vs = VERS9[:nver]
        cases += [(vs, *LOW, zero_bits(4), CAP), (vs, *LOW, zero_bits(12), CAP), (vs, *LOW, 0, CAP)]
    cases.append((VERS9[:6], *LOW, zero_bits(8), 0))          # count mode
    cases.append((VERS9[:6], *LOW, zero_bits(8), 100))        # count > cap
    cases.append((VERS4, 4200, 4200, U256, CAP))
    cases.append((VERS9[:5], 777, 1000, U256, CAP))
    cases.append((VERS4, *TOP, zero_bits(12), CAP))
    return cases


@pytest.mark.parametrize("env", [{"BTCMINER_HEADER_GROUP": "1"}, {"BTCMINER_HEADER_GROUP": "2"},
                                 {"BTCMINER_HEADER_GROUP": "4"}, {"BTCMINER_CHUNK": "10", "BTCMINER_STREAMS": "1"}],
                         ids=lambda e: ",".join(f"{k[9:]}={v}" for k, v in e.items()))
def test_case_table_under_knobs(env):
    """The case table in a fresh child process per setting."""
    cases = _case_table()
    want = [expect(*c) for c in cases]
    arg = json.dumps([[list(vs), lo, hi, format(T, "x"), cap] for vs, lo, hi, T, cap in cases])
    r = subprocess.run([sys.executable, "-c", _CHILD, GENESIS.hex(), arg], capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, **env))
    assert r.returncode == 0, r.stderr
    got = [(c, None if hits is None else [(int(h, 16), n, i) for h, n, i in hits], (int(b[0], 16), b[1], b[2]))
           for c, hits, b in json.loads(r.stdout)]
    assert got == want


def test_case_table_one_block_per_cu(gpu_ctx):
    cases = _case_table()
    gpu_ctx.set_blocks_per_cu(1)
    try:
        got = [gpu_ctx.search_header_versions_hits(GENESIS, *c) for c in cases]
    finally:
        gpu_ctx.set_blocks_per_cu(0)
    assert got == [expect(*c) for c in cases]


# ---- 9. several devices on one GPU -------------------------------------------------

def _unaligned_range(ndev, shares):
    """(a, b) inside MULTI whose pieces under `shares` all begin on no multiple
    of 256, a and b themselves being hits at 8 zero bits: a hit is the first
    nonce of the first piece and another the last nonce of the last."""
    ns = sorted({n for h, n, i in pairs(MULTI_VERSIONS, *MULTI) if h <= zero_bits(8)})
    for a in ns[:20]:
        for b in ns[:-21:-1]:
            pieces = _lib.split_range(a, b, ndev, shares)
            if all(p is not None and p[0] % 256 != 0 and (p[1] + 1) % 256 != 0 for p in pieces):
                return a, b, pieces
    raise AssertionError("no such range")


@pytest.mark.parametrize("ndev", [2, 3])
def test_multi_device_on_one_gpu(gpu_ctx, ndev):
    lo, hi = MULTI
    vs = MULTI_VERSIONS
    with Context(devices=[0] * ndev) as ctx:
        def same(a, b, T, cap=CAP):
            want = expect(vs, a, b, T, cap)
            assert ctx.search_header_versions_hits(GENESIS, vs, a, b, T, cap) == want
            assert gpu_ctx.search_header_versions_hits(GENESIS, vs, a, b, T, cap) == want
            return want

        for z, count in zip(ZBITS, MULTI_COUNTS):
            want = same(lo, hi, zero_bits(z))
            assert want[0] == count
            st = ctx.last_stats()
            assert st.launches == 2 * ndev and st.combine_used == _lib.BM_COMBINED_HOST  # groups 2 + 1 per device
            assert st.nonces == (hi - lo + 1) * 3 and st.devices == ndev
        assert same(lo, hi, 0)[0] == 0
        shares = [1, 5, 2][:ndev]
        ctx.set_split(shares)
        assert same(lo, hi, zero_bits(8))[0] == MULTI_COUNTS[1]
        # a range shorter than the device count leaves a device empty
        n = lo + 5
        assert same(n, n, U256)[0] == 3
        assert ctx.last_stats().launches == 2
        assert same(n, n + 1, U256)[0] == 6
        # pieces that begin on no multiple of 256: hits at the very ends, and every pair once across the cuts
        a, b, cut = _unaligned_range(ndev, shares)
        want = same(a, b, zero_bits(8))
        assert want[1][0][1] == a == cut[0][0] and want[1][-1][1] == b == cut[-1][1]
        assert same(a, b, U256, MAX_CAP)[0] == (b - a + 1) * 3
        assert ctx.last_stats().combine_used == _lib.BM_COMBINED_HOST


# ---- 10. failure paths -------------------------------------------------------------

def test_rank_context_is_refused():
    with Context(devices=[0], rank=1, world=2) as ctx:
        with pytest.raises(_lib.BtcMinerError) as ei:
            ctx.search_header_versions_hits(GENESIS, VERS4, 0, 1000, 0)
        assert ei.value.status == _lib.BM_EINVAL
    with Context(devices=[0], rank=0, world=1) as ctx:  # a group of one is a single device
        assert ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, zero_bits(12)) == expect(VERS4, *LOW, zero_bits(12))


def test_failed_call_leaves_out_hits_and_context_alone(gpu_ctx):
    r = _lib.HeaderVersionsHitsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    buf = (_lib.HeaderVersionHit * 64)()
    ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
    before = bytes(r), bytes(buf)
    T = zero_bits(12)
    first = gpu_ctx.search_header_versions(GENESIS, VERS4, *LOW, 0)
    dispatched = gpu_ctx.last_target_stats().nonces_dispatched
    gpu_ctx.set_test_fault(0)
    try:
        rc = _raw(gpu_ctx, GENESIS, VERS4, 0, 65535, T.to_bytes(32, "big"), buf, 64, r)
        assert rc == _lib.BM_EINTERNAL
        assert (bytes(r), bytes(buf)) == before
    finally:
        gpu_ctx.set_test_fault(-1)
    want = expect(VERS4, *LOW, T)
    assert want[0] == 58
    assert gpu_ctx.search(b"bradfitz", 0, 9999) == (1419516646206828, 9898)
    assert gpu_ctx.search_header_versions(GENESIS, VERS4, *LOW, T) == (True,) + want[1][0]
    assert gpu_ctx.search_header_versions(GENESIS, VERS4, *LOW, 0) == first == (False,) + want[2]
    assert gpu_ctx.search_header_versions_hits(GENESIS, VERS4, *LOW, T) == want
    # the target stats are a first-hit search's: this call does not touch them
    assert gpu_ctx.last_target_stats().nonces_dispatched == dispatched == 4 * 65536


# ---- 11. CLI -----------------------------------------------------------------------

def test_version_shares_cli(gpu_ctx):
    versions = _lib.roll_versions(1, 4)
    count, hits, best = expect(tuple(versions), *LOW, zero_bits(12))
    own = bits_to_target(GEN["bits"])
    lines = [f"{'Block' if h <= own else 'Share'} {h:064x} {n} {versions[i]:08x}" for h, n, i in hits]
    lines.append(f"Shares {count} Best {best[0]:064x} {best[1]} {versions[best[2]]:08x}")
    assert count > 10
    argv = [GENESIS.hex(), "--versions", "4", "--zero-bits", "12", "0", "65535"]
    out = io.StringIO()
    assert version_shares.main(argv, out=out, ctx=gpu_ctx) == 0
    assert out.getvalue().splitlines() == lines
    out = io.StringIO()  # an over-full piece is halved and scanned again
    assert version_shares.main(argv + ["--cap", "4"], out=out, ctx=gpu_ctx) == 0
    assert out.getvalue().splitlines() == lines
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.version_shares", *argv],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == lines


def test_version_shares_cli_prints_the_block(gpu_ctx):
    lo, hi = GEN["nonce"] - 100, GEN["nonce"] + 100
    out = io.StringIO()
    assert version_shares.main([GENESIS.hex(), "--zero-bits", "30", str(lo), str(hi)], out=out, ctx=gpu_ctx) == 0
    assert f"Block {GEN['hash']} {GEN['nonce']} 00000001" in out.getvalue().splitlines()


# ---- 12. the whole nonce space -------------------------------------------------------

def test_full_range(gpu_ctx):
    """[0, 2^32-1] under four versions at 32 zero bits: about 0.6 s of GPU
    work.  The expected list cannot be computed here, so: every returned entry
    is a hit by hashlib, the list ascends strictly in (n, i), holds the genesis
    block, the best share is in it, and the counts agree."""
    T = zero_bits(32)
    count, hits, best = gpu_ctx.search_header_versions_hits(GENESIS, VERS4, 0, U32, T)
    st = gpu_ctx.last_stats()
    print("full range:", count, [(f"{h:064x}", n, i) for h, n, i in hits], "best", f"{best[0]:064x}", best[1:])
    assert hits is not None and count == len(hits)  # the list is read up to `stored`: count == stored == len
    assert all(H(VERS4[i], n) == h <= T for h, n, i in hits)
    assert all((a[1], a[2]) < (b[1], b[2]) for a, b in zip(hits, hits[1:]))
    assert (int(GEN["hash"], 16), GEN["nonce"], 2) in hits and GEN["nonce"] == 2083236893
    assert best in hits and all((best[0] >> 192, best[1], best[2]) <= (h >> 192, n, i) for h, n, i in hits)
    assert st.nonces == 4 * 2 ** 32 and st.launches == 1
