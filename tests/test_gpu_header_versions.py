"""bm_search_header_versions_gpu on the GPU against hashlib, never against the
library itself.

H(i, n) = sha256d(le32(versions[i]) || header[4:76] || le32(n)) as a
little-endian 256-bit integer.  found: the pair minimising (n, i) among the
hits; not found: the pair minimising (H >> 192, n, i).  Every hashlib window
holds at most 2^16 nonces and 9 versions (the multi-device window the issue
asks for, 3 * 2^15 nonces, holds 3), computed once and shared.  H, column,
pairs, smallest and expect take the genesis header unless given another
(test_other_headers: at most 5 * 2^13 pairs per case)."""
import ctypes
import functools
import hashlib
import heapq
import io
import json
import os
import random
import struct
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden
from distributed_bitcoin_minter_amd import Context, _lib, bits_to_target, mine_versions

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("header_vectors.json")
GEN = next(g for g in GOLDEN["headers"] if g["name"] == "genesis")
GENESIS = bytes.fromhex(GEN["header"])
U32 = (1 << 32) - 1
U256 = (1 << 256) - 1
VERS4 = (0x20000000, 0x20002000, 1, 0x3fffe000)  # index 2 is the genesis block's own version
VERS9 = VERS4 + (0, 0xffffffff, 2, 0x20004000, 0x1fffe000)
LOW = (0, 65535)
NVERS = (1, 2, 3, 4, 5, 7, 9)  # groups 1, 2, 2+1, 4, 4+1, 4+2+1, 4+4+1


def H(version: int, nonce: int, header: bytes = GENESIS) -> int:
    d = hashlib.sha256(struct.pack("<I", version) + header[4:76] + struct.pack("<I", nonce)).digest()
    return int.from_bytes(hashlib.sha256(d).digest(), "little")


@functools.lru_cache(maxsize=None)
def column(version: int, lo: int, hi: int, header: bytes = GENESIS):
    """(H(version, n)) for n in [lo, hi], computed once and never changed (a
    piece of the genesis header's LOW is cut from LOW's)."""
    if header == GENESIS and (lo, hi) != LOW and LOW[0] <= lo and hi <= LOW[1]:
        return column(version, *LOW)[lo:hi + 1]
    return tuple(H(version, n, header) for n in range(lo, hi + 1))


def pairs(versions, lo, hi, header: bytes = GENESIS):
    """Every (h, n, i) of the window, in (n, i) order."""
    cols = [column(v, lo, hi) if header == GENESIS else column(v, lo, hi, header) for v in versions]
    return [(cols[i][n - lo], n, i) for n in range(lo, hi + 1) for i in range(len(versions))]


@functools.lru_cache(maxsize=None)
def smallest(versions, lo, hi, count=100, header: bytes = GENESIS):
    """The window's `count` smallest (h, n, i), ascending."""
    return tuple(heapq.nsmallest(count, pairs(versions, lo, hi, header)))


@functools.lru_cache(maxsize=None)
def expect(versions, lo, hi, target, header: bytes = GENESIS):
    """What bm_search_header_versions_gpu must return, from hashlib."""
    p = pairs(versions, lo, hi, header)
    hit = next(((True, h, n, i) for h, n, i in p if h <= target), None)  # p ascends in (n, i)
    if hit is not None:
        return hit
    _, n, i = min((h >> 192, n, i) for h, n, i in p)
    return (False, H(versions[i], n, header), n, i)


# ---- 1. known answer ---------------------------------------------------------

def test_known_answer_genesis(gpu_ctx):
    lo, hi = GEN["nonce"] - 2 ** 15, GEN["nonce"] + 2 ** 15 - 1
    target = bits_to_target(GEN["bits"])
    want = (True, int(GEN["hash"], 16), GEN["nonce"], 2)
    assert expect(VERS4, lo, hi, target) == want
    assert gpu_ctx.search_header_versions(GENESIS, VERS4, lo, hi, target) == want
    # bytes 0..3 and 76..79 of the caller's header are ignored
    other = b"\xde\xad\xbe\xef" + GENESIS[4:76] + b"\x00\x00\x00\x00"
    assert gpu_ctx.search_header_versions(other, list(VERS4), lo, hi, target.to_bytes(32, "big")) == want
    r = _lib.HeaderVersionsResult()
    arr = (ctypes.c_uint32 * 4)(*VERS4)
    assert gpu_ctx._lib.bm_search_header_versions_gpu(gpu_ctx.handle, GENESIS, arr, 4, lo, hi,
                                                      target.to_bytes(32, "big"), ctypes.byref(r)) == _lib.BM_OK
    assert (r.found, r.nonce, r.version_index, r.version) == (1, GEN["nonce"], 2, 1)
    assert bytes(r.hash).hex() == GEN["hash"]


# ---- 2. every group size -----------------------------------------------------

def group_cases():
    """(versions, lo, hi, target) over LOW for every nver: T the k-th smallest
    hash of the window's own pairs, and one below the minimum."""
    cases = []
    for nver in NVERS:
        vs = VERS9[:nver]
        by_hash = smallest(vs, *LOW)
        for k in (1, 2, 10, 100):
            cases.append((vs, *LOW, by_hash[k - 1][0]))
        cases.append((vs, *LOW, by_hash[0][0] - 1))
    return cases


@pytest.mark.parametrize("nver", NVERS)
def test_group_sizes(gpu_ctx, nver):
    vs = VERS9[:nver]
    by_hash = smallest(vs, *LOW)
    for k in (1, 2, 10, 100):
        T = by_hash[k - 1][0]
        n, i, h = min((n, i, h) for h, n, i in by_hash[:k])
        assert expect(vs, *LOW, T) == (True, h, n, i)
        assert gpu_ctx.search_header_versions(GENESIS, vs, *LOW, T) == (True, h, n, i), (nver, k)
    hmin = by_hash[0][0]
    want = expect(vs, *LOW, hmin - 1)
    assert not want[0] and want[1] == hmin
    assert gpu_ctx.search_header_versions(GENESIS, vs, *LOW, hmin - 1) == want
    assert gpu_ctx.last_target_stats().nonces_dispatched == 65536 * nver
    st = gpu_ctx.last_stats()
    groups = nver // 4 + (nver % 4) // 2 + nver % 2
    assert st.launches == groups and st.nonces == 65536 * nver
    assert sum(st.launch[k].nonces for k in range(groups)) == 65536 * nver


# ---- 3. ties -----------------------------------------------------------------

def test_ties(gpu_ctx):
    n = 4200
    hs = [H(v, n) for v in VERS4]
    assert gpu_ctx.search_header_versions(GENESIS, VERS4, n, n, U256) == (True, hs[0], n, 0)
    # a repeated version loses the tie to its first occurrence
    v = VERS4[1]
    assert gpu_ctx.search_header_versions(GENESIS, [v, v], n, n, hs[1]) == (True, hs[1], n, 0)
    assert gpu_ctx.search_header_versions(GENESIS, [v, v], n, n, hs[1] - 1) == (False, hs[1], n, 0)
    assert gpu_ctx.search_header_versions(GENESIS, [VERS4[0], v, v, v, v], *LOW, U256) == (True, H(VERS4[0], 0), 0, 0)
    # T = the smallest hash at that nonce: only that slot hits
    for n in (4200, 4201, 4202, 4203, 65535):
        hs = [H(v, n) for v in VERS4]
        i = hs.index(min(hs))
        assert gpu_ctx.search_header_versions(GENESIS, VERS4, n, n, hs[i]) == (True, hs[i], n, i)
    assert len({[H(v, n) for v in VERS4].index(min(H(v, n) for v in VERS4)) for n in (4200, 4201, 4202, 4203, 65535)}) > 1


# ---- 4. the hit word is shared by a device's group launches -------------------

@functools.lru_cache(maxsize=None)
def _cross_case(first_group_wins: bool):
    """(lo, hi, T, want) over 6 versions (groups 0..3 and 4..5) such that the
    range's only hits at T are one pair of indices 4..5 at nonce a and one of
    indices 0..3 at nonce b, with b < a (first_group_wins) or a < b."""
    vs = VERS9[:6]
    by_hash = smallest(vs, *LOW, 150)
    best = None
    for x in range(len(by_hash)):
        for y in range(x):  # by_hash[y] < by_hash[x]: T = by_hash[x]'s hash
            (hx, nx, ix), (hy, ny, iy) = by_hash[x], by_hash[y]
            if (ix < 4) == (iy < 4) or nx == ny:
                continue
            (na, ia), (nb, ib) = ((nx, ix), (ny, iy)) if ix >= 4 else ((ny, iy), (nx, ix))  # a: indices 4..5
            if (nb < na) != first_group_wins:
                continue
            lo, hi = min(na, nb), max(na, nb)
            if sum(1 for h, n, i in by_hash[:x + 1] if lo <= n <= hi) != 2:
                continue  # another hit inside
            # widen the range as far as no third hit comes in
            others = [n for h, n, i in by_hash[:x + 1] if not lo <= n <= hi]
            wlo = max([n + 1 for n in others if n < lo] + [LOW[0]])
            whi = min([n - 1 for n in others if n > hi] + [LOW[1]])
            if best is None or whi - wlo > best[1] - best[0]:
                best = (wlo, whi, hx, (na, ia), (nb, ib))
    assert best is not None
    return best


@pytest.mark.parametrize("first_group_wins", [False, True])
def test_hit_word_is_shared_across_launches(gpu_ctx, first_group_wins):
    vs = VERS9[:6]
    lo, hi, T, (na, ia), (nb, ib) = _cross_case(first_group_wins)
    hits = [(n, i) for h, n, i in pairs(vs, lo, hi) if h <= T]
    assert sorted(hits) == sorted([(na, ia), (nb, ib)]) and ia >= 4 > ib and hi - lo >= 1000
    n, i = min(hits)
    assert (n, i) == ((nb, ib) if first_group_wins else (na, ia))
    want = (True, H(vs[i], n), n, i)
    assert expect(vs, lo, hi, T) == want
    for _ in range(3):
        assert gpu_ctx.search_header_versions(GENESIS, vs, lo, hi, T) == want
    assert gpu_ctx.last_stats().launches == 2


# ---- 5. the hot path's 32-bit filter ------------------------------------------

def test_hot_path_boundary(gpu_ctx):
    """T = a pair's hash with only its top 32 bits kept: that hash's top word
    equals the target's, so the filter lets it through and the full compare
    decides."""
    cols = [column(v, *LOW) for v in VERS4]
    for n, i in ((0, 0), (4200, 2), (8603, 1), (30001, 3), (65535, 2)):
        T = (cols[i][n] >> 224) << 224
        assert gpu_ctx.search_header_versions(GENESIS, VERS4, *LOW, T) == expect(VERS4, *LOW, T), (n, i)


# ---- 6. edges ----------------------------------------------------------------

def test_empty_and_single_ranges(gpu_ctx):
    assert gpu_ctx.search_header_versions(GENESIS, VERS4, 5, 4, U256) == (False, U256, U32, 0)
    assert gpu_ctx.last_target_stats().nonces_dispatched == 0
    r = _lib.HeaderVersionsResult()
    arr = (ctypes.c_uint32 * 3)(7, 8, 9)
    assert gpu_ctx._lib.bm_search_header_versions_gpu(gpu_ctx.handle, GENESIS, arr, 3, U32, 0, bytes(32),
                                                      ctypes.byref(r)) == _lib.BM_OK
    assert (r.found, r.nonce, r.version_index, r.version, bytes(r.hash)) == (0, U32, 0, 7, b"\xff" * 32)
    for n in (0, 255, 256, U32):
        hs = [H(v, n) for v in VERS4]
        assert gpu_ctx.search_header_versions(GENESIS, VERS4, n, n, U256) == (True, hs[0], n, 0)
        _, i = min((h >> 192, i) for i, h in enumerate(hs))
        assert gpu_ctx.search_header_versions(GENESIS, VERS4, n, n, 0) == (False, hs[i], n, i)
        assert gpu_ctx.last_target_stats().nonces_dispatched == 4
        h3 = H(VERS9[2], n)
        assert gpu_ctx.search_header_versions(GENESIS, VERS9[:3], n, n, min(hs[:3])) == \
            (True, min(hs[:3]), n, hs.index(min(hs[:3])))
        assert h3 == hs[2]


def test_top_window(gpu_ctx):
    lo, hi = GOLDEN["genesis_windows"]["top"]["range"]
    assert (lo, hi) == (2 ** 32 - 2 ** 16, U32)
    T = smallest(VERS4, lo, hi)[2][0]
    assert gpu_ctx.search_header_versions(GENESIS, VERS4, lo, hi, T) == expect(VERS4, lo, hi, T)
    # no wrap past 2^32-1: the whole window, and nothing else, is scanned
    assert gpu_ctx.search_header_versions(GENESIS, VERS4, lo, hi, 0) == expect(VERS4, lo, hi, 0)
    assert gpu_ctx.last_target_stats().nonces_dispatched == 65536 * 4


def _edge_cases(vs):
    """[(versions, lo, hi, target, want, pairs dispatched or None)]: what
    test_empty_and_single_ranges and test_top_window assert, for any list."""
    nver = len(vs)
    cases = [(vs, 5, 4, U256, (False, U256, U32, 0), 0), (vs, U32, 0, 0, (False, U256, U32, 0), 0)]
    for n in (0, 255, 256, U32):
        hs = [H(v, n) for v in vs]
        _, i = min((h >> 192, i) for i, h in enumerate(hs))
        cases.append((vs, n, n, U256, (True, hs[0], n, 0), None))
        cases.append((vs, n, n, 0, (False, hs[i], n, i), nver))
        cases.append((vs, n, n, min(hs), (True, min(hs), n, hs.index(min(hs))), None))
        cases.append((vs, n, n, min(hs) - 1, (False, hs[i], n, i), nver))
    lo, hi = GOLDEN["genesis_windows"]["top"]["range"]
    assert (lo, hi) == (2 ** 32 - 2 ** 16, U32)
    T = smallest(vs, lo, hi)[2][0]
    cases.append((vs, lo, hi, T, expect(vs, lo, hi, T), None))
    # no wrap past 2^32-1: the whole window, and nothing else, is scanned
    cases.append((vs, lo, hi, 0, expect(vs, lo, hi, 0), 65536 * nver))
    for c in cases[2:]:
        assert c[4] == expect(*c[:4])
    return cases


@pytest.mark.parametrize("nver", [4, 2, 1])
def test_edges_every_kernel(gpu_ctx, nver):
    """The empty, single-nonce and top-of-range cases for M = 4, 2 and 1."""
    for vs, lo, hi, T, want, dispatched in _edge_cases(VERS4[:nver]):
        assert gpu_ctx.search_header_versions(GENESIS, vs, lo, hi, T) == want, (lo, hi, hex(T))
        if dispatched is not None:
            assert gpu_ctx.last_target_stats().nonces_dispatched == dispatched, (lo, hi, hex(T))
        if lo <= hi:
            assert gpu_ctx.last_stats().launches == 1


_CHILD_EDGES = r"""
import json, sys
from distributed_bitcoin_minter_amd import Context
header = bytes.fromhex(sys.argv[1])
cases = json.loads(sys.argv[2])
out = []
with Context(num_gpus=1) as ctx:
    for vs, lo, hi, t in cases:
        f, h, n, i = ctx.search_header_versions(header, vs, lo, hi, int(t, 16))
        out.append([f, format(h, "x"), n, i, ctx.last_target_stats().nonces_dispatched, ctx.last_stats().launches])
print(json.dumps(out))
"""


def test_edges_one_version_per_launch():
    """The same cases under BTCMINER_HEADER_GROUP=1, in one fresh child: every
    list runs as launches of the M = 1 kernel."""
    cases = [c for nver in (4, 2, 1) for c in _edge_cases(VERS4[:nver])]
    arg = json.dumps([[list(vs), lo, hi, format(T, "x")] for vs, lo, hi, T, _, _ in cases])
    r = subprocess.run([sys.executable, "-c", _CHILD_EDGES, GENESIS.hex(), arg], capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, BTCMINER_HEADER_GROUP="1"))
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert len(got) == len(cases)
    for (vs, lo, hi, T, want, dispatched), (f, h, n, i, disp, launches) in zip(cases, got):
        assert (bool(f), int(h, 16), n, i) == want, (vs, lo, hi, hex(T))
        if dispatched is not None:
            assert disp == dispatched, (vs, lo, hi, hex(T))
        if lo <= hi:
            assert launches == len(vs)


# ---- 6b. other headers ---------------------------------------------------------

def _other_headers():
    rng = random.Random(0xC0DE)
    return [bytes(rng.getrandbits(8) for _ in range(80)) for _ in range(4)] + [b"\x00" * 80, b"\xff" * 80]


OTHER_VERSIONS = ((0, 0xffffffff, 0x20000000, 1),                   # one launch of 4
                  (0x3fffe000, 0, 2, 0xffffffff, 0x20004000),       # 4 + 1
                  (0xffffffff, 0x1fffe000, 0))                      # 2 + 1


def _other_cases():
    """(header, versions, lo, hi, pick): six headers under three version lists
    each, ranges of at most 2^13 nonces (at most 5 * 2^13 pairs), a third
    starting at 0, a third ending at 2^32-1, the rest anywhere."""
    assert all(set(vs) <= set(VERS9) and {0, 0xffffffff} <= set(vs) for vs in OTHER_VERSIONS)
    rng = random.Random(0x0715)
    cases = []
    for hi_, header in enumerate(_other_headers()):
        for vi, vs in enumerate(OTHER_VERSIONS):
            k = 3 * hi_ + vi
            length = [1, 255, 256, 257, 8192, 8191][k] if k < 6 else rng.randint(2, 8192)
            where = (hi_ + vi) % 3
            lo = 0 if where == 0 else U32 - length + 1 if where == 1 else rng.randint(1, U32 - length)
            cases.append((header, vs, lo, lo + length - 1, rng.random()))
    return cases


@pytest.mark.parametrize("case", _other_cases(), ids=lambda c: f"{c[0][:2].hex()}-{len(c[1])}v-{c[2]}+{c[3] - c[2] + 1}")
def test_other_headers(gpu_ctx, case):
    """The shared schedule words (w16, w17, k18, k19, k31, k32) come from header
    bytes 64..75: here they take other values than the genesis block's."""
    header, vs, lo, hi, pick = case
    nver, length = len(vs), hi - lo + 1
    assert length <= 2 ** 13 and header[64:76] != GENESIS[64:76]
    by_hash = smallest(vs, lo, hi, 50, header)
    T = by_hash[int(pick * min(len(by_hash), 50))][0]  # one of the window's own 50 smallest pair hashes
    want = expect(vs, lo, hi, T, header)
    assert want[0]
    assert gpu_ctx.search_header_versions(header, vs, lo, hi, T) == want
    want = expect(vs, lo, hi, by_hash[0][0] - 1, header)
    assert want == (False,) + by_hash[0]
    assert gpu_ctx.search_header_versions(header, vs, lo, hi, by_hash[0][0] - 1) == want
    assert gpu_ctx.last_target_stats().nonces_dispatched == length * nver
    assert gpu_ctx.last_stats().launches == nver // 4 + (nver % 4) // 2 + nver % 2


# ---- 7. independence from grouping and scheduling ------------------------------

_CHILD = r"""
import json, sys
from distributed_bitcoin_minter_amd import Context
header = bytes.fromhex(sys.argv[1])
cases = json.loads(sys.argv[2])
with Context(num_gpus=1) as ctx:
    out = [list(ctx.search_header_versions(header, vs, lo, hi, int(t, 16))) for vs, lo, hi, t in cases]
print(json.dumps([[f, format(h, "x"), n, i] for f, h, n, i in out]))
"""


def _case_table():
    cases = group_cases()
    for first in (False, True):
        lo, hi, T, _, _ = _cross_case(first)
        cases.append((VERS9[:6], lo, hi, T))
    cases.append((VERS4, 4200, 4200, U256))
    return cases


@pytest.mark.parametrize("env", [{"BTCMINER_HEADER_GROUP": "1"}, {"BTCMINER_HEADER_GROUP": "2"},
                                 {"BTCMINER_HEADER_GROUP": "4"}, {"BTCMINER_CHUNK": "10", "BTCMINER_STREAMS": "1"}],
                         ids=lambda e: ",".join(f"{k[9:]}={v}" for k, v in e.items()))
def test_case_table_under_knobs(env):
    cases = _case_table()
    want = [expect(*c) for c in cases]
    arg = json.dumps([[list(vs), lo, hi, format(T, "x")] for vs, lo, hi, T in cases])
    r = subprocess.run([sys.executable, "-c", _CHILD, GENESIS.hex(), arg], capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, **env))
    assert r.returncode == 0, r.stderr
    got = [(bool(f), int(h, 16), n, i) for f, h, n, i in json.loads(r.stdout)]
    assert got == want


def test_case_table_one_block_per_cu(gpu_ctx):
    cases = _case_table()
    gpu_ctx.set_blocks_per_cu(1)
    try:
        got = [gpu_ctx.search_header_versions(GENESIS, *c) for c in cases]
    finally:
        gpu_ctx.set_blocks_per_cu(0)
    assert got == [expect(*c) for c in cases]


# ---- 8. multi-device on one GPU ----------------------------------------------

MULTI = (393216, 393216 + 3 * 2 ** 15 - 1)
MULTI_VERSIONS = (0x36001, 1, 0x40001)  # the minima of the window's halves and thirds over these descend (asserted below)


def test_multi_device_on_one_gpu(gpu_ctx):
    lo, hi = MULTI
    vs = MULTI_VERSIONS
    p = pairs(vs, lo, hi)
    for ndev in (2, 3):
        pieces = _lib.split_range(lo, hi, ndev)
        with Context(devices=[0] * ndev) as ctx:
            for k, (a, b) in enumerate(pieces):
                # T = piece k's minimum: no earlier piece holds a hit, so the winning hit lies in piece k
                T = min(h for h, n, i in p if a <= n <= b)
                want = expect(vs, lo, hi, T)
                assert want[0] and a <= want[2] <= b, (ndev, k)
                assert ctx.search_header_versions(GENESIS, vs, lo, hi, T) == want, (ndev, k)
                ts = ctx.last_target_stats()
                assert ts.devices == ndev and sum(ts.dev_dispatched[:ndev]) == ts.nonces_dispatched
                assert gpu_ctx.search_header_versions(GENESIS, vs, lo, hi, T) == want
            # hits in every piece: the lowest device's wins
            T = smallest(vs, lo, hi)[40][0]
            assert ctx.search_header_versions(GENESIS, vs, lo, hi, T) == expect(vs, lo, hi, T)
            # not found
            want = expect(vs, lo, hi, 0)
            assert ctx.search_header_versions(GENESIS, vs, lo, hi, 0) == want
            assert gpu_ctx.search_header_versions(GENESIS, vs, lo, hi, 0) == want
            assert ctx.last_target_stats().nonces_dispatched == (hi - lo + 1) * 3
            st = ctx.last_stats()
            assert st.launches == 2 * ndev and st.combine_used == _lib.BM_COMBINED_HOST  # groups 2 + 1 per device
            ctx.set_split([1, 5, 2][:ndev])
            assert ctx.search_header_versions(GENESIS, vs, lo, hi, 0) == want
            # a range shorter than the device count leaves a device empty
            n = lo + 5
            hs = [H(v, n) for v in vs]
            _, i = min((h >> 192, i) for i, h in enumerate(hs))
            assert ctx.search_header_versions(GENESIS, vs, n, n, 0) == (False, hs[i], n, i)
            assert ctx.search_header_versions(GENESIS, vs, n, n, U256) == (True, hs[0], n, 0)


# ---- 9. failure paths --------------------------------------------------------

def test_bad_arguments(gpu_ctx):
    f = gpu_ctx._lib.bm_search_header_versions_gpu
    r = _lib.HeaderVersionsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    before = bytes(r)
    tgt, out = bytes(32), ctypes.byref(r)
    arr = (ctypes.c_uint32 * 65)(*range(65))
    h = gpu_ctx.handle
    assert f(None, GENESIS, arr, 4, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert f(h, None, arr, 4, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, None, 4, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 4, 0, 1, None, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 4, 0, 1, tgt, None) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 0, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert f(h, GENESIS, arr, 65, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert bytes(r) == before
    assert f(h, GENESIS, arr, 64, 0, 255, tgt, out) == _lib.BM_OK  # 64 versions: 16 launches of 4
    assert r.found == 0 and gpu_ctx.last_target_stats().nonces_dispatched == 256 * 64
    assert gpu_ctx.last_stats().launches == 16


def test_rank_context_is_refused():
    with Context(devices=[0], rank=1, world=2) as ctx:
        with pytest.raises(_lib.BtcMinerError) as ei:
            ctx.search_header_versions(GENESIS, VERS4, 0, 1000, 0)
        assert ei.value.status == _lib.BM_EINVAL
    with Context(devices=[0], rank=0, world=1) as ctx:  # a group of one is a single device
        T = (1 << 244) - 1
        assert ctx.search_header_versions(GENESIS, VERS4, *LOW, T) == expect(VERS4, *LOW, T)


def test_failed_call_leaves_out_and_context_alone(gpu_ctx):
    r = _lib.HeaderVersionsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    before = bytes(r)
    arr = (ctypes.c_uint32 * 4)(*VERS4)
    gpu_ctx.set_test_fault(0)
    try:
        rc = gpu_ctx._lib.bm_search_header_versions_gpu(gpu_ctx.handle, GENESIS, arr, 4, 0, 65535, bytes(32),
                                                        ctypes.byref(r))
        assert rc == _lib.BM_EINTERNAL
        assert bytes(r) == before
        assert gpu_ctx.last_target_stats().nonces_dispatched == 0
    finally:
        gpu_ctx.set_test_fault(-1)
    T = (1 << 244) - 1
    assert gpu_ctx.search(b"bradfitz", 0, 9999) == (1419516646206828, 9898)
    assert gpu_ctx.search_header(GENESIS, *LOW, T) == (True, H(1, 4200), 4200)
    assert gpu_ctx.search_header_versions(GENESIS, VERS4, *LOW, T) == expect(VERS4, *LOW, T)


# ---- 10. CLI -----------------------------------------------------------------

def test_mine_versions_cli(gpu_ctx):
    versions = _lib.roll_versions(1, 4)
    found, h, n, i = expect(tuple(versions), *LOW, (1 << 244) - 1)
    assert found
    out = io.StringIO()
    assert mine_versions.main([GENESIS.hex(), "--versions", "4", "--zero-bits", "12", "0", "65535"], out=out,
                              ctx=gpu_ctx) == 0
    assert out.getvalue() == f"Found {h:064x} {n} {versions[i]:08x}\n"
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.mine_versions", GENESIS.hex(),
                        "--versions", "4", "--zero-bits", "12", "0", "65535"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
    assert r.stdout == out.getvalue()


# ---- 11. the whole nonce space -------------------------------------------------

def test_full_range_genesis_bits(gpu_ctx):
    """[0, 2^32-1] under the four versions at the genesis block's own bits:
    about 0.7 s of GPU work.  The expected pair cannot be computed here (about
    1.5 hits of the other three versions are expected below the genesis nonce),
    so: the returned pair is a hit by hashlib, lies at or below the genesis
    nonce (index 2 on equality), and the dispatch count is consistent."""
    target = bits_to_target(GEN["bits"])
    found, h, n, i = gpu_ctx.search_header_versions(GENESIS, VERS4, 0, U32, target)
    ts = gpu_ctx.last_target_stats()
    print("full range:", found, f"{h:064x}", n, i, "dispatched", ts.nonces_dispatched)
    assert found
    assert H(VERS4[i], n) == h <= target
    assert n <= GEN["nonce"]
    if n == GEN["nonce"]:
        assert i == 2 and h == int(GEN["hash"], 16)
    assert n + 1 <= ts.nonces_dispatched <= 4 * 2 ** 32
    assert gpu_ctx.last_stats().launches == 1
