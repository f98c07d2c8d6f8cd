"""Launch geometry and per-call host behaviour, pinned.

tests/golden/launch_shape.json holds, for a fixed table of calls (all seven
searches; one device and three slots of one device), the result and every
bm_launch_stat_t the library recorded: layout, task size, grid, tasks per
thread.  It was recorded from the build of the commit named in its
`made_from` (tests/golden/make_launch_shape_golden.py), never from the tree
under test, and this test replays the table and asserts equality: a slip in
the sizing arithmetic changes speed, not results, and nothing else would see
it.  The geometry follows the CU count, so on a device with another count than
the file's the replay skips.

Also here: a header search submits its devices' work like the other searches
(bm_stats_t.start_threads), and its failure path on several devices."""
import ctypes
import importlib.util
import os

import pytest

from conftest import GOLDEN, load_golden
from distributed_bitcoin_minter_amd import Context, _lib

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_launch_shape_golden",
                                               os.path.join(GOLDEN, "make_launch_shape_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

SHAPES = load_golden("launch_shape.json")
GENESIS = gen.genesis_header()


@pytest.fixture(scope="module")
def cus():
    return gen.device_cus(Context)


def test_golden_covers_the_table():
    # the file is data: the calls replayed are the generator's table, all of it
    assert [{k: v for k, v in c.items() if k != "expect"} for c in SHAPES["cases"]] == gen.CASES


@pytest.mark.parametrize("case", SHAPES["cases"], ids=lambda c: c["name"])
def test_launch_shape(cus, case):
    if cus != SHAPES["cus"]:
        pytest.skip(f"the golden launch shapes are for {SHAPES['cus']} CUs; this device has {cus}")
    assert gen.run_case(Context, case) == case["expect"]


def test_header_search_submits_like_a_search():
    with Context(devices=[0] * 3) as ctx:
        ctx.search(b"msg", 0, 99999)
        threads = ctx.last_stats().start_threads
        assert threads == 3  # the caller and one pool thread per further device
        ctx.search_header(GENESIS, 393216, 393216 + 3 * 2**15 - 1, 0)
        assert ctx.last_stats().start_threads == threads


def test_header_fault_on_two_slots():
    lo, hi, target = 0, 16383, (1 << 244) - 1
    want = expect_header(lo, hi, target)
    lib = _lib.load()
    with Context(devices=[0, 0]) as ctx:
        ctx.set_test_fault(1)  # one launch goes out, the other slot's is refused
        r = _lib.HeaderResult()
        ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
        before = bytes(r)
        rc = lib.bm_search_header_gpu(ctx.handle, GENESIS, lo, hi, bytes(32), ctypes.byref(r))
        assert rc == _lib.BM_EINTERNAL
        assert bytes(r) == before
        assert ctx.last_target_stats().nonces_dispatched == 0
        ctx.set_test_fault(-1)
        assert ctx.search_header(GENESIS, lo, hi, target) == want
        assert ctx.search(b"msg", 0, 2) == (4754799531757243342, 1)  # the README's worked example


def expect_header(lo, hi, target):
    """bm_search_header_gpu's answer over a small window, from hashlib."""
    import hashlib
    import struct

    def H(n):
        return int.from_bytes(hashlib.sha256(hashlib.sha256(GENESIS[:76] + struct.pack("<I", n)).digest()).digest(),
                              "little")
    hit = next((n for n in range(lo, hi + 1) if H(n) <= target), None)
    if hit is not None:
        return (True, H(hit), hit)
    n = min(range(lo, hi + 1), key=lambda n: (H(n) >> 192, n))
    return (False, H(n), n)
