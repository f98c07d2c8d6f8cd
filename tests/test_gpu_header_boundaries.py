"""A device boundary inside a 256-nonce task: the three block-header entry
points over several devices (one GPU listed two and three times), against
hashlib and against a one-device context.

The kernels scan whole tasks of 256 nonces and clip them to the launch's
range (n >= lo && n <= hi).  When a piece of a split range begins or ends
inside a task, the two neighbouring devices both hash that task, and the clip
alone keeps every nonce counted once and on the right device.  The piece
boundaries are read from the library's partitioner and asserted to fall where
each case needs them; no rounding rule is assumed.

Every window lies inside tests/test_gpu_header.py's LOW (at most 50,001
nonces; the three-version cases cut theirs from the LOW columns of
tests/test_gpu_header_versions.py), computed once and shared."""
import struct

import pytest

from distributed_bitcoin_minter_amd import Context, _lib
from test_gpu_header import GENESIS, H, expect as expect_first, window
from test_gpu_header_hits import CAP, expect as expect_hits
from test_gpu_header_versions import H as HV, VERS4, column, expect as expect_versions, smallest

pytestmark = pytest.mark.gpu

U256 = (1 << 256) - 1
TASK = 256
NMIN = 8603  # the nonce of LOW's smallest hash under the genesis header: 33 * 256 + 155
VERS3 = VERS4[:3]  # (0x20000000, 0x20002000, 1): groups 2 + 1; index 2 is the genesis block's own version


# ---- 1. the minimum on either side of a cut ------------------------------------

def _range_cut_at(side):
    """A range of about 10^4 nonces around 8603 that two devices cut so that
    piece 1 begins at 8603 ("first") or piece 0 ends at 8603 ("last")."""
    for lo, hi in ((NMIN - 5000, NMIN + 4999), (NMIN - 5000, NMIN + 5000), (NMIN - 5000, NMIN + 4998),
                   (NMIN - 4999, NMIN + 5000), (NMIN - 4999, NMIN + 4999), (NMIN - 4999, NMIN + 5001)):
        pieces = _lib.split_range(lo, hi, 2)
        if None in pieces:
            continue
        (a0, b0), (a1, b1) = pieces
        if (a1 if side == "first" else b0) == NMIN:
            return lo, hi, pieces
    pytest.fail(f"no range around {NMIN} is cut with {NMIN} as the {side} nonce of a piece")


@pytest.mark.parametrize("side", ["first", "last"])
def test_minimum_beside_a_cut(gpu_ctx, side):
    lo, hi, ((a0, b0), (a1, b1)) = _range_cut_at(side)
    assert (a0, b1) == (lo, hi) and a1 == b0 + 1 and 9000 <= hi - lo + 1 <= 11000
    assert (a1 if side == "first" else b0) == NMIN and NMIN % TASK == 155 and a1 % TASK != 0
    hmin = H(GENESIS, NMIN)
    assert min(window(GENESIS, lo, hi)) == (hmin, NMIN)
    assert smallest(VERS3, lo, hi, 1)[0] == (hmin, NMIN, 2) and HV(1, NMIN) == hmin
    with Context(devices=[0, 0]) as ctx:
        for c in (ctx, gpu_ctx):
            # T = H(8603): found, and listed, exactly once
            assert c.search_header(GENESIS, lo, hi, hmin) == (True, hmin, NMIN) == expect_first(GENESIS, lo, hi, hmin)
            assert c.search_header_hits(GENESIS, lo, hi, hmin, CAP) == (1, [(hmin, NMIN)], (hmin, NMIN))
            assert c.search_header_versions(GENESIS, VERS3, lo, hi, hmin) == (True, hmin, NMIN, 2)
            # one below: nothing found, 8603 the best share
            assert c.search_header(GENESIS, lo, hi, hmin - 1) == (False, hmin, NMIN)
            assert c.last_target_stats().nonces_dispatched == hi - lo + 1
            assert c.search_header_hits(GENESIS, lo, hi, hmin - 1, CAP) == (0, [], (hmin, NMIN))
            assert c.search_header_versions(GENESIS, VERS3, lo, hi, hmin - 1) == (False, hmin, NMIN, 2)
            assert c.last_target_stats().nonces_dispatched == (hi - lo + 1) * 3
            # every nonce, each exactly once
            got = c.search_header_hits(GENESIS, lo, hi, U256, CAP)
            assert got[0] == hi - lo + 1 and got == expect_hits(GENESIS, lo, hi, U256)
            assert c.search_header_hits(GENESIS, lo, hi, U256, 0)[0] == hi - lo + 1  # count mode
        assert expect_hits(GENESIS, lo, hi, hmin) == (1, [(hmin, NMIN)], (hmin, NMIN))
        assert expect_versions(VERS3, lo, hi, hmin) == (True, hmin, NMIN, 2)
        assert expect_versions(VERS3, lo, hi, hmin - 1) == (False, hmin, NMIN, 2)
        assert ctx.last_stats().launches == 2


# ---- 2. unaligned pieces in general --------------------------------------------

ODD = (1000, 51000)  # 50,001 nonces: its halves and thirds begin on no multiple of 256
# Under version 0x2001a000 the window's smallest hash lies at nonce 47644, in the
# last piece of every split below; under the other two versions nothing is as low.
LATE_VERSION = 0x2001a000
LATE = struct.pack("<I", LATE_VERSION) + GENESIS[4:]
LATE_VERSIONS = (0x20000000, LATE_VERSION, 1)


@pytest.mark.parametrize("ndev,shares", [(2, None), (3, None), (2, [1, 5]), (3, [1, 5, 2])],
                         ids=["2", "3", "2-shares", "3-shares"])
def test_unaligned_pieces(gpu_ctx, ndev, shares):
    lo, hi = ODD
    length = hi - lo + 1
    assert shares is None or shares == [1, 5, 2][:ndev]
    pieces = _lib.split_range(lo, hi, ndev, shares)
    assert None not in pieces and pieces[0][0] == lo and pieces[-1][1] == hi
    for (a, b), (a2, b2) in zip(pieces, pieces[1:]):
        assert a2 == b + 1 and a2 % TASK != 0, pieces
    a_last = pieces[-1][0]
    with Context(devices=[0] * ndev) as ctx:
        if shares is not None:
            ctx.set_split(shares)
        # every nonce once
        got = ctx.search_header_hits(GENESIS, lo, hi, U256, CAP)
        assert got[0] == length and got == expect_hits(GENESIS, lo, hi, U256)
        st = ctx.last_stats()
        assert st.launches == ndev and st.nonces == length
        # the window's 300th smallest hash: hits in every piece
        T = sorted(window(GENESIS, lo, hi))[299][0]
        want = expect_hits(GENESIS, lo, hi, T)
        assert want[0] == 300 and all(any(a <= n <= b for _, n in want[1]) for a, b in pieces)
        assert ctx.search_header_hits(GENESIS, lo, hi, T, CAP) == want
        assert gpu_ctx.search_header_hits(GENESIS, lo, hi, T, CAP) == want
        # the first hit lies in the last piece
        hmin, nmin = min(window(LATE, lo, hi))
        want = expect_first(LATE, lo, hi, hmin)
        assert want == (True, hmin, nmin) and nmin >= a_last and nmin == 47644
        assert ctx.search_header(LATE, lo, hi, hmin) == want == gpu_ctx.search_header(LATE, lo, hi, hmin)
        wantv = expect_versions(LATE_VERSIONS, lo, hi, hmin)
        assert wantv == (True, hmin, nmin, 1) and column(LATE_VERSION, lo, hi)[nmin - lo] == hmin
        assert ctx.search_header_versions(GENESIS, LATE_VERSIONS, lo, hi, hmin) == wantv
        assert gpu_ctx.search_header_versions(GENESIS, LATE_VERSIONS, lo, hi, hmin) == wantv
        # nothing found: every nonce handed out once, the best share hashlib's
        want = expect_first(GENESIS, lo, hi, 0)
        assert not want[0]
        assert ctx.search_header(GENESIS, lo, hi, 0) == want
        ts = ctx.last_target_stats()
        assert ts.nonces_dispatched == length and ts.devices == ndev and sum(ts.dev_dispatched[:ndev]) == length
        wantv = expect_versions(LATE_VERSIONS, lo, hi, 0)
        assert wantv == (False, hmin, nmin, 1)
        assert ctx.search_header_versions(GENESIS, LATE_VERSIONS, lo, hi, 0) == wantv
        assert ctx.last_target_stats().nonces_dispatched == length * 3
        assert ctx.last_stats().launches == 2 * ndev  # groups 2 + 1 per device
