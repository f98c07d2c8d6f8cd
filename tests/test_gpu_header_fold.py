"""bm_search_header_gpu and bm_search_header_hits_gpu are the one-version case
of the version-rolling searches: for a header h, search_header(h, ...) is
search_header_versions(h, [le32(h[0:4])], ...) without the index, and so for
the enumerations, and both are what hashlib says.

Three headers whose version field has four distinct non-zero bytes, so a
byte-order slip in reading it shows: the genesis header under version
0x04A1C320, and 80 bytes of random.Random(0xF01D) and random.Random(0xF01E)
under versions 0x27D5C3A1 and 0x1B2A3C4D.  Every hashlib window is computed
once (test_gpu_header.window) and shared."""
import random
import struct

import pytest

from distributed_bitcoin_minter_amd import Context
from test_gpu_header import GENESIS, H, window

pytestmark = pytest.mark.gpu

U32 = (1 << 32) - 1
U256 = (1 << 256) - 1


def _header(base: bytes, version: int) -> bytes:
    assert len({*struct.pack("<I", version)} - {0}) == 4
    return struct.pack("<I", version) + base[4:]


HEADERS = [(_header(GENESIS, 0x04A1C320), 0x04A1C320),
           (_header(random.Random(0xF01D).randbytes(80), 0x27D5C3A1), 0x27D5C3A1),
           (_header(random.Random(0xF01E).randbytes(80), 0x1B2A3C4D), 0x1B2A3C4D)]
IDS = ["genesis-04a1c320", "seed-f01d", "seed-f01e"]
BIG = (1000, 1000 + 2 ** 18)  # one piece per slot of a two-slot context
MID = BIG[0] + (BIG[1] - BIG[0] + 1) // 2  # the partitioner's cut, to within a nonce


def first_hit(header, lo, hi, target):
    """What both first-hit searches must return (without the index), from hashlib."""
    if lo > hi:
        return (False, U256, U32)
    w = window(header, lo, hi)
    hit = next(((h, n) for h, n in w if h <= target), None)
    if hit is not None:
        return (True,) + hit
    _, n = min((h >> 192, n) for h, n in w)
    return (False, H(header, n), n)


def every_hit(header, lo, hi, target, cap):
    """What both enumerations must return (without the indices), from hashlib."""
    if lo > hi:
        return 0, [], (U256, U32)
    w = window(header, lo, hi)
    hits = [(h, n) for h, n in w if h <= target]
    _, n = min((h >> 192, n) for h, n in w)
    return len(hits), hits if len(hits) <= cap else None, (H(header, n), n)


def share_target(header):
    """A target with a handful of hits on both sides of the two-slot split: the
    24th smallest hash of the window."""
    w = window(header, *BIG)
    target = sorted(h for h, _ in w)[23]
    for half in ([n for h, n in w if h <= target and n < MID - 1], [n for h, n in w if h <= target and n > MID]):
        assert 2 <= len(half) <= 64, len(half)
    return target


def check_first(ctx, header, version, lo, hi, target):
    want = first_hit(header, lo, hi, target)
    one = ctx.search_header(header, lo, hi, target)
    st_one = (ctx.last_stats().launches, ctx.last_stats().nonces, ctx.last_target_stats().nonces_dispatched)
    rolled = ctx.search_header_versions(header, [version], lo, hi, target)
    st_rolled = (ctx.last_stats().launches, ctx.last_stats().nonces, ctx.last_target_stats().nonces_dispatched)
    assert one == want, (lo, hi, hex(target), one, want)
    assert rolled == want + (0,), (lo, hi, hex(target), rolled, want)
    assert st_one == st_rolled, (lo, hi, st_one, st_rolled)
    if lo <= hi and not want[0]:
        assert st_one[2] == hi - lo + 1  # nothing hit: every nonce was handed out
    return want


def check_every(ctx, header, version, lo, hi, target, cap):
    want = every_hit(header, lo, hi, target, cap)
    one = ctx.search_header_hits(header, lo, hi, target, cap)
    st_one = (ctx.last_stats().launches, ctx.last_stats().nonces)
    count, hits, best = ctx.search_header_versions_hits(header, [version], lo, hi, target, cap)
    st_rolled = (ctx.last_stats().launches, ctx.last_stats().nonces)
    assert one == want, (lo, hi, hex(target), cap, one[0], want[0])
    assert best[2] == 0 and (hits is None or all(i == 0 for _, _, i in hits))
    assert (count, None if hits is None else [s[:2] for s in hits], best[:2]) == want
    assert st_one == st_rolled, (lo, hi, st_one, st_rolled)
    return want


@pytest.mark.parametrize("header,version", HEADERS, ids=IDS)
def test_small_ranges(gpu_ctx, header, version):
    """[255, 257] clips inside two 256-nonce tasks; the top of the nonce space,
    where the key of the last nonce sits next to the all-ones "none"; single
    nonces; an empty range."""
    ranges = [(255, 257), (0xFFFFFF00, U32), (256, 256), (U32, U32), (5, 4)]
    for lo, hi in ranges:
        hashes = sorted(h for h, _ in window(header, lo, hi)) if lo <= hi else [1]
        for target in (0, U256, hashes[0], hashes[0] - 1, hashes[-1]):
            check_first(gpu_ctx, header, version, lo, hi, target)
            for cap in (0, 1, 256):
                check_every(gpu_ctx, header, version, lo, hi, target, cap)
    # the last nonce alone hits: the hit word holds the highest key there is
    h_top = H(header, U32)
    others = min(h for h, n in window(header, 0xFFFFFF00, U32) if n != U32)
    if h_top > others:  # else the case above at hashes[0] was this one
        got = gpu_ctx.search_header_hits(header, U32, U32, h_top, 1)
        assert got == (1, [(h_top, U32)], (h_top, U32))
    assert gpu_ctx.search_header(header, U32, U32, h_top) == (True, h_top, U32)


@pytest.mark.parametrize("header,version", HEADERS, ids=IDS)
def test_two_slots_hits_on_both_sides(header, version):
    target = share_target(header)
    with Context(devices=[0, 0]) as ctx:
        want = check_first(ctx, header, version, *BIG, target)
        assert want[0] and ctx.last_stats().launches == 2
        check_first(ctx, header, version, *BIG, 0)
        count = check_every(ctx, header, version, *BIG, target, 64)[0]
        assert count == 24
        # all or nothing, through the narrowed entry type: cap at the count, and one below it
        assert len(check_every(ctx, header, version, *BIG, target, count)[1]) == count
        assert check_every(ctx, header, version, *BIG, target, count - 1)[1] is None
        for cap in (0, 1):
            assert check_every(ctx, header, version, *BIG, 0, cap)[:2] == (0, [])
        full = BIG[1] - BIG[0] + 1
        assert len(check_every(ctx, header, version, *BIG, U256, full)[1]) == full
        assert check_every(ctx, header, version, *BIG, U256, full - 1)[:2] == (full, None)
