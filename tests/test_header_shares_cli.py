"""The `header_shares` command line (no GPU): parsing, the halving on
count > cap, ntime rolling and the output lines, with a stand-in context that
answers from hashlib."""
import hashlib
import io
import struct

import pytest

from conftest import load_golden
from distributed_bitcoin_minter_amd import header_shares

GOLDEN = load_golden("header_vectors.json")
G = next(g for g in GOLDEN["headers"] if g["name"] == "genesis")
HX = G["header"]
GENESIS = bytes.fromhex(HX)
NTIME = 1231006505
U32 = (1 << 32) - 1
U256 = (1 << 256) - 1


def H(header: bytes, nonce: int) -> int:
    d = hashlib.sha256(hashlib.sha256(header[:76] + struct.pack("<I", nonce)).digest()).digest()
    return int.from_bytes(d, "little")


class Ctx:
    """search_header_hits as the library defines it, from hashlib."""

    def __init__(self):
        self.calls = []

    def search_header_hits(self, header, lo, hi, target, cap):
        self.calls.append((header, lo, hi, target, cap))
        if lo > hi:
            return 0, [], (U256, U32)
        w = [(H(header, n), n) for n in range(lo, hi + 1)]
        hits = [(h, n) for h, n in w if h <= target]
        _, n = min((h >> 192, n) for h, n in w)
        return len(hits), hits if len(hits) <= cap else None, (H(header, n), n)


def run(argv):
    c, out = Ctx(), io.StringIO()
    assert header_shares.main(argv, out=out, ctx=c) == 0
    return c, out.getvalue().splitlines()


def test_parsing():
    assert header_shares.header_ntime(GENESIS) == NTIME
    assert header_shares.parse_args([HX, "--zero-bits", "12"]) == (GENESIS, (1 << 244) - 1, 0, U32, 4096, 1)
    assert header_shares.parse_args([HX, "--target", "ff", "5", "9", "--cap", "7", "--ntime-rolls", "3"]) == (
        GENESIS, 0xff, 5, 9, 7, 3)
    assert header_shares.parse_args([HX, "--cap", str(1 << 20), "--zero-bits", "0", "10"])[1:] == (
        U256, 10, U32, 1 << 20, 1)
    assert header_shares.with_ntime(GENESIS, NTIME) == GENESIS
    rolled = header_shares.with_ntime(GENESIS, U32 + 1)  # wraps
    assert rolled[68:72] == bytes(4) and rolled[:68] == GENESIS[:68] and rolled[72:] == GENESIS[72:]


@pytest.mark.parametrize("argv", [
    [], [HX],  # a target is required
    ["00", "--zero-bits", "1"], [HX[:-2], "--zero-bits", "1"], ["zz" + HX[2:], "--zero-bits", "1"],
    [HX, "--target", "f" * 65], [HX, "--target", "xyz"], [HX, "--target", ""],
    [HX, "--zero-bits", "257"], [HX, "--zero-bits", "-1"], [HX, "--zero-bits", "1_0"],
    [HX, "--target", "ff", "--zero-bits", "3"],
    [HX, "--zero-bits", "1", "-5"], [HX, "--zero-bits", "1", "0", str(U32 + 1)], [HX, "--zero-bits", "1", "0", "x"],
    [HX, "--zero-bits", "1", "0", "1", "2"],
    [HX, "--zero-bits", "1", "--cap", "0"], [HX, "--zero-bits", "1", "--cap", str((1 << 20) + 1)],
    [HX, "--zero-bits", "1", "--cap", "x"], [HX, "--zero-bits", "1", "--cap", "-4"],
    [HX, "--zero-bits", "1", "--ntime-rolls", "0"], [HX, "--zero-bits", "1", "--ntime-rolls", "1.5"],
    [HX, "--zero-bits", "1", "--ntime-rolls", str((1 << 16) + 1)], [HX, "--zero-bits", "1", "--bogus"],
])
def test_bad_input_exits_with_2(argv, capsys):
    c = Ctx()
    assert header_shares.main(argv, out=io.StringIO(), ctx=c) == 2
    assert capsys.readouterr().err.strip()
    assert c.calls == []  # rejected before any library call


def test_halving_returns_every_hit_once_and_in_order():
    lo, hi, target = 4000, 4999, (1 << 252) - 1  # 4 zero bits: about 60 of 1000
    want = [(H(GENESIS, n), n) for n in range(lo, hi + 1) if H(GENESIS, n) <= target]
    assert len(want) > 40
    c, lines = run([HX, "--zero-bits", "4", "--cap", "5", str(lo), str(hi)])
    assert lines[:-1] == [f"Share {h:064x} {NTIME} {n}" for h, n in want]
    bh, bn = min(((H(GENESIS, n), n) for n in range(lo, hi + 1)), key=lambda s: (s[0] >> 192, s[1]))
    assert lines[-1] == f"Shares {len(want)} Best {bh:064x} {NTIME} {bn}"
    assert len(c.calls) > len(want) // 5 and all(call[4] == 5 for call in c.calls)
    # the pieces that gave their hits tile the range, ascending
    done = [(a, b) for (_, a, b, _, _) in c.calls
            if sum(1 for _, n in want if a <= n <= b) <= 5]
    assert done[0][0] == lo and done[-1][1] == hi
    assert all(done[i][1] + 1 == done[i + 1][0] for i in range(len(done) - 1))
    # one call when the hits fit
    c, lines2 = run([HX, "--zero-bits", "4", "--cap", str(len(want)), str(lo), str(hi)])
    assert lines2 == lines and len(c.calls) == 1


def test_ntime_rolls_hash_the_rolled_header():
    lo, hi, target = 0, 599, (1 << 251) - 1
    c, lines = run([HX, "--zero-bits", "5", "--ntime-rolls", "3", str(lo), str(hi)])
    want, best = [], None
    for t in (NTIME, NTIME + 1, NTIME + 2):
        header = GENESIS[:68] + struct.pack("<I", t) + GENESIS[72:]
        for n in range(lo, hi + 1):
            h = H(header, n)
            if h <= target:
                want.append(f"Share {h:064x} {t} {n}")
            if best is None or (h >> 192, t, n) < (best[0] >> 192, best[1], best[2]):
                best = (h, t, n)
    assert len(want) > 30 and lines[:-1] == want  # ascending by (ntime, nonce)
    assert lines[-1] == f"Shares {len(want)} Best {best[0]:064x} {best[1]} {best[2]}"
    assert [call[0][68:72] for call in c.calls] == [struct.pack("<I", NTIME + r) for r in range(3)]
    assert all(call[0][:68] == GENESIS[:68] and call[0][72:] == GENESIS[72:] for call in c.calls)


def test_block_line():
    """A hit that also meets the header's own bits target is a Block."""
    n0 = G["nonce"]
    c, lines = run([HX, "--zero-bits", "3", str(n0 - 20), str(n0 + 20)])
    block = f"Block {G['hash']} {NTIME} {n0}"
    assert lines.count(block) == 1 and sum(ln.startswith("Block") for ln in lines) == 1
    assert sum(ln.startswith("Share ") for ln in lines) >= 2
    assert lines[-1] == f"Shares {len(lines) - 1} Best {G['hash']} {NTIME} {n0}"
    # an empty range: nothing to list, the empty best share
    c, lines = run([HX, "--zero-bits", "3", "9", "5"])
    assert lines == [f"Shares 0 Best {'f' * 64} {NTIME} {U32}"] and c.calls == []
