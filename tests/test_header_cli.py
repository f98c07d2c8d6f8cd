"""The `mine` command line: argument parsing, targets and error returns (no GPU)."""
import io

import pytest

from conftest import load_golden
from distributed_bitcoin_minter_amd import mine

GOLDEN = load_golden("header_vectors.json")
GENESIS = next(g for g in GOLDEN["headers"] if g["name"] == "genesis")
U32 = (1 << 32) - 1


def test_default_target_is_the_headers_bits():
    header, target, lo, hi = mine.parse_args([GENESIS["header"]])
    assert header == bytes.fromhex(GENESIS["header"]) and (lo, hi) == (0, U32)
    assert mine.header_bits(header) == 0x1d00ffff
    assert f"{target:064x}" == GENESIS["target"]
    b = next(g for g in GOLDEN["headers"] if g["name"] == "block125552")
    assert f"{mine.parse_args([b['header'].upper()])[1]:064x}" == b["target"]


def test_targets_and_bounds():
    hx = GENESIS["header"]
    assert mine.parse_args([hx, "--target", "ff"])[1:] == (0xff, 0, U32)
    assert mine.parse_args([hx, "--target", "0x" + "f" * 64])[1] == (1 << 256) - 1
    assert mine.parse_args([hx, "--zero-bits", "0"])[1] == (1 << 256) - 1
    assert mine.parse_args([hx, "--zero-bits", "16", "5"])[1:] == ((1 << 240) - 1, 5, U32)
    assert mine.parse_args([hx, "--zero-bits", "256", "7", "9"])[1:] == (0, 7, 9)
    assert mine.parse_args([hx, "10", str(U32)])[2:] == (10, U32)
    assert mine.target_for_zero_bits(12) == (1 << 244) - 1


@pytest.mark.parametrize("argv", [
    ["00"], [GENESIS["header"][:-2]], [GENESIS["header"] + "00"], ["zz" + GENESIS["header"][2:]],
    [GENESIS["header"], "--target", "f" * 65], [GENESIS["header"], "--target", "xyz"], [GENESIS["header"], "--target", ""],
    [GENESIS["header"], "--zero-bits", "257"], [GENESIS["header"], "--zero-bits", "-1"],
    [GENESIS["header"], "--zero-bits", "1_0"], [GENESIS["header"], "-5"], [GENESIS["header"], "0", str(U32 + 1)],
    [GENESIS["header"], "0", "x"],
    # a header whose bits field has the sign bit set, and no explicit target
    [GENESIS["header"][:144] + "ffff801d" + GENESIS["header"][152:]],
])
def test_bad_input_returns_2(argv, capsys):
    with pytest.raises(ValueError):
        mine.parse_args(argv)
    assert mine.main(argv) == 2  # rejected before any context is made
    assert capsys.readouterr().err.strip()


def test_both_target_forms_are_refused():
    with pytest.raises(SystemExit) as ei:
        mine.parse_args([GENESIS["header"], "--target", "ff", "--zero-bits", "3"])
    assert ei.value.code == 2


def test_output_lines():
    """main() prints the 64-digit hash and the nonce (a stand-in context: no GPU)."""
    class Ctx:
        def __init__(self, answer):
            self.answer, self.calls = answer, []

        def search_header(self, header, lo, hi, target):
            self.calls.append((header, lo, hi, target))
            return self.answer

    h = int(GENESIS["hash"], 16)
    c, out = Ctx((True, h, GENESIS["nonce"])), io.StringIO()
    assert mine.main([GENESIS["header"]], out=out, ctx=c) == 0
    assert out.getvalue() == ("Found 000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f "
                              "2083236893\n")
    assert c.calls == [(bytes.fromhex(GENESIS["header"]), 0, U32, int(GENESIS["target"], 16))]
    c, out = Ctx((False, 0xabc, 7)), io.StringIO()
    assert mine.main([GENESIS["header"], "--zero-bits", "250", "3", "9"], out=out, ctx=c) == 0
    assert out.getvalue() == "NotFound " + "0" * 61 + "abc 7\n"
    assert c.calls[0][1:] == (3, 9, 63)
