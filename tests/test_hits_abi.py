"""The hit enumeration's C ABI, ctypes mirror and CLI logic (no GPU):
bm_search_hits_gpu is additive, so the ABI version stays 7 and no existing
struct changes (tests/test_abi.py, tests/test_target_abi.py)."""
import ctypes
import io
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import _lib, shares

U64 = (1 << 64) - 1


def test_hits_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_search_hits_gpu", "bm_register_hits_kernel"):
        assert hasattr(lib, name), name
    assert pkg.HitsResult is _lib.HitsResult
    assert _lib.BM_MAX_HITS == 1 << 22


def test_hits_argument_validation():
    lib = _lib.load()
    out = _lib.HitsResult(1, 2, 3, 4)
    hits = (_lib.Result * 2)(_lib.Result(5, 6), _lib.Result(7, 8))
    fake = ctypes.c_void_p(1)  # never dereferenced: the argument checks come first
    f = lib.bm_search_hits_gpu
    o = ctypes.byref(out)
    assert f(None, b"x", 1, 0, 1, 5, hits, 2, o) == _lib.BM_EINVAL
    assert f(fake, None, 1, 0, 1, 5, hits, 2, o) == _lib.BM_EINVAL
    assert f(fake, b"x", 1, 0, 1, 5, hits, 2, None) == _lib.BM_EINVAL
    assert f(fake, b"x", (1 << 20) + 1, 0, 1, 5, hits, 2, o) == _lib.BM_EINVAL
    assert f(fake, b"x", 1, 0, 1, 5, hits, _lib.BM_MAX_HITS + 1, o) == _lib.BM_EINVAL
    assert f(fake, b"x", 1, 0, 1, 5, None, 1, o) == _lib.BM_EINVAL
    assert (out.hash, out.nonce, out.count, out.stored) == (1, 2, 3, 4)  # untouched
    assert [(h.hash, h.nonce) for h in hits] == [(5, 6), (7, 8)]


def test_hits_struct_layout_matches_the_header():
    """Size and every field offset of bm_hits_result_t, and BM_MAX_HITS, from
    a C program compiled against include/btcminer.h."""
    cname, py = "bm_hits_result_t", _lib.HitsResult
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {",
             f'printf("{cname} size %zu\\n", sizeof({cname}));']
    for f, _t in py._fields_:
        lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['printf("abi version %d\\n", BM_ABI_VERSION);', 'printf("max hits %u\\n", BM_MAX_HITS);',
              'printf("entry size %zu\\n", sizeof(bm_result_t));', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out if ln.strip()}
    assert got[("abi", "version")] == 7
    assert got[("max", "hits")] == _lib.BM_MAX_HITS == shares.MAX_CAP
    assert got[("entry", "size")] == ctypes.sizeof(_lib.Result) == 16
    assert got[(cname, "size")] == ctypes.sizeof(py) == 32
    for f, _t in py._fields_:
        assert got[(cname, f)] == getattr(py, f).offset, f
    assert [f for f, _t in py._fields_] == ["hash", "nonce", "count", "stored"]


def test_shares_argument_parsing():
    assert shares.parse_args(["bradfitz", "16", "0", "199999"]) == (b"bradfitz", 16, 0, 199999, 4096)
    assert shares.parse_args(["a b", "0", "7", str(U64), "--cap", "1"]) == (b"a b", 0, 7, U64, 1)
    assert shares.parse_args(["m", "64", "5", "4", "--cap", str(1 << 22)]) == (b"m", 64, 5, 4, 1 << 22)
    for argv in (["m", "65", "0", "9"], ["m", "-1", "0", "9"], ["m", "x", "0", "9"], ["m", "16", "-3", "9"],
                 ["m", "16", "0", str(U64 + 1)], ["m", "16", "1_0", "9"], ["m", "16", "0", "9", "--cap", "0"],
                 ["m", "16", "0", "9", "--cap", str((1 << 22) + 1)], ["m", "16", "0", "9", "--cap", "x"]):
        with pytest.raises(ValueError):
            shares.parse_args(argv)
    # rejected before any context is made; UPPER is required
    assert shares.main(["m", "65", "0", "9"]) == 2
    assert shares.main(["m", "16", "0", "9", "--cap", "0"]) == 2
    with pytest.raises(SystemExit) as ei:
        shares.parse_args(["m", "16", "0"])
    assert ei.value.code == 2


class _Ctx:
    """A stand-in context: hits are the given (hash, nonce) pairs, the range's
    minimum is taken over `floor` (hash per nonce) where given."""

    def __init__(self, hits, mins):
        self.hits, self.mins, self.calls = sorted(hits, key=lambda e: e[1]), mins, []

    def search_hits(self, msg, lo, hi, target, cap):
        self.calls.append((lo, hi, target, cap))
        got = [(h, n) for h, n in self.hits if lo <= n <= hi]
        assert all(h <= target for h, _ in got)
        low = min([m for m in self.mins if lo <= m[1] <= hi], default=(U64, U64))
        return len(got), (got if len(got) <= cap else None), low


def test_shares_steps_halving_and_merge():
    """enumerate_hits() walks the range in steps, halves a step that
    overflows and rescans both halves, returns the hits ascending and the
    lexicographic min of the pieces' minima (a stand-in context: no GPU)."""
    T = shares.target_for_bits(60)
    hits = [(9, 3), (4, 11), (2, 12), (7, 13), (4, 17), (15, 25)]
    mins = hits + [(20, 0), (30, 29)]
    c = _Ctx(hits, mins)
    got, best = shares.enumerate_hits(c, b"m", 60, 0, 29, cap=2, step=10)
    assert got == sorted(hits, key=lambda e: e[1])
    assert [n for _, n in got] == sorted(n for _, n in got)
    assert best == (2, 12)
    # step 2 holds 4 hits > cap 2: halved into [10, 14] (3 hits: halved again) and [15, 19]
    assert c.calls == [(0, 9, T, 2), (10, 19, T, 2), (10, 14, T, 2), (10, 12, T, 2), (13, 14, T, 2),
                       (15, 19, T, 2), (20, 29, T, 2)]
    # a tie on the hash: the lower nonce is the minimum
    c = _Ctx([(4, 11), (4, 17)], [(4, 17), (4, 11)])
    assert shares.enumerate_hits(c, b"m", 60, 10, 19, cap=4, step=10) == ([(4, 11), (4, 17)], (4, 11))
    assert len(c.calls) == 1
    # the top of the nonce space, an empty range, a single nonce that overflows nothing
    c = _Ctx([(5, U64)], [(5, U64)])
    assert shares.enumerate_hits(c, b"m", 60, U64 - 3, U64) == ([(5, U64)], (5, U64))
    assert c.calls == [(U64 - 3, U64, T, 4096)]
    assert shares.enumerate_hits(_Ctx([], []), b"m", 1, 5, 4) == ([], (U64, U64))
    # every nonce a hit with cap 1: down to single nonces, each exactly once
    dense = [(n % 7, n) for n in range(8)]
    c = _Ctx(dense, dense)
    got, best = shares.enumerate_hits(c, b"m", 60, 0, 7, cap=1, step=8)
    assert got == dense and best == (0, 0)


def test_shares_output_lines():
    """main()'s lines, with the context replaced by the stand-in."""
    hits = [(9, 3), (2, 12)]
    buf = io.StringIO()
    c = _Ctx(hits, hits)
    assert shares.main(["m", "60", "0", "29", "--cap", "1"], out=buf, ctx=c) == 0
    assert buf.getvalue() == "Share 9 3\nShare 2 12\nShares 2 Min 2 12\n"
    T = shares.target_for_bits(60)  # [0, 29] and then [0, 14] hold both hits
    assert c.calls == [(0, 29, T, 1), (0, 14, T, 1), (0, 7, T, 1), (8, 14, T, 1), (15, 29, T, 1)]
    buf = io.StringIO()
    assert shares.main(["m", "60", "5", "4"], out=buf, ctx=_Ctx([], [])) == 0
    assert buf.getvalue() == f"Shares 0 Min {U64} {U64}\n"
