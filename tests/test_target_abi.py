"""The target search's C ABI, ctypes mirrors and CLI arguments (no GPU):
bm_search_target_gpu / bm_ctx_last_target_stats are additive, so the ABI
version stays 7 and bm_stats_t keeps its layout (tests/test_abi.py)."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
from distributed_bitcoin_minter_amd import _lib, pow as powcli

U64 = (1 << 64) - 1


def test_target_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_search_target_gpu", "bm_ctx_last_target_stats", "bm_register_target_kernel"):
        assert hasattr(lib, name), name


def test_target_argument_validation():
    lib = _lib.load()
    r = _lib.TargetResult(1, 2, 3, 4)
    ts = _lib.TargetStats()
    fake = ctypes.c_void_p(1)  # never dereferenced: the argument checks come first
    assert lib.bm_search_target_gpu(None, b"x", 1, 0, 1, 5, ctypes.byref(r)) == _lib.BM_EINVAL
    assert lib.bm_search_target_gpu(fake, b"x", 1, 0, 1, 5, None) == _lib.BM_EINVAL
    assert lib.bm_search_target_gpu(fake, None, 1, 0, 1, 5, ctypes.byref(r)) == _lib.BM_EINVAL
    assert lib.bm_search_target_gpu(fake, b"x", (1 << 20) + 1, 0, 1, 5, ctypes.byref(r)) == _lib.BM_EINVAL
    assert (r.hash, r.nonce, r.found, r.reserved) == (1, 2, 3, 4)  # untouched
    assert lib.bm_ctx_last_target_stats(None, ctypes.byref(ts)) == _lib.BM_EINVAL
    assert lib.bm_ctx_last_target_stats(fake, None) == _lib.BM_EINVAL


def test_target_struct_layouts_match_the_header():
    """Sizes and every field offset of the two new structs, from a C program
    compiled against include/btcminer.h."""
    structs = {"bm_target_result_t": _lib.TargetResult, "bm_target_stats_t": _lib.TargetStats}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _t in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['printf("abi version %d\\n", BM_ABI_VERSION);', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out if ln.strip()}
    assert got[("abi", "version")] == 7
    for cname, py in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f, _t in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert ctypes.sizeof(_lib.TargetResult) == 24
    assert ctypes.sizeof(_lib.TargetStats) == 8 + 8 * _lib.BM_MAX_STAT_DEVICES + 8


def test_pow_target_arithmetic():
    assert powcli.target_for_bits(0) == U64
    assert powcli.target_for_bits(1) == (1 << 63) - 1
    assert powcli.target_for_bits(16) == (1 << 48) - 1
    assert powcli.target_for_bits(63) == 1
    assert powcli.target_for_bits(64) == 0
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            powcli.target_for_bits(bad)
    # BITS leading zero bits <=> hash <= target
    for bits in (1, 16, 40, 64):
        t = powcli.target_for_bits(bits)
        assert t >> (64 - bits) == 0 and (t + 1) >> (64 - bits) == 1


def test_pow_argument_parsing():
    assert powcli.parse_args(["bradfitz", "0"]) == (b"bradfitz", 0, 0, U64)
    assert powcli.parse_args(["bradfitz", "64", "5"]) == (b"bradfitz", 64, 5, U64)
    assert powcli.parse_args(["a b", "16", "7", "99999"]) == (b"a b", 16, 7, 99999)
    assert powcli.parse_args(["m", "16", "0", str(U64)])[3] == U64
    for argv in (["m", "65"], ["m", "-1"], ["m", "x"], ["m", "16", "-3"], ["m", "16", "0", str(U64 + 1)],
                 ["m", "16", "1_0"]):
        with pytest.raises(ValueError):
            powcli.parse_args(argv)
    assert powcli.main(["m", "65"]) == 2  # rejected before any context is made


def test_pow_steps_and_merge():
    """search() walks the range in steps, stops at the first hit and merges
    the not-found minima lexicographically (a stand-in context: no GPU)."""
    class Ctx:
        def __init__(self, answers):
            self.answers, self.calls = answers, []

        def search_target(self, msg, lo, hi, target):
            self.calls.append((lo, hi, target))
            return self.answers[len(self.calls) - 1]

    c = Ctx([(False, 9, 3), (False, 7, 14), (False, 7, 12)])
    assert powcli.search(c, b"m", 60, 0, 29, step=10) == (False, 7, 12)
    assert c.calls == [(0, 9, 15), (10, 19, 15), (20, 29, 15)]
    c = Ctx([(False, 9, 3), (True, 2, 14), (True, 1, 25)])
    assert powcli.search(c, b"m", 60, 0, 29, step=10) == (True, 2, 14)
    assert len(c.calls) == 2
    c = Ctx([(False, 5, U64)])
    assert powcli.search(c, b"m", 64, U64 - 3, U64, step=1 << 32) == (False, 5, U64)
    assert c.calls == [(U64 - 3, U64, 0)]
    assert powcli.search(Ctx([]), b"m", 1, 5, 4) == (False, U64, U64)
