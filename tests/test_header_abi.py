"""The block-header search's C ABI and ctypes mirrors (no GPU):
bm_search_header_gpu / bm_header_hash_gpu / bm_header_target_from_bits are
additive, so the ABI version stays 7."""
import ctypes
import hashlib
import os
import struct
import subprocess
import tempfile

import pytest

from conftest import ROOT, load_golden
from distributed_bitcoin_minter_amd import _lib, bits_to_target

GOLDEN = load_golden("header_vectors.json")


def test_header_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_search_header_gpu", "bm_header_hash_gpu", "bm_header_target_from_bits"):
        assert hasattr(lib, name), name


def test_header_result_layout_matches_the_header():
    """Size and every field offset of bm_header_result_t, from a C program
    compiled against include/btcminer.h."""
    fields = ["hash", "nonce", "found"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(bm_header_result_t));']
    lines += [f'printf("{f} %zu\\n", offsetof(bm_header_result_t, {f}));' for f in fields]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("maxn %u\\n", BM_MAX_HEADER_HASHES);', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got["abi"] == 7
    assert got["size"] == ctypes.sizeof(_lib.HeaderResult) == 40
    assert (got["hash"], got["nonce"], got["found"]) == (0, 32, 36)
    for f in fields:
        assert got[f] == getattr(_lib.HeaderResult, f).offset, f
    assert got["maxn"] == _lib.BM_MAX_HEADER_HASHES


def test_header_argument_validation():
    lib = _lib.load()
    r = _lib.HeaderResult()
    before = bytes(r)
    fake = ctypes.c_void_p(1)  # never dereferenced: the argument checks come first
    hdr, tgt = bytes(80), bytes(32)
    assert lib.bm_search_header_gpu(None, hdr, 0, 1, tgt, ctypes.byref(r)) == _lib.BM_EINVAL
    assert lib.bm_search_header_gpu(fake, None, 0, 1, tgt, ctypes.byref(r)) == _lib.BM_EINVAL
    assert lib.bm_search_header_gpu(fake, hdr, 0, 1, None, ctypes.byref(r)) == _lib.BM_EINVAL
    assert lib.bm_search_header_gpu(fake, hdr, 0, 1, tgt, None) == _lib.BM_EINVAL
    assert bytes(r) == before
    n = (ctypes.c_uint32 * 1)(5)
    out = (ctypes.c_uint8 * 32)()
    assert lib.bm_header_hash_gpu(None, hdr, n, 1, out) == _lib.BM_EINVAL
    assert lib.bm_header_hash_gpu(fake, None, n, 1, out) == _lib.BM_EINVAL
    assert lib.bm_header_hash_gpu(fake, hdr, None, 1, out) == _lib.BM_EINVAL
    assert lib.bm_header_hash_gpu(fake, hdr, n, 1, None) == _lib.BM_EINVAL
    assert lib.bm_header_hash_gpu(fake, hdr, n, _lib.BM_MAX_HEADER_HASHES + 1, out) == _lib.BM_EINVAL
    assert lib.bm_header_target_from_bits(0x1d00ffff, None) == _lib.BM_EINVAL


def test_target_from_bits():
    assert bits_to_target(0x1d00ffff) == 0xffff << 208
    assert f"{bits_to_target(0x1d00ffff):064x}" == "00000000ffff" + "0" * 52
    assert bits_to_target(0x1a44b9f2) == 0x44b9f2 << (8 * (0x1a - 3))
    # both goldens: their hash meets their own target
    for g in GOLDEN["headers"]:
        assert f"{bits_to_target(g['bits']):064x}" == g["target"]
        assert int(g["hash"], 16) <= bits_to_target(g["bits"])
    # exponents below 3 shift right
    assert bits_to_target(0x03123456) == 0x123456
    assert bits_to_target(0x02123456) == 0x1234
    assert bits_to_target(0x01123456) == 0x12
    assert bits_to_target(0x00123456) == 0
    assert bits_to_target(0x04123456) == 0x12345600
    # the largest forms that fit
    assert bits_to_target(0x207fffff) == 0x7fffff << (8 * 29)
    assert bits_to_target(0x2100ffff) == 0xffff << (8 * 30)
    assert bits_to_target(0x220000ff) == 0xff << (8 * 31)
    assert bits_to_target(0xff000000) == 0  # a zero mantissa is zero at any exponent
    # sign bit, overflow
    for bad in (0x1d80ffff, 0x01800000, 0x21010000, 0x22000100, 0x23000001, 0xff000001):
        with pytest.raises(ValueError):
            bits_to_target(bad)
        buf = (ctypes.c_uint8 * 32)(*([7] * 32))
        assert _lib.load().bm_header_target_from_bits(bad, buf) == _lib.BM_EINVAL
        assert bytes(buf) == bytes([7] * 32)  # untouched
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            bits_to_target(bad)


def test_golden_vectors_are_hashlib():
    for g in GOLDEN["headers"]:
        header = bytes.fromhex(g["header"])
        assert len(header) == 80 and struct.unpack("<I", header[76:])[0] == g["nonce"]
        assert struct.unpack("<I", header[72:76])[0] == g["bits"]
        d = hashlib.sha256(hashlib.sha256(header).digest()).digest()
        assert d[::-1].hex() == g["hash"]


def test_python_argument_checks():
    """search_header / header_hash_many reject bad input before any call
    into the library (a stand-in handle: no GPU)."""
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._lib, ctx._h = None, None  # any library call would fail on this
    hdr = bytes(80)
    for args in ((bytes(79),), (bytes(81),), (hdr, -1), (hdr, 0, 1 << 32), (hdr, 0, 1, -1), (hdr, 0, 1, 1 << 256),
                 (hdr, 0, 1, bytes(31)), (hdr, 0, 1, "ff"), (hdr, 0.0)):
        with pytest.raises(ValueError):
            ctx.search_header(*args)
    for args in ((bytes(10), [1]), (hdr, [1 << 32]), (hdr, [-1])):
        with pytest.raises(ValueError):
            ctx.header_hash_many(*args)
