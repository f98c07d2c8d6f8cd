"""The block-header share enumeration's C ABI and ctypes mirrors (no GPU):
bm_search_header_hits_gpu is additive, so the ABI version stays 7."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import _lib


def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_search_header_hits_gpu",):
        assert hasattr(lib, name), name
    assert pkg.HeaderHit is _lib.HeaderHit and pkg.HeaderHitsResult is _lib.HeaderHitsResult
    assert {"HeaderHit", "HeaderHitsResult"} <= set(pkg.__all__)


def test_struct_layouts_match_the_header():
    """Size and every field offset of bm_header_hit_t and
    bm_header_hits_result_t, from a C program compiled against
    include/btcminer.h."""
    structs = {"bm_header_hit_t": (_lib.HeaderHit, ["hash", "nonce", "reserved"]),
               "bm_header_hits_result_t": (_lib.HeaderHitsResult, ["hash", "nonce", "reserved", "count", "stored"])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name}.size %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("max %u\\n", BM_MAX_HEADER_HITS);', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got["abi"] == 7 and got["max"] == _lib.BM_MAX_HEADER_HITS == 1 << 20
    assert got["bm_header_hit_t.size"] == ctypes.sizeof(_lib.HeaderHit) == 40
    assert got["bm_header_hits_result_t.size"] == ctypes.sizeof(_lib.HeaderHitsResult) == 56
    assert [got[f"bm_header_hit_t.{f}"] for f in structs["bm_header_hit_t"][1]] == [0, 32, 36]
    assert [got[f"bm_header_hits_result_t.{f}"] for f in structs["bm_header_hits_result_t"][1]] == [0, 32, 36, 40, 48]
    for name, (mirror, fields) in structs.items():
        for f in fields:
            assert got[f"{name}.{f}"] == getattr(mirror, f).offset, (name, f)


def test_argument_validation():
    lib = _lib.load()
    f = lib.bm_search_header_hits_gpu
    r = _lib.HeaderHitsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    buf = (_lib.HeaderHit * 2)()
    ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
    before = bytes(r), bytes(buf)
    fake = ctypes.c_void_p(1)  # never dereferenced: the argument checks come first
    hdr, tgt, out = bytes(80), bytes(32), ctypes.byref(r)
    assert f(None, hdr, 0, 1, tgt, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, None, 0, 1, tgt, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, hdr, 0, 1, None, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, hdr, 0, 1, tgt, buf, 2, None) == _lib.BM_EINVAL
    assert f(fake, hdr, 0, 1, tgt, None, 2, out) == _lib.BM_EINVAL  # no buffer for cap > 0
    assert f(fake, hdr, 0, 1, tgt, buf, _lib.BM_MAX_HEADER_HITS + 1, out) == _lib.BM_EINVAL
    assert f(fake, hdr, 0, 1, tgt, None, _lib.BM_MAX_HEADER_HITS + 1, out) == _lib.BM_EINVAL
    assert (bytes(r), bytes(buf)) == before


def test_python_argument_checks():
    """search_header_hits rejects bad input before any call into the library
    (a stand-in handle: no GPU)."""
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._lib, ctx._h = None, None  # any library call would fail on this
    hdr = bytes(80)
    for args in ((bytes(79),), (bytes(81),), (hdr, -1), (hdr, 0, 1 << 32), (hdr, 0, 1, -1), (hdr, 0, 1, 1 << 256),
                 (hdr, 0, 1, bytes(31)), (hdr, 0, 1, "ff"), (hdr, 0.0), (hdr, 0, 1, 0, -1),
                 (hdr, 0, 1, 0, _lib.BM_MAX_HEADER_HITS + 1), (hdr, 0, 1, 0, 1.5), (hdr, 0, 1, 0, None),
                 (hdr, True), (hdr, 0, 1, 0, True)):
        with pytest.raises(ValueError):
            ctx.search_header_hits(*args)


def test_collect_under_sanitizers():
    """host::header_versions_hits_collect with bm_header_hit_t output over one
    version, the host half of this call, in a stand-alone program
    (tools/header_versions_hits_check.cpp, its one-version cases), built with
    ASan and UBSan and run on the CPU."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "header_versions_hits_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc"),
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "header_versions_hits_check.cpp"), "-o", exe])
        r = subprocess.run([exe, "--one-version"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("header hits check ok")
