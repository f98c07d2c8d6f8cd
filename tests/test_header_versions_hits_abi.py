"""The version-rolling share enumeration's C ABI, ctypes mirrors, host half and
the version_shares command line (no GPU): bm_search_header_versions_hits_gpu is
additive, so the ABI version stays 7."""
import ctypes
import glob
import os
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT, load_golden
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import _lib, version_shares

BUILD = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc", "build")
GENESIS_HEX = next(g for g in load_golden("header_vectors.json")["headers"] if g["name"] == "genesis")["header"]
HIT_FIELDS = ["hash", "nonce", "version_index", "version", "reserved"]
RESULT_FIELDS = HIT_FIELDS + ["count", "stored"]


def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_search_header_versions_hits_gpu", "bm_register_header_versions_hits_kernel"):
        assert hasattr(lib, name), name
    assert pkg.HeaderVersionHit is _lib.HeaderVersionHit
    assert pkg.HeaderVersionsHitsResult is _lib.HeaderVersionsHitsResult
    assert {"HeaderVersionHit", "HeaderVersionsHitsResult"} <= set(pkg.__all__)
    assert hasattr(_lib.Context, "search_header_versions_hits")


def test_struct_layouts_match_the_header():
    """Size and every field offset of bm_header_version_hit_t and
    bm_header_versions_hits_result_t, from a C program compiled against
    include/btcminer.h."""
    structs = {"bm_header_version_hit_t": (_lib.HeaderVersionHit, HIT_FIELDS),
               "bm_header_versions_hits_result_t": (_lib.HeaderVersionsHitsResult, RESULT_FIELDS)}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name}.size %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("max %u\\n", BM_MAX_HEADER_HITS);',
              'printf("maxv %d\\n", BM_MAX_HEADER_VERSIONS);', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got["abi"] == 7 and got["max"] == _lib.BM_MAX_HEADER_HITS == 1 << 20 and got["maxv"] == 64
    assert got["bm_header_version_hit_t.size"] == ctypes.sizeof(_lib.HeaderVersionHit) == 48
    assert got["bm_header_versions_hits_result_t.size"] == ctypes.sizeof(_lib.HeaderVersionsHitsResult) == 64
    assert [got[f"bm_header_version_hit_t.{f}"] for f in HIT_FIELDS] == [0, 32, 36, 40, 44]
    assert [got[f"bm_header_versions_hits_result_t.{f}"] for f in RESULT_FIELDS] == [0, 32, 36, 40, 44, 48, 56]
    for name, (mirror, fields) in structs.items():
        for f in fields:
            assert got[f"{name}.{f}"] == getattr(mirror, f).offset, (name, f)


def test_argument_validation():
    lib = _lib.load()
    f = lib.bm_search_header_versions_hits_gpu
    r = _lib.HeaderVersionsHitsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    buf = (_lib.HeaderVersionHit * 2)()
    ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
    before = bytes(r), bytes(buf)
    fake = ctypes.c_void_p(1)  # never dereferenced: the argument checks come first
    hdr, tgt, out = bytes(80), bytes(32), ctypes.byref(r)
    vers = (ctypes.c_uint32 * 65)(*range(65))
    assert f(None, hdr, vers, 4, 0, 1, tgt, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, None, vers, 4, 0, 1, tgt, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, hdr, None, 4, 0, 1, tgt, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 4, 0, 1, None, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 4, 0, 1, tgt, buf, 2, None) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 0, 0, 1, tgt, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 65, 0, 1, tgt, buf, 2, out) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 4, 0, 1, tgt, None, 2, out) == _lib.BM_EINVAL  # no buffer for cap > 0
    assert f(fake, hdr, vers, 4, 0, 1, tgt, buf, _lib.BM_MAX_HEADER_HITS + 1, out) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 4, 0, 1, tgt, None, _lib.BM_MAX_HEADER_HITS + 1, out) == _lib.BM_EINVAL
    assert (bytes(r), bytes(buf)) == before


def test_python_argument_checks():
    """search_header_versions_hits rejects bad input before any call into the
    library (a stand-in handle: no GPU)."""
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._lib, ctx._h = None, None  # any library call would fail on this
    hdr = bytes(80)
    for args in ((bytes(79), [1]), (hdr, []), (hdr, list(range(65))), (hdr, [-1]), (hdr, [1 << 32]), (hdr, [1.0]),
                 (hdr, [True]), (hdr, [1], -1), (hdr, [1], 0, 1 << 32), (hdr, [1], 0, 1, -1), (hdr, [1], 0, 1, 1 << 256),
                 (hdr, [1], 0, 1, bytes(31)), (hdr, [1], True), (hdr, [1], 0, 1, 0, -1),
                 (hdr, [1], 0, 1, 0, _lib.BM_MAX_HEADER_HITS + 1), (hdr, [1], 0, 1, 0, 1.5), (hdr, [1], 0, 1, 0, None),
                 (hdr, [1], 0, 1, 0, True)):
        with pytest.raises(ValueError):
            ctx.search_header_versions_hits(*args)


def test_version_shares_parse_args():
    ok = version_shares.parse_args([GENESIS_HEX, "--versions", "4", "--zero-bits", "12", "0", "65535"])
    assert ok == (bytes.fromhex(GENESIS_HEX), [1, 0x2001, 0x4001, 0x6001], (1 << 244) - 1, 0, 65535, 65536)
    header, versions, target, lo, hi, cap = version_shares.parse_args(
        [GENESIS_HEX, "--target", "ff", "--versions", "2", "--mask", "0x30", "--cap", "2"])
    assert versions == [1, 0x11] and (lo, hi) == (0, (1 << 32) - 1) and target == 0xff and cap == 2
    assert len(version_shares.parse_args([GENESIS_HEX, "--zero-bits", "8"])[1]) == 4  # the default
    bad = [
        [GENESIS_HEX[:-2], "--zero-bits", "8"],                       # a short header
        [GENESIS_HEX],                                                 # a target is required
        [GENESIS_HEX, "--zero-bits", "8", "--target", "ff"],
        [GENESIS_HEX, "--zero-bits", "8", "--versions", "0"],
        [GENESIS_HEX, "--zero-bits", "8", "--versions", "65"],
        [GENESIS_HEX, "--zero-bits", "8", "--versions", "four"],
        [GENESIS_HEX, "--zero-bits", "8", "--mask", "xyz"],
        [GENESIS_HEX, "--zero-bits", "8", "--mask", "100000000"],     # 33 bits
        [GENESIS_HEX, "--zero-bits", "8", "--mask", "2000"],          # the mask holds 2 versions, 4 asked for
        [GENESIS_HEX, "--zero-bits", "257"],
        [GENESIS_HEX, "--target", "zz"],
        [GENESIS_HEX, "--zero-bits", "8", "-1"],
        [GENESIS_HEX, "--zero-bits", "8", "0", "4294967296"],
        [GENESIS_HEX, "--zero-bits", "8", "--cap", "0"],
        [GENESIS_HEX, "--zero-bits", "8", "--cap", str((1 << 20) + 1)],
        [GENESIS_HEX, "--zero-bits", "8", "--cap", "3"],              # below the 4 default versions
        [GENESIS_HEX, "--zero-bits", "8", "--versions", "9", "--cap", "8"],
    ]
    for argv in bad:
        with pytest.raises((ValueError, SystemExit)):
            version_shares.parse_args(argv)
        assert version_shares.main(argv) == 2, argv
    assert version_shares.parse_args([GENESIS_HEX, "--zero-bits", "8", "--versions", "9", "--cap", "9"])[5] == 9


def test_version_shares_cli_argument_errors_exit_2():
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.version_shares", GENESIS_HEX,
                        "--zero-bits", "8", "--versions", "8", "--cap", "7"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 2 and "--cap" in r.stderr and r.stdout == ""


class _FakeContext:
    """search_header_versions_hits over a fixed set of hits, all or nothing."""

    def __init__(self, hits):
        self.hits, self.calls = sorted(hits, key=lambda s: (s[1], s[2])), []

    def search_header_versions_hits(self, header, versions, lo, hi, target, cap):
        self.calls.append((lo, hi))
        got = [s for s in self.hits if lo <= s[1] <= hi]
        best = min(got, key=lambda s: (s[0] >> 192, s[1], s[2])) if got else ((1 << 256) - 1 - lo, lo, 0)
        return len(got), (got if len(got) <= cap else None), best


def test_enumerate_hits_halves_an_over_full_piece():
    hits = [(5 << 200, 7, 0), (4 << 200, 7, 1), (6 << 200, 7, 3), (3 << 200, 100, 2), (9 << 200, 4000, 0)]
    ctx = _FakeContext(hits)
    got, best = version_shares.enumerate_hits(ctx, bytes(80), [1, 2, 3, 4], 1 << 255, 0, 4095, cap=4)
    assert got == ctx.hits and best == (3 << 200, 100, 2)
    assert ctx.calls[0] == (0, 4095) and len(ctx.calls) > 1
    assert all(a <= b for a, b in ctx.calls)
    # three hits at one nonce fit a cap of 4 (the number of versions): the halving ends
    ctx = _FakeContext(hits[:3] + [(1 << 200, 7, 2)])
    got, best = version_shares.enumerate_hits(ctx, bytes(80), [1, 2, 3, 4], 1 << 255, 0, 4095, cap=4)
    assert len(got) == 4 and best == (1 << 200, 7, 2)
    assert version_shares.enumerate_hits(ctx, bytes(80), [1], 0, 5, 4) == ([], ((1 << 256) - 1, (1 << 32) - 1, 0))


def test_host_half_under_sanitizers():
    """host::header_versions_hits_collect and header_versions_hits_best in a
    stand-alone program of its own (tools/header_versions_hits_check.cpp), built
    with ASan and UBSan and run on the CPU."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "header_versions_hits_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc"),
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "header_versions_hits_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("header versions hits check ok")


def _rows(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_inner.py"), BUILD, *flags, "-v"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout


def _field(row, key):
    return float(row.split(key + "=")[1].split()[0])


def test_hits_kernels_inner_loop_is_register_only():
    """The built header_versions_hits_kernel<M>: no scratch or memory operation
    in the per-nonce code, and for M = 2 and 4 the shared schedule still shows:
    fewer VALU ops and fewer issue slots per hash than header_versions_kernel<1>
    (the first-hit kernel of one version) in the same build, as for
    header_versions_kernel<M>; at M = 1 the hits mode costs what the first-hit
    mode does, within 1% (tools/check_inner.py --header-versions-hits)."""
    if not (glob.glob(os.path.join(BUILD, "bm_header_versions_hits_inst-hip-amdgcn-amd-amdhsa-gfx950.s")) and
            glob.glob(os.path.join(BUILD, "bm_header_versions_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        pytest.skip("device assembly not built (make -C distributed_bitcoin_minter_amd/csrc)")
    out = _rows("--header-versions-hits")
    assert "3 kernels checked, 0 with scratch" in out, out[-500:]
    hdr = next(ln for ln in _rows("--header-versions").splitlines() if ":hdrv1 " in ln)
    hdr_valu = _field(hdr, "VALU")
    hdr_slots = _field(hdr, "slots/hash")  # max(slow, (slow + fast) / 2)
    print(hdr)
    hits1 = next(ln for ln in out.splitlines() if ":hdrvh1 " in ln)
    assert abs(_field(hits1, "VALU") - hdr_valu) <= 0.01 * hdr_valu, (hits1, hdr)
    for m in (1, 2, 4):
        row = next(ln for ln in out.splitlines() if f":hdrvh{m} " in ln)
        print(row)
        assert "mem=0" in row, row
        assert _field(row, "VALU") == pytest.approx(_field(row, "VALU/hash") * m, abs=m)
        if m > 1:
            assert _field(row, "VALU/hash") < hdr_valu, (row, hdr)
            assert _field(row, "slots/hash") < hdr_slots, (row, hdr)
    # the older modes' rows are as they were: the new mode adds rows, it changes none
    assert "3 kernels checked" in _rows("--header-versions") and ":hdrvh" not in _rows("--header-versions")
    with open(os.path.join(BUILD, "bm_header_versions_hits_inst.res")) as f:
        res = f.read()
    assert res.count("header_versions_hits_kernel") >= 3 and res.count("ScratchSize [bytes/lane]: 0") >= 3, res[-1500:]
