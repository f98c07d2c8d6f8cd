"""The version-rolling header search's C ABI, ctypes mirror, roll_versions and
the mine_versions command line (no GPU): bm_search_header_versions_gpu is
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
from distributed_bitcoin_minter_amd import _lib, mine_versions, roll_versions

BUILD = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc", "build")
GENESIS_HEX = next(g for g in load_golden("header_vectors.json")["headers"] if g["name"] == "genesis")["header"]
FIELDS = ["hash", "nonce", "version_index", "version", "found"]


def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_search_header_versions_gpu", "bm_register_header_versions_kernel"):
        assert hasattr(lib, name), name
    assert pkg.HeaderVersionsResult is _lib.HeaderVersionsResult and pkg.roll_versions is _lib.roll_versions
    assert {"HeaderVersionsResult", "roll_versions"} <= set(pkg.__all__)
    assert hasattr(_lib.Context, "search_header_versions")


def test_struct_layout_matches_the_header():
    """Size and every field offset of bm_header_versions_result_t, from a C
    program compiled against include/btcminer.h."""
    name = "bm_header_versions_result_t"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {",
             f'printf("size %zu\\n", sizeof({name}));']
    lines += [f'printf("{f} %zu\\n", offsetof({name}, {f}));' for f in FIELDS]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("max %d\\n", BM_MAX_HEADER_VERSIONS);', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got["abi"] == 7 and got["max"] == _lib.BM_MAX_HEADER_VERSIONS == 64
    assert got["size"] == ctypes.sizeof(_lib.HeaderVersionsResult) == 48
    assert [got[f] for f in FIELDS] == [0, 32, 36, 40, 44]
    for f in FIELDS:
        assert got[f] == getattr(_lib.HeaderVersionsResult, f).offset, f


def test_argument_validation():
    lib = _lib.load()
    f = lib.bm_search_header_versions_gpu
    r = _lib.HeaderVersionsResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    before = bytes(r)
    fake = ctypes.c_void_p(1)  # never dereferenced: the argument checks come first
    hdr, tgt, out = bytes(80), bytes(32), ctypes.byref(r)
    vers = (ctypes.c_uint32 * 65)(*range(65))
    assert f(None, hdr, vers, 4, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert f(fake, None, vers, 4, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert f(fake, hdr, None, 4, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 4, 0, 1, None, out) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 4, 0, 1, tgt, None) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 0, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert f(fake, hdr, vers, 65, 0, 1, tgt, out) == _lib.BM_EINVAL
    assert bytes(r) == before


def test_roll_versions():
    base = 0x20000000
    assert roll_versions(base, 1) == [base]
    assert roll_versions(base, 0) == []
    # the default mask 0x1fffe000: its lowest bit is bit 13
    assert roll_versions(base, 4) == [0x20000000, 0x20002000, 0x20004000, 0x20006000]
    assert roll_versions(base, 2)[1] == base | 1 << 13
    assert roll_versions(1, 3) == [1, 0x2001, 0x4001]
    # index 2^16 - 1 fills the mask; bits of the base under the mask are replaced
    assert roll_versions(base, 1 << 16)[-1] == 0x3fffe000
    assert roll_versions(0xffffffff, 2) == [0xe0001fff, 0xe0003fff]
    # a sparse mask: bits 0, 4 and 31, lowest first
    assert roll_versions(0, 8, 0x80000011) == [0, 1, 0x10, 0x11, 0x80000000, 0x80000001, 0x80000010, 0x80000011]
    assert roll_versions(0x0f0, 4, 0x110) == [0x0e0, 0x0f0, 0x1e0, 0x1f0]
    assert roll_versions(7, 1, 0) == [7]
    # more than the mask holds
    for args in ((0, 9, 0x80000011), (0, 2, 0), (0, (1 << 16) + 1)):
        with pytest.raises(ValueError):
            roll_versions(*args)
    for args in ((-1, 1), (1 << 32, 1), (0, -1), (0, 1, 1 << 32), (0, 1.0), (0, True), ("0", 1)):
        with pytest.raises(ValueError):
            roll_versions(*args)


def test_python_argument_checks():
    """search_header_versions rejects bad input before any call into the
    library (a stand-in handle: no GPU)."""
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._lib, ctx._h = None, None  # any library call would fail on this
    hdr = bytes(80)
    for args in ((bytes(79), [1]), (hdr, []), (hdr, list(range(65))), (hdr, [-1]), (hdr, [1 << 32]), (hdr, [1.0]),
                 (hdr, [True]), (hdr, [1], -1), (hdr, [1], 0, 1 << 32), (hdr, [1], 0, 1, -1), (hdr, [1], 0, 1, 1 << 256),
                 (hdr, [1], 0, 1, bytes(31)), (hdr, [1], True)):
        with pytest.raises(ValueError):
            ctx.search_header_versions(*args)


def test_mine_versions_parse_args():
    ok = mine_versions.parse_args([GENESIS_HEX, "--versions", "4", "--zero-bits", "12", "0", "65535"])
    assert ok == (bytes.fromhex(GENESIS_HEX), [1, 0x2001, 0x4001, 0x6001], (1 << 244) - 1, 0, 65535)
    header, versions, target, lo, hi = mine_versions.parse_args([GENESIS_HEX, "--versions", "2", "--mask", "0x30"])
    assert versions == [1, 0x11] and (lo, hi) == (0, (1 << 32) - 1) and target == _lib.bits_to_target(0x1d00ffff)
    bad = [
        [GENESIS_HEX[:-2], "--versions", "4"],                 # a short header
        [GENESIS_HEX, "--versions", "0"],
        [GENESIS_HEX, "--versions", "65"],
        [GENESIS_HEX, "--versions", "four"],
        [GENESIS_HEX, "--versions", "4", "--mask", "xyz"],
        [GENESIS_HEX, "--versions", "4", "--mask", "100000000"],  # 33 bits
        [GENESIS_HEX, "--versions", "4", "--mask", "2000"],        # the mask holds 2 versions
        [GENESIS_HEX, "--versions", "4", "--zero-bits", "257"],
        [GENESIS_HEX, "--versions", "4", "--target", "zz"],
        [GENESIS_HEX, "--versions", "4", "-1"],
        [GENESIS_HEX, "--versions", "4", "0", "4294967296"],
    ]
    for argv in bad:
        with pytest.raises((ValueError, SystemExit)):
            mine_versions.parse_args(argv)
        assert mine_versions.main(argv) == 2, argv
    with pytest.raises(SystemExit):  # --versions is required
        mine_versions.parse_args([GENESIS_HEX])
    assert mine_versions.main([GENESIS_HEX]) == 2


def test_host_half_under_sanitizers():
    """The precompute, the key, the grouping and the host's selection in a
    stand-alone program of its own (tools/header_versions_check.cpp), built with
    ASan and UBSan and run on the CPU."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "header_versions_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc"),
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "header_versions_check.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("header versions check ok")


def _rows(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_inner.py"), BUILD, *flags, "-v"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout


def _field(row, key):
    return float(row.split(key + "=")[1].split()[0])


def test_shared_schedule_costs_less_per_hash():
    """The built header_versions_kernel<M>: no scratch or memory operation in
    the per-nonce code, and for M = 2 and 4 fewer VALU ops and fewer issue
    slots per hash than M = 1 (the kernel bm_search_header_gpu runs) in the
    same build (tools/check_inner.py --header-versions)."""
    if not glob.glob(os.path.join(BUILD, "bm_header_versions_inst-hip-amdgcn-amd-amdhsa-gfx950.s")):
        pytest.skip("device assembly not built (make -C distributed_bitcoin_minter_amd/csrc)")
    out = _rows("--header-versions")
    assert "3 kernels checked, 0 with scratch" in out, out[-500:]
    hdr = next(ln for ln in out.splitlines() if ":hdrv1 " in ln)
    hdr_valu = _field(hdr, "VALU")
    hdr_slots = _field(hdr, "slots/hash")  # max(slow, (slow + fast) / 2)
    assert 2000 < hdr_valu < 3000, hdr  # two 61-round passes, about 21 ops a round
    for m in (1, 2, 4):
        row = next(ln for ln in out.splitlines() if f":hdrv{m} " in ln)
        print(row)
        assert "mem=0" in row, row
        assert _field(row, "VALU") == pytest.approx(_field(row, "VALU/hash") * m, abs=m)
        if m > 1:
            assert _field(row, "VALU/hash") < hdr_valu, (row, hdr)
            assert _field(row, "slots/hash") < hdr_slots, (row, hdr)
    with open(os.path.join(BUILD, "bm_header_versions_inst.res")) as f:
        res = f.read()
    assert res.count("header_versions_kernel") >= 3 and res.count("ScratchSize [bytes/lane]: 0") >= 3, res[-1500:]
