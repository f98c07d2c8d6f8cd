"""The Stratum job layer's C ABI, ctypes mirrors and pure-CPU entries (no GPU):
bm_job_prevhash_from_stratum, bm_job_header and bm_target_from_difficulty
against hashlib and fractions.Fraction restated here, the refusals, the struct
layouts against a compiled C consumer, submit_params.  The calls are additive,
so the ABI version stays 7."""
import ctypes
import hashlib
import math
import os
import struct
import subprocess
import tempfile
from fractions import Fraction

import pytest

from conftest import ROOT, load_golden
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import Job, _lib, difficulty_to_target, submit_params

GENESIS = bytes.fromhex(next(g for g in load_golden("header_vectors.json")["headers"]
                             if g["name"] == "genesis")["header"])
JOB = load_golden("stratum_genesis_job.json")
BRANCH2 = [hashlib.sha256(b"branch 0").digest(), hashlib.sha256(b"branch 1").digest()]
DIFF1 = 0xffff << 208
U256 = (1 << 256) - 1
JOB_FIELDS = ["coinb1", "coinb1_len", "extranonce1", "extranonce1_len", "extranonce2_size", "coinb2", "coinb2_len",
              "branch", "nbranch", "prevhash", "version", "nbits"]
SHARE_FIELDS = ["hash", "extranonce2", "nonce", "ntime", "version_index", "version", "is_block", "reserved"]
RESULT_FIELDS = ["hash", "extranonce2", "nonce", "version_index", "version", "reserved", "count", "stored", "headers"]


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def header_of(coinb1, en1, en2, size, coinb2, branch, prevhash, version, ntime, nbits, nonce=0):
    """The issue's recipe, with hashlib."""
    root = sha256d(coinb1 + en1 + en2.to_bytes(size, "big") + coinb2)
    for entry in branch:
        root = sha256d(root + entry)
    return struct.pack("<I", version) + prevhash + root + struct.pack("<III", ntime, nbits, nonce)


def genesis_job(**kw):
    return Job.from_notify(kw.get("notify", JOB["notify"]), JOB["extranonce1"], JOB["extranonce2_size"])


def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_job_prevhash_from_stratum", "bm_job_header", "bm_target_from_difficulty",
                 "bm_search_job_shares_gpu"):
        assert hasattr(lib, name), name
    assert {"Job", "JobShare", "JobSharesResult", "difficulty_to_target", "submit_params"} <= set(pkg.__all__)
    assert pkg.Job is _lib.Job and pkg.JobShare is _lib.JobShare and pkg.JobSharesResult is _lib.JobSharesResult
    assert hasattr(_lib.Context, "search_job_shares")


def test_struct_layouts_match_the_header():
    """Size and every field offset of bm_job_t, bm_job_share_t and
    bm_job_shares_result_t, from a C program compiled against include/btcminer.h."""
    structs = {"bm_job_t": (_lib.JobStruct, JOB_FIELDS), "bm_job_share_t": (_lib.JobShare, SHARE_FIELDS),
               "bm_job_shares_result_t": (_lib.JobSharesResult, RESULT_FIELDS)}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name}.size %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("coinbase %u\\n", BM_MAX_JOB_COINBASE);',
              'printf("branch %d\\n", BM_MAX_JOB_BRANCH);', 'printf("headers %d\\n", BM_MAX_JOB_HEADERS);',
              "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got["abi"] == 7
    assert got["coinbase"] == _lib.BM_MAX_JOB_COINBASE == 1 << 16
    assert got["branch"] == _lib.BM_MAX_JOB_BRANCH == 32 and got["headers"] == _lib.BM_MAX_JOB_HEADERS == 4096
    assert got["bm_job_share_t.size"] == ctypes.sizeof(_lib.JobShare) == 64
    assert got["bm_job_shares_result_t.size"] == ctypes.sizeof(_lib.JobSharesResult) == 80
    assert got["bm_job_t.size"] == ctypes.sizeof(_lib.JobStruct)
    assert [got[f"bm_job_share_t.{f}"] for f in SHARE_FIELDS] == [0, 32, 40, 44, 48, 52, 56, 60]
    assert [got[f"bm_job_shares_result_t.{f}"] for f in RESULT_FIELDS] == [0, 32, 40, 44, 48, 52, 56, 64, 72]
    for name, (mirror, fields) in structs.items():
        for f in fields:
            assert got[f"{name}.{f}"] == getattr(mirror, f).offset, (name, f)


def test_prevhash_vector():
    """Block 1's notify prevhash gives the genesis header's digest, as digested."""
    sent = bytes.fromhex("0a8ce26f72b3f1b646a2a6c14ff763ae65831e939c085ae10019d66800000000")
    want = sha256d(GENESIS)
    assert want.hex().startswith("6fe28c0a") and want.hex().endswith("00000000")
    out = (ctypes.c_uint8 * 32)()
    assert _lib.load().bm_job_prevhash_from_stratum(sent, out) == _lib.BM_OK
    assert bytes(out) == want == b"".join(sent[i:i + 4][::-1] for i in range(0, 32, 4))
    notify = list(JOB["notify"])
    notify[1] = sent.hex()
    assert genesis_job(notify=notify).prevhash == want
    assert _lib.load().bm_job_prevhash_from_stratum(None, out) == _lib.BM_EINVAL
    assert _lib.load().bm_job_prevhash_from_stratum(sent, None) == _lib.BM_EINVAL


def test_genesis_job_reproduces_the_genesis_header():
    job = genesis_job()
    tx = job.coinb1 + job.extranonce1 + (29).to_bytes(2, "big") + job.coinb2
    assert len(tx) == 204 and len(job.coinb1) == 43 and job.coinb1.hex().endswith("ffffffff4d04")
    assert sha256d(tx) == GENESIS[36:68]
    assert (job.version, job.nbits, job.ntime, job.job_id) == (1, 0x1d00ffff, 0x495fab29, "genesis")
    assert job.header(29, nonce=2083236893) == GENESIS
    assert job.header(29) == GENESIS[:76] + bytes(4)
    # another extranonce2, ntime and version change the root, the time and the version fields only
    h = job.header(30, ntime=0x495fab2a, version=0x20002000, nonce=7)
    assert h == header_of(job.coinb1, job.extranonce1, 30, 2, job.coinb2, [], bytes(32), 0x20002000, 0x495fab2a,
                          0x1d00ffff, 7)
    assert h[4:36] == GENESIS[4:36] and h[36:68] != GENESIS[36:68]


def test_branch_fold_order():
    notify = list(JOB["notify"])
    notify[4] = [b.hex() for b in BRANCH2]
    job = genesis_job(notify=notify)
    for en2 in (0, 28, 29, 30, 0xffff):
        want = header_of(job.coinb1, job.extranonce1, en2, 2, job.coinb2, BRANCH2, bytes(32), 1, 0x495fab29, 0x1d00ffff)
        assert job.header(en2) == want, en2
    # the fold is root || entry, in the order sent: the reverse order is another root
    notify[4] = notify[4][::-1]
    assert genesis_job(notify=notify).header(29) != job.header(29)


@pytest.mark.parametrize("size", range(1, 9))
def test_every_extranonce2_size(size):
    """Coinbase lengths on both sides of the 64-byte block edges, 0 to 3 branch entries."""
    for total, nbranch in ((55, 0), (56, 1), (63, 2), (64, 3), (65, 0), (119, 1), (120, 2), (300, 3)):
        body = hashlib.shake_128(bytes([size, total % 251])).digest(total - size + 32 * nbranch + 32)
        en1_len = size % 3
        rest = total - size - en1_len
        coinb1, en1 = body[:rest // 2], body[rest // 2:rest // 2 + en1_len]
        coinb2 = body[rest // 2 + en1_len:rest + en1_len]
        tail = body[rest + en1_len:]
        branch = [tail[32 * i:32 * i + 32] for i in range(nbranch)]
        prevhash = tail[32 * nbranch:32 * nbranch + 32]
        job = Job(coinb1, en1, size, coinb2, branch, prevhash, 0x20000000, 0x1715a35c, 0x60000000)
        top = (1 << (8 * size)) - 1
        for en2 in (0, 1, top - 1, top, 0x0102030405060708 & top):
            want = header_of(coinb1, en1, en2, size, coinb2, branch, prevhash, 0x20000000, 0x60000000, 0x1715a35c)
            assert job.header(en2) == want, (size, total, en2)
        with pytest.raises(ValueError):
            job.header(top + 1)
        buf = (ctypes.c_uint8 * 80)(*([0xA5] * 80))
        if size < 8:
            assert _lib.load().bm_job_header(ctypes.byref(job.struct), top + 1, 0, 0, buf) == _lib.BM_EINVAL
            assert bytes(buf) == b"\xa5" * 80


def floor_target(d):
    """floor(diff1 / d) for the float's exact rational value, saturated."""
    return min(U256, math.floor(Fraction(DIFF1) / Fraction(d)))


def test_difficulty_to_target_is_exact():
    assert difficulty_to_target(1.0) == difficulty_to_target(1) == DIFF1 == _lib.bits_to_target(0x1d00ffff)
    assert difficulty_to_target(65536.0) == 0xffff << 192
    values = [1.0, 65536.0, 0.001, 0.3, 2.0 ** -40, 1e-30, 3.0, 7.0, 1 / 3, 1e-3, 0.5, 2.0, 1e6, 123456.789, 2.0 ** 52 + 1,
              1e15, 8.7e13, 65535 * 2.0 ** -48, math.nextafter(65535 * 2.0 ** -48, 1.0),
              math.nextafter(65535 * 2.0 ** -48, 0.0), 65535 * 2.0 ** 208, math.nextafter(65535 * 2.0 ** 208, math.inf),
              2.0 ** 223, 2.0 ** 224, 1e300, 1.7976931348623157e308, 5e-324, 2.2250738585072014e-308, 1e-310]
    values += [2.0 ** k for k in range(-60, 240, 7)]
    values += [struct.unpack("<d", hashlib.sha256(bytes([i])).digest()[:8])[0] for i in range(64)]
    checked = 0
    for d in values:
        if not (math.isfinite(d) and d > 0):
            continue  # a hashed bit pattern that is no positive finite double
        assert difficulty_to_target(d) == floor_target(d), d
        checked += 1
    assert checked > 80
    # the issue's list, recomputed above and pinned here
    assert difficulty_to_target(0.001) == 0x3e7fc17fffffffa2405dc00000008c9f735fffffff2d10d2f00000013c6 == floor_target(0.001)
    assert difficulty_to_target(0.3) == 0x355520000000008e385555555556d09638e38e38e7819097b425ed140 == floor_target(0.3)
    assert difficulty_to_target(2.0 ** -40) == difficulty_to_target(1e-30) == U256
    for bad in (0.0, -0.0, -1.0, math.nan, math.inf, -math.inf, "1", None, True, 10 ** 400):
        with pytest.raises(ValueError):
            difficulty_to_target(bad)
    buf = (ctypes.c_uint8 * 32)(*([0xA5] * 32))
    f = _lib.load().bm_target_from_difficulty
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert f(bad, buf) == _lib.BM_EINVAL
    assert f(1.0, None) == _lib.BM_EINVAL
    assert bytes(buf) == b"\xa5" * 32


def test_job_header_refusals():
    f = _lib.load().bm_job_header
    good = Job(b"\x01" * 10, b"\x02" * 4, 4, b"\x03" * 20, [bytes(32)] * 2)
    buf = (ctypes.c_uint8 * 80)(*([0xA5] * 80))
    assert f(ctypes.byref(good.struct), 1, 2, 3, buf) == _lib.BM_OK
    buf = (ctypes.c_uint8 * 80)(*([0xA5] * 80))

    def variant(**kw):
        s = _lib.JobStruct.from_buffer_copy(bytes(good.struct))
        for k, v in kw.items():
            setattr(s, k, v)
        return ctypes.byref(s)

    assert f(None, 1, 2, 3, buf) == _lib.BM_EINVAL
    assert f(ctypes.byref(good.struct), 1, 2, 3, None) == _lib.BM_EINVAL
    for field in ("coinb1", "extranonce1", "coinb2", "branch"):
        assert f(variant(**{field: None}), 1, 2, 3, buf) == _lib.BM_EINVAL, field
    assert f(variant(extranonce2_size=0), 0, 2, 3, buf) == _lib.BM_EINVAL
    assert f(variant(extranonce2_size=9), 0, 2, 3, buf) == _lib.BM_EINVAL
    assert f(variant(nbranch=33), 0, 2, 3, buf) == _lib.BM_EINVAL
    assert f(variant(coinb2_len=(1 << 16) - 17), 0, 2, 3, buf) == _lib.BM_EINVAL   # 65537 bytes (never read)
    assert f(variant(coinb1_len=(1 << 64) - 1), 0, 2, 3, buf) == _lib.BM_EINVAL     # the sum would wrap
    assert f(ctypes.byref(good.struct), 1 << 32, 2, 3, buf) == _lib.BM_EINVAL
    assert bytes(buf) == b"\xa5" * 80
    # NULL pointers with zero lengths are legal
    assert f(variant(coinb1=None, coinb1_len=0, extranonce1=None, extranonce1_len=0, coinb2=None, coinb2_len=0,
                     branch=None, nbranch=0), 5, 2, 3, buf) == _lib.BM_OK
    assert bytes(buf) == header_of(b"", b"", 5, 4, b"", [], bytes(32), 3, 2, 0)
    # a coinbase of exactly the limit is legal
    big = Job(b"\x07" * 40000, b"", 8, b"\x09" * ((1 << 16) - 40008))
    assert big.header(5) == header_of(big.coinb1, b"", 5, 8, big.coinb2, [], bytes(32), 0, 0, 0)


def test_python_job_checks():
    for args in ((b"", b"", 0, b""), (b"", b"", 9, b""), (b"", b"", True, b""), (b"", b"", 4, b"", [bytes(31)]),
                 (b"", b"", 4, b"", [bytes(32)] * 33), (b"", b"", 4, b"", [], bytes(31)),
                 (bytes(1 << 16), b"", 1, b""), (b"", b"", 4, b"", [], bytes(32), 1 << 32)):
        with pytest.raises(ValueError):
            Job(*args)
    n = JOB["notify"]
    for bad in (n[:8], n[:1] + ["zz" * 32] + n[2:], n[:1] + ["00" * 31] + n[2:], n[:2] + ["0g"] + n[3:],
                n[:4] + ["00" * 32] + n[5:], n[:4] + [["00" * 31]] + n[5:], n[:5] + ["1"] + n[6:],
                n[:5] + [1] + n[6:]):
        with pytest.raises(ValueError):
            Job.from_notify(bad, "ffff", 2)
    with pytest.raises(ValueError):
        Job.from_notify(n, "fff", 2)
    job = genesis_job()
    for args in ((-1,), (1 << 16,), (1.0,), (True,), (0, -1), (0, 1 << 32), (0, None, 1 << 32), (0, None, None, 1 << 32)):
        with pytest.raises(ValueError):
            job.header(*args)


def test_search_job_shares_argument_validation():
    """Every refusal comes before anything is dereferenced (a stand-in context pointer)."""
    f = _lib.load().bm_search_job_shares_gpu
    r = _lib.JobSharesResult()
    ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    buf = (_lib.JobShare * 2)()
    ctypes.memset(buf, 0x5A, ctypes.sizeof(buf))
    before = bytes(r), bytes(buf)
    fake = ctypes.c_void_p(1)
    job = genesis_job()
    j, tgt, out = ctypes.byref(job.struct), bytes(32), ctypes.byref(r)
    vers = (ctypes.c_uint32 * 65)(*range(65))
    size8 = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
    size8.extranonce2_size = 8
    size9 = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
    size9.extranonce2_size = 9
    E = _lib.BM_EINVAL
    assert f(None, j, 0, 0, 1, vers, 4, 0, 1, tgt, buf, 2, out) == E
    assert f(fake, None, 0, 0, 1, vers, 4, 0, 1, tgt, buf, 2, out) == E
    assert f(fake, j, 0, 0, 1, None, 4, 0, 1, tgt, buf, 2, out) == E
    assert f(fake, j, 0, 0, 1, vers, 4, 0, 1, None, buf, 2, out) == E
    assert f(fake, j, 0, 0, 1, vers, 4, 0, 1, tgt, buf, 2, None) == E
    assert f(fake, j, 0, 0, 1, vers, 0, 0, 1, tgt, buf, 2, out) == E
    assert f(fake, j, 0, 0, 1, vers, 65, 0, 1, tgt, buf, 2, out) == E
    assert f(fake, j, 0, 0, 1, vers, 4, 0, 1, tgt, None, 2, out) == E                 # no buffer for cap > 0
    assert f(fake, j, 0, 0, 1, vers, 4, 0, 1, tgt, buf, _lib.BM_MAX_HEADER_HITS + 1, out) == E
    assert f(fake, ctypes.byref(size9), 0, 0, 1, vers, 4, 0, 1, tgt, buf, 2, out) == E
    assert f(fake, j, 0, 0, 4096, vers, 4, 0, 1, tgt, buf, 2, out) == E               # 4097 values
    assert f(fake, j, 0, 100, 4196, vers, 4, 0, 1, tgt, buf, 2, out) == E
    assert f(fake, j, 0, 0xffff, 0x10000, vers, 4, 0, 1, tgt, buf, 2, out) == E       # past the 2-byte field
    assert f(fake, ctypes.byref(size8), 0, 0, (1 << 64) - 1, vers, 4, 0, 1, tgt, buf, 2, out) == E  # 2^64 values
    assert (bytes(r), bytes(buf)) == before


def test_python_search_job_shares_checks():
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._lib, ctx._h = None, None  # any library call would fail on this
    job = genesis_job()
    for args in (("job", [1], 0, 0), (job, [], 0, 0), (job, list(range(65)), 0, 0), (job, [-1], 0, 0),
                 (job, [1 << 32], 0, 0), (job, [True], 0, 0), (job, [1], -1, 0), (job, [1], 0, 1 << 16),
                 (job, [1], 0, 4096), (job, [1], 0.0, 1), (job, [1], 0, 0, -1), (job, [1], 0, 0, 0, 1 << 32),
                 (job, [1], 0, 0, 0, 1, -1), (job, [1], 0, 0, 0, 1, bytes(31)), (job, [1], 0, 0, 0, 1, 0, -1),
                 (job, [1], 0, 0, 0, 1, 0, _lib.BM_MAX_HEADER_HITS + 1), (job, [1], 0, 0, 0, 1, 0, True),
                 (job, [1], 0, 0, 0, 1, 0, 4, 1 << 32)):
        with pytest.raises(ValueError):
            ctx.search_job_shares(*args)


def test_submit_params():
    share = {"extranonce2": 29, "extranonce2_size": 2, "ntime": 0x495fab29, "nonce": 2083236893, "version": 1}
    assert submit_params("satoshi.1", "genesis", share, 0x1fffe000) == \
        ["satoshi.1", "genesis", "001d", "495fab29", "7c2bac1d", "00000000"]
    share = {"extranonce2": 0x0102030405060708, "extranonce2_size": 8, "ntime": 1, "nonce": 0xffffffff,
             "version": 0x3fffe001}
    assert submit_params("w", "ab12", share, 0x1fffe000) == ["w", "ab12", "0102030405060708", "00000001", "ffffffff",
                                                             "1fffe000"]
    assert submit_params("w", "j", dict(share, extranonce2=0, extranonce2_size=1, version=0x20006000), 0x2000)[2:] == \
        ["00", "00000001", "ffffffff", "00002000"]
    assert submit_params("w", "j", share)[5] == "1fffe000"  # BIP 320's mask by default
    with pytest.raises(ValueError):
        submit_params("w", "j", share, 1 << 32)
