"""The share verifier's C ABI, ctypes mirrors and CPU entry (no GPU):
bm_job_verify_cpu against hashlib (tests/verify_ref.py) over the layout grid,
the genesis job, INVALID entries, the refusals with canaries, the struct layouts
against a compiled C consumer, parse_submit, and the built kernel's resources.
The calls are additive, so the ABI version stays 7."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

from conftest import ROOT, load_golden
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import (Job, _lib, difficulty_to_target, parse_submit, submit_params,
                                            verify_submits_cpu)
import verify_ref as ref

JOB = load_golden("stratum_genesis_job.json")
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
BUILD = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc", "build")
SUBMIT_FIELDS = ["extranonce2", "ntime", "nonce", "version", "reserved"]
VERDICT_FIELDS = ["hash", "status", "reserved"]
RESULT_FIELDS = ["n", "shares", "blocks", "invalid"]


def genesis_job():
    return Job.from_notify(JOB["notify"], JOB["extranonce1"], JOB["extranonce2_size"])


def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_job_verify_cpu", "bm_job_verify_gpu"):
        assert hasattr(lib, name), name
    names = {"JobSubmit", "JobVerdict", "JobVerifyResult", "parse_submit", "verify_submits_cpu"}
    assert names <= set(pkg.__all__)
    assert all(getattr(pkg, n) is getattr(_lib, n) for n in names)
    assert hasattr(_lib.Context, "verify_submits")
    assert (_lib.BM_SUBMIT_SHARE, _lib.BM_SUBMIT_BLOCK, _lib.BM_SUBMIT_INVALID) == (1, 2, 4)


def test_struct_layouts_match_the_header():
    """Size and every field offset of the three structs, and the constants, from
    a C program compiled against include/btcminer.h."""
    structs = {"bm_job_submit_t": (_lib.JobSubmit, SUBMIT_FIELDS), "bm_job_verdict_t": (_lib.JobVerdict, VERDICT_FIELDS),
               "bm_job_verify_result_t": (_lib.JobVerifyResult, RESULT_FIELDS)}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name}.size %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("max %u\\n", BM_MAX_JOB_SUBMITS);',
              'printf("flags %u %u %u\\n", BM_SUBMIT_SHARE, BM_SUBMIT_BLOCK, BM_SUBMIT_INVALID);', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out if ln.strip()}
    assert got["abi"] == [7] and got["max"] == [_lib.BM_MAX_JOB_SUBMITS] == [1 << 20] and got["flags"] == [1, 2, 4]
    assert got["bm_job_submit_t.size"] == [ctypes.sizeof(_lib.JobSubmit)] == [24]
    assert got["bm_job_verdict_t.size"] == [ctypes.sizeof(_lib.JobVerdict)] == [40]
    assert got["bm_job_verify_result_t.size"] == [ctypes.sizeof(_lib.JobVerifyResult)] == [32]
    assert [got[f"bm_job_submit_t.{f}"][0] for f in SUBMIT_FIELDS] == [0, 8, 12, 16, 20]
    assert [got[f"bm_job_verdict_t.{f}"][0] for f in VERDICT_FIELDS] == [0, 32, 36]
    assert [got[f"bm_job_verify_result_t.{f}"][0] for f in RESULT_FIELDS] == [0, 8, 16, 24]
    for name, (mirror, fields) in structs.items():
        for f in fields:
            assert got[f"{name}.{f}"] == [getattr(mirror, f).offset], (name, f)


def test_cpu_entry_against_hashlib_over_the_layout_grid():
    grid = ref.layout_grid()
    assert len(grid) == 400 and sum(len(subs) for _, _, subs, _ in grid) == 26000
    seen = set()
    for label, job, subs, want in grid:
        verdicts, r = verify_submits_cpu(job, ref.sub_array(subs), ref.GRID_TARGET)
        assert ref.as_tuples(verdicts) == want, label
        assert ref.result_tuple(r) == ref.counts(want), label
        seen |= {status for _, status in want}
    assert seen == {0, 1, 3}  # rejects, shares and blocks all occur (the block target lies below the share target)


@pytest.mark.parametrize("depth", [0, 1, 2, 12, 32])
def test_cpu_entry_branch_depths(depth):
    rng = random.Random(depth)
    job = ref.synthetic_job(rng, 45, 4, 250, depth)
    subs = ref.random_subs(rng, 4, 33)
    verdicts, r = verify_submits_cpu(job, subs, ref.GRID_TARGET)  # plain tuples: the Python layer builds the array
    want = [ref.verdict(job, ref.GRID_TARGET, s) for s in subs]
    assert ref.as_tuples(verdicts) == want and ref.result_tuple(r) == ref.counts(want)


def test_genesis_submission():
    job = genesis_job()
    target = difficulty_to_target(JOB["difficulty"])
    sub = (29, job.ntime, 2083236893, 1)
    assert ref.verdict(job, target, sub) == (GENESIS_HASH, 3)
    verdicts, r = verify_submits_cpu(job, [sub, (28,) + sub[1:], {"extranonce2": 29, "ntime": job.ntime,
                                                                "nonce": 2083236893, "version": 0x2001}], target)
    assert ref.as_tuples(verdicts)[0] == (GENESIS_HASH, 3)
    assert verdicts[0].is_share and verdicts[0].is_block and not verdicts[0].is_invalid
    assert f"{verdicts[0].value:064x}".startswith("000000000019d668") and f"{verdicts[0].value:064x}".endswith("0a8ce26f")
    assert ref.as_tuples(verdicts)[1:] == [ref.verdict(job, target, (28,) + sub[1:]),
                                           ref.verdict(job, target, (29, job.ntime, 2083236893, 0x2001))]
    assert verdicts[1].status == 0 and ref.result_tuple(r) == (3, 1, 1, 0)


def test_invalid_entries_and_flag_independence():
    rng = random.Random(7)
    job = ref.synthetic_job(rng, 70, 2, 150, 1)
    subs = [(0xffff, 1, 2, 3), (0x10000, 1, 2, 3), (ref.U64, 1, 2, 3), (5, 6, 7, 8)]
    want = [ref.verdict(job, ref.U256, s) for s in subs]
    assert want[1] == want[2] == ref.INVALID_VERDICT and want[0][1] & 1
    verdicts, r = verify_submits_cpu(job, subs, ref.U256)
    assert ref.as_tuples(verdicts) == want and ref.result_tuple(r) == ref.counts(want) and r.invalid == 2
    assert bytes(verdicts[1].hash) == b"\xff" * 32 and verdicts[1].status == 4 and verdicts[1].is_invalid
    # size 8 accepts 2^64 - 1
    job8 = ref.synthetic_job(rng, 61, 8, 130, 0)
    verdicts, r = verify_submits_cpu(job8, [(ref.U64, 1, 2, 3)], ref.U256)
    assert ref.as_tuples(verdicts) == [ref.verdict(job8, ref.U256, (ref.U64, 1, 2, 3))] and r.invalid == 0
    # a share target below the hash and a block target above it: BLOCK without SHARE
    wide = ref.synthetic_job(rng, 10, 4, 100, 0, nbits=0x2100ffff)
    h, st = ref.verdict(wide, 0, (1, 2, 3, 4))
    assert st == 2 and h <= ref.block_target(0x2100ffff) == 0xffff << 240
    verdicts, r = verify_submits_cpu(wide, [(1, 2, 3, 4)], 0)
    assert ref.as_tuples(verdicts) == [(h, 2)] and ref.result_tuple(r) == (1, 0, 1, 0)
    # an nbits that does not decode (the sign bit; past 256 bits) leaves BLOCK clear
    for nbits in (0x1d80ffff, 0x2300ffff):
        assert ref.block_target(nbits) is None
        job = ref.synthetic_job(rng, 10, 4, 100, 0, nbits=nbits)
        verdicts, r = verify_submits_cpu(job, [(1, 2, 3, 4)], ref.U256)
        assert ref.as_tuples(verdicts) == [ref.verdict(job, ref.U256, (1, 2, 3, 4))] and verdicts[0].status == 1


def _canaries(n=3):
    verdicts = (_lib.JobVerdict * n)()
    ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
    r = _lib.JobVerifyResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    return verdicts, r


def _refusals(call):
    """Every refusal of the issue that needs no context, through call(job, target,
    submits, n, verdicts, out): BM_EINVAL, verdicts and out untouched."""
    job = genesis_job()
    subs = ref.sub_array([(1, 2, 3, 4)] * 3)
    verdicts, r = _canaries()
    before = bytes(verdicts), bytes(r)
    j, tgt, out = ctypes.byref(job.struct), bytes(32), ctypes.byref(r)

    def variant(**kw):
        s = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
        for k, v in kw.items():
            setattr(s, k, v)
        return ctypes.byref(s)

    E = _lib.BM_EINVAL
    assert call(None, tgt, subs, 3, verdicts, out) == E
    assert call(j, None, subs, 3, verdicts, out) == E
    assert call(j, tgt, None, 3, verdicts, out) == E
    assert call(j, tgt, subs, 3, None, out) == E
    assert call(j, tgt, subs, 3, verdicts, None) == E
    assert call(j, tgt, subs, _lib.BM_MAX_JOB_SUBMITS + 1, verdicts, out) == E  # refused before anything is read
    assert call(None, tgt, None, 0, None, out) == E                             # n == 0 excuses the arrays only
    assert call(j, tgt, None, 0, None, None) == E
    for kw in (dict(extranonce2_size=0), dict(extranonce2_size=9), dict(nbranch=33), dict(coinb1=None),
               dict(coinb2_len=1 << 16), dict(coinb1_len=(1 << 64) - 1)):
        assert call(variant(**kw), tgt, subs, 3, verdicts, out) == E, kw
    assert (bytes(verdicts), bytes(r)) == before
    return j, tgt, subs, verdicts, r, before


def test_cpu_entry_refusals_and_empty_batch():
    f = _lib.load().bm_job_verify_cpu
    j, tgt, subs, verdicts, r, before = _refusals(f)
    # n == 0: zeros, no array touched or needed
    assert f(j, tgt, None, 0, None, ctypes.byref(r)) == _lib.BM_OK and ref.result_tuple(r) == (0, 0, 0, 0)
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    assert f(j, tgt, subs, 0, verdicts, ctypes.byref(r)) == _lib.BM_OK and ref.result_tuple(r) == (0, 0, 0, 0)
    assert bytes(verdicts) == before[0]
    # a batch shorter than its arrays leaves the rest alone
    assert f(j, tgt, subs, 2, verdicts, ctypes.byref(r)) == _lib.BM_OK and r.n == 2
    assert bytes(verdicts[2]) == b"\xa5" * 40 and bytes(verdicts[1]) != b"\xa5" * 40


def test_gpu_entry_refuses_before_it_touches_the_context():
    """The same refusals through bm_job_verify_gpu over a stand-in context pointer, and a NULL context."""
    f = _lib.load().bm_job_verify_gpu
    fake = ctypes.c_void_p(1)
    j, tgt, subs, verdicts, r, before = _refusals(lambda *a: f(fake, *a))
    assert f(None, j, tgt, subs, 3, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
    assert (bytes(verdicts), bytes(r)) == before


def test_python_layer_checks():
    job = genesis_job()
    for bad in ([(1, 2, 3)], [(1, 2, 3, 4, 5)], [(-1, 2, 3, 4)], [(1 << 64, 2, 3, 4)], [(1, 1 << 32, 3, 4)],
                [(1, 2, -3, 4)], [(1, 2, 3, True)], [{"extranonce2": 1, "ntime": 2, "nonce": 3}]):
        with pytest.raises((ValueError, KeyError)):
            verify_submits_cpu(job, bad, 0)
    for target in (-1, 1 << 256, bytes(31), None):
        with pytest.raises(ValueError):
            verify_submits_cpu(job, [(1, 2, 3, 4)], target)
    with pytest.raises(ValueError):
        verify_submits_cpu("job", [(1, 2, 3, 4)], 0)
    verdicts, r = verify_submits_cpu(job, [], 0)
    assert len(verdicts) == 0 and ref.result_tuple(r) == (0, 0, 0, 0)
    # the shares of search_job_shares are submissions as they are
    share = {"hash": 0, "extranonce2": 29, "extranonce2_size": 2, "ntime": job.ntime, "nonce": 2083236893,
             "version_index": 0, "version": 1, "is_block": True}
    assert ref.as_tuples(verify_submits_cpu(job, [share], ref.U256)[0]) == [(GENESIS_HASH, 3)]


@pytest.mark.parametrize("mask", [0x1fffe000, 0x00ffe000, 0xffffffff])
def test_parse_submit_inverts_submit_params(mask):
    rng = random.Random(mask)
    for _ in range(1000):
        size = rng.randint(1, 8)
        job = Job(b"", b"", size, b"", version=rng.getrandbits(32), job_id="j%d" % rng.getrandbits(16))
        # a rolled version differs from the job's inside the mask only
        version = (job.version & ~mask) | (rng.getrandbits(32) & mask)
        share = {"extranonce2": rng.getrandbits(8 * size), "extranonce2_size": size, "ntime": rng.getrandbits(32),
                 "nonce": rng.getrandbits(32), "version": version}
        params = submit_params("w.1", job.job_id, share, mask)
        assert parse_submit(params, job, mask) == share
        assert parse_submit(tuple(params[:5]), job, mask) == dict(share, version=job.version)


def test_parse_submit_rejects_with_the_reason():
    job = genesis_job()
    good = ["satoshi.1", "genesis", "001d", "495fab29", "7c2bac1d", "00002000"]
    assert parse_submit(good, job) == {"extranonce2": 29, "extranonce2_size": 2, "ntime": 0x495fab29,
                                       "nonce": 2083236893, "version": 0x2001}
    assert parse_submit(good, job, 0x2000)["version"] == 0x2001

    def reason(params, mask=0x1fffe000):
        with pytest.raises(ValueError) as e:
            parse_submit(params, job, mask)
        return str(e.value).split(":")[0]

    assert reason(good[:1] + ["other"] + good[2:]) == "job-id"
    for en2 in ("1d", "00001d", "001", "001g", "0x1d", " 01d", 29, None):
        assert reason(good[:2] + [en2] + good[3:]) == "extranonce2", en2
    for i in (3, 4, 5):
        for bad in ("495fab2", "495fab290", "495fab2g", "+95fab29", 5, None):
            assert reason(good[:i] + [bad] + good[i + 1:]) == "malformed", (i, bad)
    assert reason(good[:5] + ["00000001"]) == "version-bits"
    assert reason(good[:5] + ["20000000"]) == "version-bits"
    assert reason(good, 0x4000) == "version-bits"
    for params in (good[:4], good + ["x"], [], "genesis", None):
        assert reason(params) == "malformed"
    with pytest.raises(ValueError):
        parse_submit(good, job, 1 << 32)


def test_kernel_resources():
    """The built job_verify_kernel: no scratch, no spills (the unit's resource remarks)."""
    path = os.path.join(BUILD, "bm_job_verify_inst.res")
    if not os.path.exists(path):
        pytest.skip("device assembly not built (make -C distributed_bitcoin_minter_amd/csrc)")
    with open(path) as f:
        res = f.read()
    assert "job_verify_kernel" in res
    for line in ("ScratchSize [bytes/lane]: 0", "SGPRs Spill: 0", "VGPRs Spill: 0"):
        assert res.count(line) == 1, (line, res[-1500:])
