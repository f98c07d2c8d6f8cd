"""The share set's C ABI, ctypes mirrors and CPU set (no GPU): the symbols, the
struct layout against a compiled C consumer, the CPU set (the specification)
against hashlib plus a Python set over the scenarios the GPU tests run
(tests/share_set_ref.py), BM_EFULL and its rollback, every refusal with canaries,
and the pool_dedup command line with --cpu.  The calls are additive, so the ABI
version stays 7."""
import ctypes
import io
import json
import os
import subprocess
import sys
import tempfile

import pytest

from conftest import GOLDEN, ROOT, load_golden
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import BtcMinerError, Job, PoolSession, ShareSet, _lib, pool_dedup
import pool_verify_ref as ref
import share_set_ref as sref

JOB_PATH = os.path.join(GOLDEN, "stratum_genesis_job.json")
SESSIONS_PATH = os.path.join(GOLDEN, "stratum_genesis_sessions.json")
JOB = load_golden("stratum_genesis_job.json")
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
GENESIS_PARAMS = '["satoshi.1","genesis","001d","495fab29","7c2bac1d","00000000"]'
BLOCK_LINE = "Block %s %064x" % (GENESIS_PARAMS, GENESIS_HASH)
DIFF1 = 0xffff << 208
RESULT_FIELDS = ["n", "shares", "blocks", "invalid", "ntime", "duplicates", "recorded", "count"]
FUNCTIONS = ("bm_share_set_create", "bm_share_set_create_cpu", "bm_share_set_destroy", "bm_share_set_clear",
             "bm_share_set_count", "bm_share_set_verify")


def genesis_job():
    return Job.from_notify(JOB["notify"], JOB["extranonce1"], JOB["extranonce2_size"])


# ---- the ABI ---------------------------------------------------------------------------

def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
    names = {"ShareSet", "ShareSetResult", "BM_SUBMIT_DUPLICATE", "BM_EFULL", "BM_MAX_SHARE_SET"}
    assert names <= set(pkg.__all__)
    assert all(getattr(pkg, n) is getattr(_lib, n) for n in names)
    assert (pkg.BM_SUBMIT_DUPLICATE, pkg.BM_EFULL, pkg.BM_MAX_SHARE_SET) == (16, -9, 1 << 24)
    assert lib.bm_strerror(-9).decode() not in ("", "unknown status")
    for method in ("verify", "clear", "close", "cpu"):
        assert hasattr(ShareSet, method)


def test_struct_layout_matches_the_header():
    """Size and every field offset of bm_share_set_result_t, and the constants, from
    a C program compiled against include/btcminer.h; it also calls nothing, so the
    prototypes only have to parse."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {",
             "bm_share_set_t* set = NULL; (void)set;",
             'printf("size %zu\\n", sizeof(bm_share_set_result_t));']
    lines += [f'printf("{f} %zu\\n", offsetof(bm_share_set_result_t, {f}));' for f in RESULT_FIELDS]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);',
              'printf("consts %u %d %u\\n", BM_SUBMIT_DUPLICATE, BM_EFULL, BM_MAX_SHARE_SET);',
              'printf("flags %u %u %u %u\\n", BM_SUBMIT_SHARE, BM_SUBMIT_BLOCK, BM_SUBMIT_INVALID, BM_SUBMIT_NTIME);',
              "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out if ln.strip()}
    assert got["abi"] == [7] and got["consts"] == [16, -9, 1 << 24] and got["flags"] == [1, 2, 4, 8]
    assert got["size"] == [ctypes.sizeof(_lib.ShareSetResult)] == [64]
    assert [got[f][0] for f in RESULT_FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56]
    for f in RESULT_FIELDS:
        assert got[f] == [getattr(_lib.ShareSetResult, f).offset], f


# ---- the CPU set against hashlib and a Python set -----------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_cpu_set_batch_edges(n):
    sref.batch_edges(ShareSet.cpu, n)


def test_cpu_set_contention_case():
    sref.contention(ShareSet.cpu)


def test_cpu_set_forced_collisions_case():
    sref.forced_collisions(ShareSet.cpu)


def test_cpu_set_capacity_edges_and_rollback():
    sref.capacity_edges(ShareSet.cpu)


def test_cpu_set_across_calls():
    sref.across_calls(ShareSet.cpu)


def test_cpu_set_key_is_the_hash():
    sref.key_is_the_hash(ShareSet.cpu)


def test_cpu_set_lifecycle():
    sref.lifecycle(ShareSet.cpu)


def test_home_slot_rule_of_the_reference():
    """The documented home slot: the hash's least significant 32 bits mod the slot
    count, a power of two that is at least twice the capacity and at least 16."""
    assert sref.home_slot(0x1234_0000_001f, 8) == 15 and sref.home_slot(0x1234_0000_001f, 9) == 31
    assert sref.home_slot((7 << 32) | 5, 1) == 5 and sref.home_slot(GENESIS_HASH, 1 << 24) == GENESIS_HASH & 0x1ffffff


# ---- refusals ------------------------------------------------------------------------------

def test_creation_refusals():
    lib = _lib.load()
    h = ctypes.c_void_p(0xA5A5)
    E = _lib.BM_EINVAL
    for cap in (0, (1 << 24) + 1, (1 << 64) - 1):
        assert lib.bm_share_set_create_cpu(cap, ctypes.byref(h)) == E
        assert lib.bm_share_set_create(ctypes.c_void_p(1), cap, ctypes.byref(h)) == E  # before the context is touched
    assert lib.bm_share_set_create_cpu(8, None) == E
    assert lib.bm_share_set_create(None, 8, ctypes.byref(h)) == E
    assert lib.bm_share_set_create(ctypes.c_void_p(1), 8, None) == E
    assert h.value == 0xA5A5
    lib.bm_share_set_destroy(None)  # fine
    assert lib.bm_share_set_clear(None) == E and lib.bm_share_set_count(None, None, None) == E
    for bad in (0, -1, 1.5, True, (1 << 24) + 1, "8"):
        with pytest.raises(ValueError):
            ShareSet.cpu(bad)
    with ShareSet.cpu(1 << 24) as s:  # the largest set: a host set allocates as it fills
        assert (s.count, s.capacity) == (0, 1 << 24)
    with pytest.raises(ValueError):
        s.count  # closed


def test_verify_refusals_leave_canaries_and_the_set():
    """Everything bm_pool_verify_* refuses, and a NULL set: BM_EINVAL, `verdicts` and
    `out` untouched, the set as it was."""
    lib = _lib.load()
    f = lib.bm_share_set_verify
    job = genesis_job()
    sessions = ref.session_array([PoolSession(b"\xff\xff", DIFF1)] * 2)
    good = [(29, job.ntime, 2083236893, 1, 0)]
    subs = ref.sub_array(good * 3)
    with ShareSet.cpu(4) as s:
        verdicts, r = s.verify(job, sessions, good)
        assert ref.as_tuples(verdicts) == [(GENESIS_HASH, 3)] and sref.result_tuple(r) == (1, 1, 1, 0, 0, 0, 1, 1)
        verdicts = (_lib.JobVerdict * 3)()
        ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
        r = _lib.ShareSetResult()
        ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
        before = bytes(verdicts), bytes(r)
        j, out, h = ctypes.byref(job.struct), ctypes.byref(r), s.handle

        def variant(**kw):
            v = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
            for k, val in kw.items():
                setattr(v, k, val)
            return ctypes.byref(v)

        E, W = _lib.BM_EINVAL, (0, ref.U32)
        assert f(None, j, sessions, 2, subs, 3, *W, verdicts, out) == E
        assert f(h, None, sessions, 2, subs, 3, *W, verdicts, out) == E
        assert f(h, j, None, 2, subs, 3, *W, verdicts, out) == E
        assert f(h, j, sessions, 2, None, 3, *W, verdicts, out) == E
        assert f(h, j, sessions, 2, subs, 3, *W, None, out) == E
        assert f(h, j, sessions, 2, subs, 3, *W, verdicts, None) == E
        assert f(h, j, sessions, 2, subs, _lib.BM_MAX_JOB_SUBMITS + 1, *W, verdicts, out) == E
        assert f(h, j, sessions, _lib.BM_MAX_POOL_SESSIONS + 1, subs, 3, *W, verdicts, out) == E
        assert f(None, j, sessions, 2, None, 0, *W, None, out) == E  # n == 0 excuses the arrays only
        assert f(h, None, sessions, 2, None, 0, *W, None, out) == E
        assert f(h, j, sessions, 2, None, 0, *W, None, None) == E
        for kw in (dict(extranonce1_len=0), dict(extranonce1_len=9), dict(extranonce2_size=0), dict(extranonce2_size=9),
                   dict(nbranch=33), dict(coinb1=None), dict(coinb2_len=1 << 16), dict(coinb1_len=(1 << 64) - 1)):
            assert f(h, variant(**kw), sessions, 2, subs, 3, *W, verdicts, out) == E, kw
        assert (bytes(verdicts), bytes(r)) == before and s.count == 1
        # n == 0: legal, nothing changes; no array is touched or needed
        assert f(h, j, None, 0, None, 0, *W, None, out) == _lib.BM_OK and sref.result_tuple(r) == (0,) * 7 + (1,)
        assert f(h, j, sessions, 2, subs, 0, *W, verdicts, out) == _lib.BM_OK and bytes(verdicts) == before[0]
        # the set is as it was: the genesis hash is still the one it holds
        verdicts, r = s.verify(job, sessions, good * 2)
        assert [v.status for v in verdicts] == [3 | 16, 3 | 16] and verdicts[0].is_duplicate and r.count == 1


def test_python_layer():
    job = genesis_job()
    ses = [PoolSession(b"\xff\xff", DIFF1), PoolSession(b"\x00\x01", ref.U256)]
    with ShareSet.cpu(2) as s:
        verdicts, r = s.verify(job, ses, [{"extranonce2": 29, "ntime": job.ntime, "nonce": 2083236893, "version": 1,
                                          "session": 0}])
        assert isinstance(r, _lib.ShareSetResult) and not verdicts[0].is_duplicate and verdicts[0].is_block
        with pytest.raises(BtcMinerError) as e:  # two new hashes into one free entry
            s.verify(job, ses, [(1, 2, 3, 4, 1), (2, 2, 3, 4, 1)])
        assert e.value.status == _lib.BM_EFULL == -9 and s.count == 1
        for bad in ([(1, 2, 3, 4)], [(1 << 64, 2, 3, 4, 0)]):
            with pytest.raises(ValueError):
                s.verify(job, ses, bad)
        with pytest.raises(ValueError):
            s.verify(job, ses, [(1, 2, 3, 4, 0)], 0, 1 << 32)
        s.clear()
        assert s.count == 0
        s.close()
        s.close()  # twice is fine
        with pytest.raises(ValueError):
            s.verify(job, ses, [])


# ---- the command line ------------------------------------------------------------------------

def run(text, *flags, sessions=SESSIONS_PATH):
    out = io.StringIO()
    rc = pool_dedup.main([JOB_PATH, sessions, "-", "--cpu", *flags], out=out, stdin=io.StringIO(text))
    return rc, out.getvalue().splitlines()


def test_cli_genesis_twice():
    """The README's example: the genesis submission fed twice."""
    want = [BLOCK_LINE, "Reject duplicate " + GENESIS_PARAMS, "Verified 2 Accepted 1 Blocks 1 Rejected 1 Duplicates 1"]
    text = GENESIS_PARAMS + "\n" + BLOCK_LINE + "\n"
    assert run(text) == (0, want)
    assert run(text, "--batch", "1") == (0, want)  # across two calls on the set
    assert run(text, "--batch", "2", "--capacity", "1") == (0, want)
    assert run(GENESIS_PARAMS + "\n") == (0, [BLOCK_LINE, "Verified 1 Accepted 1 Blocks 1 Rejected 0 Duplicates 0"])
    assert run("") == (0, ["Verified 0 Accepted 0 Blocks 0 Rejected 0 Duplicates 0"])


def test_cli_lines_batches_and_a_full_set(tmp_path, capsys):
    good = json.loads(GENESIS_PARAMS)

    def with_(i, v, params=good):
        return json.dumps(params[:i] + [v] + params[i + 1:], separators=(",", ":"))

    # two workers that share an extranonce1: the same work is a duplicate, whoever sends it; an easy worker
    # accepts other nonces, each once
    path = tmp_path / "sessions.json"
    path.write_text(json.dumps({"workers": {"satoshi.1": {"extranonce1": "ffff", "difficulty": 1},
                                            "twin.1": {"extranonce1": "ffff", "difficulty": 1},
                                            "easy.1": {"extranonce1": "ffff", "difficulty": 2.0 ** -40},
                                            "hal.1": {"extranonce1": "0001", "difficulty": 1}}}))
    easy = ["easy.1"] + good[1:]
    e1, e2 = with_(4, "7c2bac1e", easy), with_(4, "7c2bac1f", easy)
    job = genesis_job()
    hashes = [ref.verdict(job, [PoolSession(b"\xff\xff", ref.U256)], (29, 0x495fab29, nonce, 1, 0))[0]
              for nonce in (0x7c2bac1e, 0x7c2bac1f)]
    lines = [GENESIS_PARAMS, e1, with_(0, "twin.1"), "hello", with_(0, "hal.1"), e2, e1, with_(0, "hal.1"),
             with_(4, "7c2bac1e"), with_(0, "nobody"), "", e2]
    want = [BLOCK_LINE, "Accept %s %064x" % (e1, hashes[0]), "Reject duplicate " + with_(0, "twin.1"),
            "Reject malformed hello", "Reject above-target " + with_(0, "hal.1"), "Accept %s %064x" % (e2, hashes[1]),
            "Reject duplicate " + e1, "Reject above-target " + with_(0, "hal.1"),
            "Reject above-target " + with_(4, "7c2bac1e"),  # above satoshi.1's target: never in the set, never a duplicate
            "Reject worker " + with_(0, "nobody"), "Reject duplicate " + e2,
            "Verified 11 Accepted 3 Blocks 1 Rejected 8 Duplicates 3"]
    text = "\n".join(lines) + "\n"
    for flags in ((), ("--batch", "1"), ("--batch", "2"), ("--batch", "5"), ("--batch", "0x100"), ("--capacity", "3")):
        assert run(text, *flags, sessions=str(path)) == (0, want), flags
    # outside the window a line is an ntime reject, duplicate or not
    got = run(text, "--ntime-window", "0", "5", sessions=str(path))[1]
    assert got[0] == "Reject ntime " + GENESIS_PARAMS and got[2] == "Reject ntime " + with_(0, "twin.1")
    assert got[-1] == "Verified 11 Accepted 0 Blocks 0 Rejected 11 Duplicates 0"
    # a set too small for the three distinct accepted hashes: status 3, a message, nothing printed
    capsys.readouterr()
    for flags in (("--capacity", "2"), ("--capacity", "2", "--batch", "1")):
        assert run(text, *flags, sessions=str(path)) == (3, [])
        assert "full" in capsys.readouterr().err
    # argument errors: status 2
    for flags in (("--capacity", "0"), ("--batch", "0"), ("--capacity", "x"), ("--batch", str((1 << 20) + 1)),
                  ("--capacity", str((1 << 24) + 1)), ("--ntime-window", "1")):
        assert run(text, *flags, sessions=str(path))[0] == 2, flags
    assert pool_dedup.main([]) == 2 and pool_dedup.main([JOB_PATH]) == 2
    assert pool_dedup.main([JOB_PATH + ".missing", SESSIONS_PATH, "-", "--cpu"], stdin=io.StringIO("")) == 2
    assert pool_dedup.main([JOB_PATH, SESSIONS_PATH, str(tmp_path / "missing.txt"), "--cpu"]) == 2


def test_cli_as_a_module():
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "distributed_bitcoin_minter_amd.pool_dedup", JOB_PATH, SESSIONS_PATH, "--cpu"]
    r = subprocess.run(cmd, input=GENESIS_PARAMS + "\n" + GENESIS_PARAMS + "\n", capture_output=True, text=True,
                       timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0 and r.stdout.splitlines() == [
        BLOCK_LINE, "Reject duplicate " + GENESIS_PARAMS, "Verified 2 Accepted 1 Blocks 1 Rejected 1 Duplicates 1"], r.stderr


# ---- the C++ wrapper -------------------------------------------------------------------------

CPP = r"""
#include <cstdio>
#include <utility>
#include "btcminer.hpp"
int main() {
    btcminer::Job job;
    job.coinb1 = {1, 2, 3};
    job.extranonce1 = {9, 9};
    job.extranonce2_size = 2;
    job.coinb2 = {4, 5};
    job.nbits = 0x1d00ffff;
    std::vector<bm_pool_session_t> ses(1);
    for (auto& b : ses[0].target) b = 0xFF;
    for (auto& b : ses[0].extranonce1) b = 7;
    bm_pool_submit_t subs[3] = {{1, 2, 3, 4, 0}, {2, 2, 3, 4, 0}, {1, 2, 3, 4, 0}};
    std::vector<bm_job_verdict_t> v;
    btcminer::ShareSet a = btcminer::ShareSet::cpu(2);
    btcminer::ShareSet set = std::move(a);
    bm_share_set_result_t r = set.verify(job, ses, subs, 3, v);
    std::printf("%d %d %d %d\n", (int)r.recorded, (int)r.duplicates, (int)set.count(), (int)set.capacity());
    std::printf("%u %u %u\n", v[0].status, v[1].status, v[2].status);
    bm_pool_submit_t more[1] = {{3, 2, 3, 4, 0}};
    try {
        set.verify(job, ses, more, 1, v);
        std::printf("no error\n");
    } catch (const btcminer::Error& e) {
        std::printf("status %d kept %zu\n", e.status(), v.size());
    }
    set.clear();
    std::printf("%d\n", (int)set.count());
    a = btcminer::ShareSet::cpu(1);
    set = std::move(a);
    std::printf("%d %d\n", (int)set.capacity(), a.get() == nullptr);
    return 0;
}
"""


def test_cpp_wrapper():
    """include/btcminer.hpp's ShareSet over a CPU set: move-only ownership, verify,
    BM_EFULL as an Error that leaves `verdicts`, clear, count, capacity."""
    pkg_dir = os.path.dirname(_lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "wrapper.cpp"), os.path.join(d, "wrapper")
        with open(src, "w") as f:
            f.write(CPP)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                               "-L", pkg_dir, "-lbtcminer", "-Wl,-rpath," + pkg_dir, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    assert out == ["2 1 2 2", "1 1 17", "status -9 kept 3", "0", "1 1"]
