"""The pool verifier's C ABI, ctypes mirrors and CPU entry (no GPU):
bm_pool_verify_cpu against hashlib (tests/pool_verify_ref.py) over the layout
grid, per-session targets, the ntime window, INVALID entries, the refusals with
canaries, the struct layouts against a compiled C consumer, parse_pool_submit and
the pool_verify command line with --cpu.  The calls are additive, so the ABI
version stays 7."""
import ctypes
import io
import json
import os
import random
import subprocess
import sys
import tempfile

import pytest

from conftest import GOLDEN, ROOT, load_golden
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import (Job, PoolSession, _lib, parse_pool_submit, pool_verify,
                                            verify_pool_submits_cpu)
import pool_verify_ref as ref

JOB_PATH = os.path.join(GOLDEN, "stratum_genesis_job.json")
SESSIONS_PATH = os.path.join(GOLDEN, "stratum_genesis_sessions.json")
JOB = load_golden("stratum_genesis_job.json")
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
GENESIS_PARAMS = '["satoshi.1","genesis","001d","495fab29","7c2bac1d","00000000"]'
# what `stratum_job tests/golden/stratum_genesis_job.json --versions 1 --extranonce2 29 29 2083236608 2083237119` prints
MINED = ("Block %s %064x\n" % (GENESIS_PARAMS, GENESIS_HASH)
         + "Shares 1 Best %064x 001d 2083236893 00000001\n" % GENESIS_HASH)
DIFF1 = 0xffff << 208
SESSION_FIELDS = ["extranonce1", "target"]
SUBMIT_FIELDS = ["extranonce2", "ntime", "nonce", "version", "session"]
RESULT_FIELDS = ["n", "shares", "blocks", "invalid", "ntime"]


def genesis_job():
    return Job.from_notify(JOB["notify"], JOB["extranonce1"], JOB["extranonce2_size"])


def check(job, sessions, subs, lo=0, hi=ref.U32, want=None):
    """One call of the CPU entry; every verdict and the counts against hashlib."""
    want = [ref.verdict(job, sessions, s, lo, hi) for s in subs] if want is None else want
    verdicts, r = verify_pool_submits_cpu(job, ref.session_array(sessions), ref.sub_array(subs), lo, hi)
    assert ref.as_tuples(verdicts) == want
    assert ref.result_tuple(r) == ref.counts(want)
    return want


# ---- the ABI ---------------------------------------------------------------------------

def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_pool_verify_cpu", "bm_pool_verify_gpu"):
        assert hasattr(lib, name), name
    names = {"PoolSession", "PoolSubmit", "PoolVerifyResult", "parse_pool_submit", "verify_pool_submits_cpu"}
    assert names <= set(pkg.__all__)
    assert all(getattr(pkg, n) is getattr(_lib, n) for n in names)
    assert hasattr(_lib.Context, "verify_pool_submits")
    assert (_lib.BM_SUBMIT_NTIME, _lib.BM_MAX_POOL_SESSIONS) == (8, 1 << 20)


def test_struct_layouts_match_the_header():
    """Size and every field offset of the three structs, and the constants, from
    a C program compiled against include/btcminer.h."""
    structs = {"bm_pool_session_t": (_lib.PoolSessionStruct, SESSION_FIELDS),
               "bm_pool_submit_t": (_lib.PoolSubmit, SUBMIT_FIELDS),
               "bm_pool_verify_result_t": (_lib.PoolVerifyResult, RESULT_FIELDS)}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name}.size %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("max %u %u\\n", BM_MAX_JOB_SUBMITS, BM_MAX_POOL_SESSIONS);',
              'printf("flags %u %u %u %u\\n", BM_SUBMIT_SHARE, BM_SUBMIT_BLOCK, BM_SUBMIT_INVALID, BM_SUBMIT_NTIME);',
              'printf("reserved %zu\\n", offsetof(bm_job_submit_t, reserved));', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out if ln.strip()}
    assert got["abi"] == [7] and got["max"] == [1 << 20, 1 << 20] and got["flags"] == [1, 2, 4, 8]
    assert got["bm_pool_session_t.size"] == [ctypes.sizeof(_lib.PoolSessionStruct)] == [40]
    assert got["bm_pool_submit_t.size"] == [ctypes.sizeof(_lib.PoolSubmit)] == [24]
    assert got["bm_pool_verify_result_t.size"] == [ctypes.sizeof(_lib.PoolVerifyResult)] == [40]
    assert [got[f"bm_pool_session_t.{f}"][0] for f in SESSION_FIELDS] == [0, 8]
    assert [got[f"bm_pool_submit_t.{f}"][0] for f in SUBMIT_FIELDS] == [0, 8, 12, 16, 20]
    assert got["reserved"] == [20]  # session sits where bm_job_submit_t has reserved
    assert [got[f"bm_pool_verify_result_t.{f}"][0] for f in RESULT_FIELDS] == [0, 8, 16, 24, 32]
    for name, (mirror, fields) in structs.items():
        for f in fields:
            assert got[f"{name}.{f}"] == [getattr(mirror, f).offset], (name, f)


def _canaries(n=3):
    verdicts = (_lib.JobVerdict * n)()
    ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
    r = _lib.PoolVerifyResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    return verdicts, r


def _refusals(call):
    """Every refusal that needs no context, through call(job, sessions, nsessions,
    submits, n, lo, hi, verdicts, out): BM_EINVAL, verdicts and out untouched."""
    job = genesis_job()
    sessions = ref.session_array([PoolSession(b"\xff\xff", DIFF1)] * 2)
    subs = ref.sub_array([(1, 2, 3, 4, 0)] * 3)
    verdicts, r = _canaries()
    before = bytes(verdicts), bytes(r)
    j, out = ctypes.byref(job.struct), ctypes.byref(r)

    def variant(**kw):
        s = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
        for k, v in kw.items():
            setattr(s, k, v)
        return ctypes.byref(s)

    E = _lib.BM_EINVAL
    W = (0, ref.U32)
    assert call(None, sessions, 2, subs, 3, *W, verdicts, out) == E
    assert call(j, None, 2, subs, 3, *W, verdicts, out) == E
    assert call(j, sessions, 2, None, 3, *W, verdicts, out) == E
    assert call(j, sessions, 2, subs, 3, *W, None, out) == E
    assert call(j, sessions, 2, subs, 3, *W, verdicts, None) == E
    assert call(j, sessions, 2, subs, _lib.BM_MAX_JOB_SUBMITS + 1, *W, verdicts, out) == E  # before anything is read
    assert call(j, sessions, _lib.BM_MAX_POOL_SESSIONS + 1, subs, 3, *W, verdicts, out) == E
    assert call(None, sessions, 2, None, 0, *W, None, out) == E                             # n == 0 excuses the arrays only
    assert call(j, sessions, 2, None, 0, *W, None, None) == E
    for kw in (dict(extranonce1_len=0), dict(extranonce1_len=9), dict(extranonce1_len=(1 << 64) - 1),
               dict(extranonce2_size=0), dict(extranonce2_size=9), dict(nbranch=33), dict(coinb1=None),
               dict(coinb2_len=1 << 16), dict(coinb1_len=(1 << 64) - 1)):
        assert call(variant(**kw), sessions, 2, subs, 3, *W, verdicts, out) == E, kw
    assert (bytes(verdicts), bytes(r)) == before
    return job, j, sessions, subs, verdicts, r, before


def test_cpu_entry_refusals_and_empty_batch():
    f = _lib.load().bm_pool_verify_cpu
    job, j, sessions, subs, verdicts, r, before = _refusals(f)
    W = (0, ref.U32)
    # n == 0: zeros, no array touched or needed
    assert f(j, sessions, 2, None, 0, *W, None, ctypes.byref(r)) == _lib.BM_OK and ref.result_tuple(r) == (0,) * 5
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    assert f(j, None, 0, subs, 0, *W, verdicts, ctypes.byref(r)) == _lib.BM_OK and ref.result_tuple(r) == (0,) * 5
    assert bytes(verdicts) == before[0]
    # a batch shorter than its arrays leaves the rest alone
    assert f(j, sessions, 2, subs, 2, *W, verdicts, ctypes.byref(r)) == _lib.BM_OK and r.n == 2
    assert bytes(verdicts[2]) == b"\xa5" * 40 and bytes(verdicts[1]) != b"\xa5" * 40
    # job->extranonce1 is ignored and may be NULL: only its length counts
    null_en1 = _lib.JobStruct.from_buffer_copy(bytes(job.struct))
    null_en1.extranonce1 = None
    other = (_lib.JobVerdict * 2)()
    assert f(ctypes.byref(null_en1), sessions, 2, subs, 2, *W, other, ctypes.byref(r)) == _lib.BM_OK
    assert bytes(other) == bytes(verdicts)[:80]


def test_gpu_entry_refuses_before_it_touches_the_context():
    """The same refusals through bm_pool_verify_gpu over a stand-in context pointer, and a NULL context."""
    f = _lib.load().bm_pool_verify_gpu
    fake = ctypes.c_void_p(1)
    _job, j, sessions, subs, verdicts, r, before = _refusals(lambda *a: f(fake, *a))
    assert f(None, j, sessions, 2, subs, 3, 0, ref.U32, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
    assert (bytes(verdicts), bytes(r)) == before


def test_python_layer_checks():
    job = genesis_job()
    ses = [PoolSession(b"\xff\xff", DIFF1)]
    for bad in ([(1, 2, 3, 4)], [(1, 2, 3, 4, 5, 6)], [(-1, 2, 3, 4, 0)], [(1 << 64, 2, 3, 4, 0)], [(1, 1 << 32, 3, 4, 0)],
                [(1, 2, 3, 4, -1)], [(1, 2, 3, 4, 1 << 32)], [{"extranonce2": 1, "ntime": 2, "nonce": 3, "version": 4}]):
        with pytest.raises((ValueError, KeyError)):
            verify_pool_submits_cpu(job, ses, bad)
    for bad in ([PoolSession(b"\xff", 0)], [(b"\xff\xff\xff", 0)], [(b"\xff\xff", -1)], [(b"\xff\xff", 1 << 256)]):
        with pytest.raises(ValueError):
            verify_pool_submits_cpu(job, bad, [(1, 2, 3, 4, 0)])
    for window in ((-1, 5), (0, 1 << 32)):
        with pytest.raises(ValueError):
            verify_pool_submits_cpu(job, ses, [(1, 2, 3, 4, 0)], *window)
    with pytest.raises(ValueError):
        verify_pool_submits_cpu("job", ses, [(1, 2, 3, 4, 0)])
    with pytest.raises(ValueError):  # the job's extranonce1 gives the size: 1..8
        verify_pool_submits_cpu(Job(b"", b"", 2, b""), [], [(1, 2, 3, 4, 0)])
    verdicts, r = verify_pool_submits_cpu(job, ses, [])
    assert len(verdicts) == 0 and ref.result_tuple(r) == (0,) * 5
    # pairs in place of PoolSession, dicts in place of tuples
    sub = {"extranonce2": 29, "ntime": job.ntime, "nonce": 2083236893, "version": 1, "session": 0}
    verdicts, r = verify_pool_submits_cpu(job, [(b"\xff\xff", DIFF1)], [sub])
    assert ref.as_tuples(verdicts) == [(GENESIS_HASH, 3)] and verdicts[0].is_block and not verdicts[0].is_ntime


# ---- the CPU entry against hashlib ----------------------------------------------------

def test_the_grid_covers_the_field_cases():
    """The four cases the field can meet, by the grid's own labels: five words; the
    block edge inside extranonce1, between the fields, inside extranonce2."""
    labels = [label for label, *_ in ref.layout_grid()]
    assert len(labels) == 900 == len(set(labels))
    assert any(off % 4 == 3 and s1 + s2 == 16 for off, _, s1, s2, _ in labels)
    assert any(off < 64 < off + s1 for off, _, s1, s2, _ in labels)
    assert any(off + s1 == 64 for off, _, s1, s2, _ in labels)
    assert any(off + s1 < 64 < off + s1 + s2 for off, _, s1, s2, _ in labels)


def test_cpu_entry_against_hashlib_over_the_layout_grid():
    grid = ref.layout_grid()
    assert len(grid) == 900 and sum(len(subs) for *_, subs, _ in grid) == 58500
    seen = set()
    for label, job, sessions, subs, want in grid:
        assert len(sessions) == 7 and all(a[4] != b[4] for a, b in zip(subs, subs[1:]))
        assert sessions[0].extranonce1 == bytes(label[2]) and sessions[1].extranonce1 == b"\xff" * label[2]
        assert subs[0][0] == 0 and subs[1][0] == (1 << (8 * label[3])) - 1
        verdicts, r = verify_pool_submits_cpu(job, ref.session_array(sessions), ref.sub_array(subs), *ref.GRID_WINDOW)
        assert ref.as_tuples(verdicts) == want, label
        assert ref.result_tuple(r) == ref.counts(want), label
        seen |= {status for _, status in want}
    # rejects, shares, blocks with and (under the sessions whose target lies below the block target) without
    # SHARE, each inside and outside the window
    assert seen == {0, 1, 2, 3, 8, 9, 10, 11}


@pytest.mark.parametrize("depth", [0, 1, 12, 32])
def test_cpu_entry_branch_depths(depth):
    rng = random.Random(depth)
    job = ref.synthetic_job(rng, 45, 4, 4, 250, depth)
    sessions = ref.synthetic_sessions(rng, 4)
    check(job, sessions, ref.random_subs(rng, 4, 33, 7))


def test_genesis_submission_under_two_sessions():
    job = genesis_job()
    sessions = [PoolSession(b"\xff\xff", DIFF1), PoolSession(b"\x00\x01", DIFF1)]
    subs = [(29, job.ntime, 2083236893, 1, 0), (29, job.ntime, 2083236893, 1, 1)]
    want = check(job, sessions, subs)
    assert want[0] == (GENESIS_HASH, 3) and want[1][1] == 0 and want[1][0] != GENESIS_HASH


def test_per_session_targets_flip_share_exactly_at_equality():
    job, sessions, subs, expect = ref.ladder_case()
    assert len(sessions) == 29
    assert check(job, sessions, subs) == expect


def test_block_without_share():
    rng = random.Random(13)
    job = ref.synthetic_job(rng, 10, 4, 4, 100, 0, nbits=0x2100ffff)  # the block target: 0xffff << 240
    sessions = [PoolSession(rng.randbytes(4), 0), PoolSession(rng.randbytes(4), ref.U256)]
    subs = ref.random_subs(rng, 4, 64, 2)
    want = check(job, sessions, subs)
    # all but one hash in 2^16 meets that block target: BLOCK alone under target 0, with SHARE under 2^256 - 1
    assert {st for (_, st), s in zip(want, subs) if s[4] == 0} == {2}
    assert {st for (_, st), s in zip(want, subs) if s[4] == 1} == {3}
    # an nbits that does not decode leaves BLOCK clear everywhere
    for nbits in (0x1d80ffff, 0x2300ffff):
        job = ref.synthetic_job(rng, 10, 4, 4, 100, 0, nbits=nbits)
        assert {st for _, st in check(job, sessions, subs)} == {0, 1}


def test_ntime_window():
    rng = random.Random(17)
    job = ref.synthetic_job(rng, 70, 2, 2, 150, 1)
    sessions = [PoolSession(rng.randbytes(2), ref.U256), PoolSession(rng.randbytes(2), 0)]
    for lo, hi, subs, flagged in ref.window_cases():
        want = check(job, sessions, subs, lo, hi)
        assert [bool(st & ref.NTIME) for _, st in want] == flagged, (lo, hi)
        # the flag is OR-ed in: the hash and SHARE are what they are without a window
        assert [(h, st & ~ref.NTIME) for h, st in want] == check(job, sessions, subs)


def test_invalid_entries():
    job, sessions, subs = ref.invalid_case()
    want = check(job, sessions, subs, 100, 200)  # every ntime lies outside: an INVALID entry carries no NTIME
    assert [w == ref.INVALID_VERDICT for w in want[:7]] == [True, False, True, True, True, False, True]
    assert want[1][1] == want[5][1] == 9
    verdicts, r = verify_pool_submits_cpu(job, sessions, subs, 100, 200)
    assert bytes(verdicts[0].hash) == b"\xff" * 32 and verdicts[0].status == 4 and r.invalid == 50 and r.ntime == 20
    # no sessions at all: every entry is INVALID (sessions may be NULL)
    want = check(job, [], subs)
    assert all(w == ref.INVALID_VERDICT for w in want)
    out = (_lib.JobVerdict * len(subs))()
    r = _lib.PoolVerifyResult()
    assert _lib.load().bm_pool_verify_cpu(ctypes.byref(job.struct), None, 0, ref.sub_array(subs), len(subs), 0, ref.U32,
                                          out, ctypes.byref(r)) == _lib.BM_OK
    assert ref.as_tuples(out) == want and ref.result_tuple(r) == (70, 0, 0, 70, 0)
    # extranonce2_size 8 accepts 2^64 - 1
    rng = random.Random(15)
    job8 = ref.synthetic_job(rng, 61, 8, 8, 130, 0)
    want = check(job8, [PoolSession(rng.randbytes(8), ref.U256)], [(ref.U64, 1, 2, 3, 0), (ref.U64, 1, 2, 3, 1)])
    assert want[0][1] == 1 and want[1] == ref.INVALID_VERDICT


def test_bytes_past_the_size_do_not_count():
    """Only the first extranonce1_len bytes of a session's extranonce1 count, and
    the job's own extranonce1 bytes do not."""
    rng = random.Random(19)
    job = ref.synthetic_job(rng, 61, 3, 5, 200, 2)
    sessions = ref.synthetic_sessions(rng, 3)
    subs = ref.random_subs(rng, 5, 20, 7)
    a, _ = verify_pool_submits_cpu(job, ref.session_array(sessions, junk=0x00), ref.sub_array(subs))
    b, _ = verify_pool_submits_cpu(job, ref.session_array(sessions, junk=0xFF), ref.sub_array(subs))
    other = Job(job.coinb1, b"\x00\x00\x00", 5, job.coinb2, job.branch, job.prevhash, job.version, job.nbits, job.ntime)
    c, _ = verify_pool_submits_cpu(other, sessions, subs)
    assert bytes(a) == bytes(b) == bytes(c)
    assert ref.as_tuples(a) == [ref.verdict(job, sessions, s) for s in subs]


# ---- parse_pool_submit and the command line -------------------------------------------

def test_parse_pool_submit():
    job = genesis_job()
    index = {"satoshi.1": 0, "hal.1": 1}
    good = json.loads(GENESIS_PARAMS)
    assert parse_pool_submit(good, job, index) == {"extranonce2": 29, "extranonce2_size": 2, "ntime": 0x495fab29,
                                                   "nonce": 2083236893, "version": 1, "session": 0}
    assert parse_pool_submit(["hal.1"] + good[1:5], job, index)["session"] == 1
    assert parse_pool_submit(good[:5] + ["00002000"], job, index, 0x2000)["version"] == 0x2001

    def reason(params, mask=0x1fffe000):
        with pytest.raises(ValueError) as e:
            parse_pool_submit(params, job, index, mask)
        return str(e.value).split(":")[0]

    for worker in ("satoshi.2", "", 5, None, ["satoshi.1"]):
        assert reason([worker] + good[1:]) == "worker", worker
    assert reason(good[:1] + ["other"] + good[2:]) == "job-id"
    assert reason(good[:2] + ["1d"] + good[3:]) == "extranonce2"
    assert reason(good[:3] + ["495fab2"] + good[4:]) == "malformed"
    assert reason(good[:5] + ["00000001"]) == "version-bits"
    for params in (good[:4], good + ["x"], [], "genesis", None):
        assert reason(params) == "malformed"


def run(text, *flags, sessions=SESSIONS_PATH):
    out = io.StringIO()
    rc = pool_verify.main([JOB_PATH, sessions, "-", "--cpu", *flags], out=out, stdin=io.StringIO(text))
    return rc, out.getvalue().splitlines()


def test_cli_genesis_round_trip():
    """stratum_job's printed line for the README's genesis example gives its Block
    line back under satoshi.1; the same params under the other worker's name are
    hashed under another extranonce1 and land above the target."""
    block = "Block %s %064x" % (GENESIS_PARAMS, GENESIS_HASH)
    assert run(MINED) == (0, [block, "Verified 1 Accepted 1 Blocks 1 Rejected 0"])
    assert run(block + "\n") == (0, [block, "Verified 1 Accepted 1 Blocks 1 Rejected 0"])
    other = GENESIS_PARAMS.replace("satoshi.1", "hal.1")
    assert run(MINED.replace("satoshi.1", "hal.1")) == (0, ["Reject above-target " + other,
                                                            "Verified 1 Accepted 0 Blocks 0 Rejected 1"])


def test_cli_reasons_and_the_window(tmp_path):
    good = json.loads(GENESIS_PARAMS)

    def with_(i, v):
        return json.dumps(good[:i] + [v] + good[i + 1:], separators=(",", ":"))

    block = "Block %s %064x" % (GENESIS_PARAMS, GENESIS_HASH)
    lines = [GENESIS_PARAMS, "Submit " + with_(0, "nobody"), with_(0, "hal.1"), with_(4, "7c2bac1e"), with_(2, "1d"),
             with_(1, "other"), with_(5, "00000001"), "hello", "", "Shares 1 Best 00 001d 5 00000001"]
    rejects = ["Reject worker " + with_(0, "nobody"), "Reject above-target " + with_(0, "hal.1"),
               "Reject above-target " + with_(4, "7c2bac1e"), "Reject extranonce2 " + with_(2, "1d"),
               "Reject job-id " + with_(1, "other"), "Reject version-bits " + with_(5, "00000001"),
               "Reject malformed hello"]
    text = "\n".join(lines) + "\n"
    assert run(text) == (0, [block] + rejects + ["Verified 8 Accepted 1 Blocks 1 Rejected 7"])
    # the window: inclusive at both ends, decimal or hex; outside it the block is a reject, and so is every
    # other hashed line
    ntime = 0x495fab29
    for lo, hi in ((str(ntime), str(ntime)), ("0", "0x495fab29"), ("0x495fab29", str(ref.U32))):
        assert run(text, "--ntime-window", lo, hi)[1][0] == block
    for lo, hi in ((str(ntime + 1), str(ref.U32)), ("0", str(ntime - 1))):
        got = run(text, "--ntime-window", lo, hi)[1]
        assert got[0] == "Reject ntime " + GENESIS_PARAMS and got[1] == rejects[0]
        assert got[2:4] == ["Reject ntime " + with_(0, "hal.1"), "Reject ntime " + with_(4, "7c2bac1e")]
        assert got[4:-1] == rejects[3:] and got[-1] == "Verified 8 Accepted 0 Blocks 0 Rejected 8"
    # a worker at an easy difficulty accepts what satoshi.1's rejects: the targets are per session
    easy = tmp_path / "sessions.json"
    easy.write_text(json.dumps({"workers": {"satoshi.1": {"extranonce1": "ffff", "difficulty": 1},
                                            "easy.1": {"extranonce1": "ffff", "difficulty": 2.0 ** -40}}}))
    above, eased = with_(4, "7c2bac1e"), json.dumps(["easy.1"] + good[1:4] + ["7c2bac1e"] + good[5:], separators=(",", ":"))
    h = ref.verdict(genesis_job(), [PoolSession(b"\xff\xff", ref.U256)], (29, ntime, 0x7c2bac1e, 1, 0))[0]
    assert run(above + "\n" + eased + "\n", sessions=str(easy)) == (
        0, ["Reject above-target " + above, "Accept %s %064x" % (eased, h), "Verified 2 Accepted 1 Blocks 0 Rejected 1"])
    assert run("") == (0, ["Verified 0 Accepted 0 Blocks 0 Rejected 0"])


def test_cli_argument_errors_exit_2(tmp_path):
    assert pool_verify.main([]) == 2
    assert pool_verify.main([JOB_PATH]) == 2
    assert pool_verify.main([JOB_PATH + ".missing", SESSIONS_PATH, "-", "--cpu"], stdin=io.StringIO("")) == 2
    assert pool_verify.main([JOB_PATH, SESSIONS_PATH + ".missing", "-", "--cpu"], stdin=io.StringIO("")) == 2
    assert pool_verify.main([JOB_PATH, SESSIONS_PATH, str(tmp_path / "missing.txt"), "--cpu"]) == 2
    assert pool_verify.main([JOB_PATH, SESSIONS_PATH, "-", "--cpu", "--ntime-window", "1"]) == 2
    assert pool_verify.main([JOB_PATH, SESSIONS_PATH, "-", "--cpu", "--ntime-window", "a", "b"], stdin=io.StringIO("")) == 2
    for bad in ({"workers": {"w": {"extranonce1": "ffffff", "difficulty": 1}}},   # not the job's size
                {"workers": {"w": {"extranonce1": "ffff"}}}, {"workers": {"w": {"extranonce1": "ffff", "difficulty": 0}}},
                {"workers": []}, []):
        path = tmp_path / "bad.json"
        path.write_text(json.dumps(bad))
        assert pool_verify.main([JOB_PATH, str(path), "-", "--cpu"], stdin=io.StringIO("")) == 2, bad
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.pool_verify", JOB_PATH, SESSIONS_PATH, "--cpu"],
                       input=MINED, capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.splitlines() == ["Block %s %064x" % (GENESIS_PARAMS, GENESIS_HASH),
                                                           "Verified 1 Accepted 1 Blocks 1 Rejected 0"], r.stderr
