"""Verification over several jobs: the C ABI, the ctypes mirrors and the CPU entries
(no GPU).  bm_jobs_verify_cpu and bm_share_set_verify_jobs on a CPU set against
hashlib (tests/jobs_verify_ref.py) over the grouping scenarios, the refusals with
canaries, the struct layouts against a compiled C consumer, the Python layer and the
C++ wrapper.  The calls are additive, so the ABI version stays 7."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import (Job, PoolJob, PoolSession, ShareSet, _lib, parse_jobs_submit,
                                            verify_jobs_submits_cpu, verify_pool_submits_cpu)
import jobs_verify_ref as jref
import pool_verify_ref as ref

JOB_FIELDS = ["job", "ntime_lo", "ntime_hi"]
SUBMIT_FIELDS = ["extranonce2", "ntime", "nonce", "version", "session", "job", "reserved"]


def cpu_call(*a):
    return _lib.load().bm_jobs_verify_cpu(*a)


# ---- the ABI ---------------------------------------------------------------------------

def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in ("bm_jobs_verify_cpu", "bm_jobs_verify_gpu", "bm_share_set_verify_jobs"):
        assert hasattr(lib, name), name
    names = {"PoolJob", "JobsSubmit", "parse_jobs_submit", "verify_jobs_submits_cpu", "BM_MAX_POOL_JOBS"}
    assert names <= set(pkg.__all__)
    assert all(getattr(pkg, n) is getattr(_lib, n) for n in names)
    assert hasattr(_lib.Context, "verify_jobs_submits") and hasattr(ShareSet, "verify_jobs")
    assert _lib.BM_MAX_POOL_JOBS == 64


def test_struct_layouts_match_the_header():
    """Size and every field offset of the two structs, and the constant, from a C
    program compiled against include/btcminer.h."""
    structs = {"bm_pool_job_t": (_lib.PoolJobStruct, JOB_FIELDS), "bm_jobs_submit_t": (_lib.JobsSubmit, SUBMIT_FIELDS)}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name}.size %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("max %u\\n", BM_MAX_POOL_JOBS);',
              'printf("job %zu\\n", sizeof(bm_job_t));', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out if ln.strip()}
    assert got["abi"] == [7] and got["max"] == [64]
    assert got["job"] == [ctypes.sizeof(_lib.JobStruct)]
    assert got["bm_jobs_submit_t.size"] == [ctypes.sizeof(_lib.JobsSubmit)] == [32]
    assert [got[f"bm_jobs_submit_t.{f}"][0] for f in SUBMIT_FIELDS] == [0, 8, 12, 16, 20, 24, 28]
    assert got["bm_pool_job_t.size"] == [ctypes.sizeof(_lib.PoolJobStruct)]
    assert got["bm_pool_job_t.size"][0] == got["job"][0] + 8 and got["bm_pool_job_t.job"] == [0]
    for name, (mirror, fields) in structs.items():
        for f in fields:
            assert got[f"{name}.{f}"] == [getattr(mirror, f).offset], (name, f)


def _refusals(call, result=_lib.PoolVerifyResult):
    """Every refusal that needs no context or set, through call(jobs, njobs,
    sessions, nsessions, submits, n, verdicts, out): BM_EINVAL, verdicts and out
    untouched."""
    jobs, sessions = jref.three_jobs()
    jarr, _keep = _lib._jobs_array(jobs)
    ses = ref.session_array(sessions)
    subs = jref.sub_array([(1, 2, 3, 4, 0, 0), (1, 2, 3, 4, 1, 1), (1, 2, 3, 4, 2, 2)])
    verdicts = (_lib.JobVerdict * 3)()
    ctypes.memset(verdicts, 0xA5, ctypes.sizeof(verdicts))
    r = result()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    before = bytes(verdicts), bytes(r)
    out = ctypes.byref(r)
    E = _lib.BM_EINVAL
    many = (_lib.PoolJobStruct * 65)(*([jarr[0]] * 65))
    assert call(None, 3, ses, 7, subs, 3, verdicts, out) == E
    assert call(many, 65, ses, 7, subs, 3, verdicts, out) == E
    assert call(jarr, 3, None, 7, subs, 3, verdicts, out) == E
    assert call(jarr, 3, ses, 7, None, 3, verdicts, out) == E
    assert call(jarr, 3, ses, 7, subs, 3, None, out) == E
    assert call(jarr, 3, ses, 7, subs, 3, verdicts, None) == E
    assert call(jarr, 3, ses, 7, subs, _lib.BM_MAX_JOB_SUBMITS + 1, verdicts, out) == E  # before anything is read
    assert call(jarr, 3, ses, _lib.BM_MAX_POOL_SESSIONS + 1, subs, 3, verdicts, out) == E
    assert call(None, 3, ses, 7, None, 0, None, out) == E          # n == 0 excuses the two arrays only
    assert call(jarr, 3, ses, 7, None, 0, None, None) == E
    for k in range(3):  # each job is checked, the last one too
        for kw in (dict(extranonce1_len=0), dict(extranonce1_len=9), dict(extranonce2_size=0), dict(extranonce2_size=9),
                   dict(nbranch=33), dict(coinb1=None), dict(coinb2_len=1 << 16), dict(coinb1_len=(1 << 64) - 1)):
            bad, _keep2 = _lib._jobs_array(jobs)
            for name, v in kw.items():
                setattr(bad[k].job, name, v)
            assert call(bad, 3, ses, 7, subs, 3, verdicts, out) == E, (k, kw)
            assert call(bad, 3, ses, 7, None, 0, None, out) == E, (k, kw)  # with an empty batch too
    assert (bytes(verdicts), bytes(r)) == before
    return jarr, ses, subs, verdicts, r, before


def test_cpu_entry_refusals_and_empty_batch():
    f = _lib.load().bm_jobs_verify_cpu
    jarr, ses, subs, verdicts, r, before = _refusals(f)
    # n == 0: zeros, no array touched or needed
    assert f(jarr, 3, ses, 7, None, 0, None, ctypes.byref(r)) == _lib.BM_OK and ref.result_tuple(r) == (0,) * 5
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    assert f(None, 0, None, 0, subs, 0, verdicts, ctypes.byref(r)) == _lib.BM_OK and ref.result_tuple(r) == (0,) * 5
    assert bytes(verdicts) == before[0]
    # a batch shorter than its arrays leaves the rest alone
    assert f(jarr, 3, ses, 7, subs, 2, verdicts, ctypes.byref(r)) == _lib.BM_OK and r.n == 2
    assert bytes(verdicts[2]) == b"\xa5" * 40 and bytes(verdicts[1]) != b"\xa5" * 40
    # exactly BM_MAX_POOL_JOBS jobs are fine
    many = (_lib.PoolJobStruct * 64)(*([jarr[0]] * 63 + [jarr[1]]))
    last = jref.sub_array([(1, 2, 3, 4, 1, 63)])
    one = (_lib.JobVerdict * 1)()
    assert f(many, 64, ses, 7, last, 1, one, ctypes.byref(r)) == _lib.BM_OK
    assert bytes(one[0]) == bytes(verdicts[1])


def test_gpu_entry_refuses_before_it_touches_the_context():
    """The same refusals through bm_jobs_verify_gpu over a stand-in context pointer, and a NULL context."""
    f = _lib.load().bm_jobs_verify_gpu
    fake = ctypes.c_void_p(1)
    jarr, ses, subs, verdicts, r, before = _refusals(lambda *a: f(fake, *a))
    assert f(None, jarr, 3, ses, 7, subs, 3, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
    assert (bytes(verdicts), bytes(r)) == before


def test_share_set_entry_refusals():
    f = _lib.load().bm_share_set_verify_jobs
    with ShareSet.cpu(8) as s:
        jarr, ses, subs, verdicts, r, before = _refusals(lambda *a: f(s.handle, *a), _lib.ShareSetResult)
        assert f(None, jarr, 3, ses, 7, subs, 3, verdicts, ctypes.byref(r)) == _lib.BM_EINVAL
        assert (bytes(verdicts), bytes(r)) == before and s.count == 0
        assert f(s.handle, jarr, 3, ses, 7, None, 0, None, ctypes.byref(r)) == _lib.BM_OK
        assert jref.ss.result_tuple(r) == (0,) * 8


def test_python_layer():
    jobs, sessions = jref.three_jobs()
    good = (1, 2, 3, 4, 0, 0)
    for bad in ([good[:5]], [good + (0,)], [(-1,) + good[1:]], [good[:5] + (1 << 32,)], [good[:5] + (-1,)],
                [{"extranonce2": 1, "ntime": 2, "nonce": 3, "version": 4, "session": 0}]):
        with pytest.raises((ValueError, KeyError)):
            verify_jobs_submits_cpu(jobs, sessions, bad)
    with pytest.raises(ValueError):  # a session shorter than the longest extranonce1 the jobs state
        verify_jobs_submits_cpu(jobs, [PoolSession(b"\x01\x02\x03\x04", 0)], [good])
    with pytest.raises(ValueError):
        verify_jobs_submits_cpu([jobs[0]] * 65, sessions, [good])
    with pytest.raises(ValueError):
        PoolJob("job")
    with pytest.raises(ValueError):
        PoolJob(Job(b"", b"", 2, b""))
    with pytest.raises(ValueError):
        PoolJob(jobs[0].job, 0, 1 << 32)
    verdicts, r = verify_jobs_submits_cpu(jobs, sessions, [])
    assert len(verdicts) == 0 and ref.result_tuple(r) == (0,) * 5
    # a bare Job has no window; a triple is a PoolJob; dicts in place of tuples
    sub = dict(zip(("extranonce2", "ntime", "nonce", "version", "session", "job"), (7, 1, 2, 3, 4, 1)))
    a, _ = verify_jobs_submits_cpu([jobs[0].job, (jobs[1].job, 5, 7)], sessions, [sub, (7, 5, 2, 3, 4, 1)])
    want = jref.verdicts([PoolJob(jobs[0].job), jobs[1]], sessions, [(7, 1, 2, 3, 4, 1), (7, 5, 2, 3, 4, 1)])
    assert ref.as_tuples(a) == want and a[0].is_ntime and not a[1].is_ntime


def test_parse_jobs_submit():
    jobs, _ = jref.three_jobs()
    a = Job(b"\x01" * 10, b"\x00\x00", 2, b"\x02" * 5, job_id="a", version=0x20000000)
    b = Job(b"\x01" * 10, b"\x00\x00", 4, b"\x02" * 5, job_id="b")
    by_id = {"a": (0, a), "b": (1, b)}
    index = {"w": 3}
    assert parse_jobs_submit(["w", "b", "0000001d", "00000005", "00000006"], by_id, index) == {
        "extranonce2": 29, "extranonce2_size": 4, "ntime": 5, "nonce": 6, "version": 0, "session": 3, "job": 1}
    assert parse_jobs_submit(["w", "a", "001d", "00000005", "00000006", "00002000"], by_id, index)["version"] == 0x20002000

    def reason(params):
        with pytest.raises(ValueError) as e:
            parse_jobs_submit(params, by_id, index)
        return str(e.value).split(":")[0]

    assert reason(["w", "c", "001d", "00000005", "00000006"]) == "job"
    assert reason(["w", 5, "001d", "00000005", "00000006"]) == "job"
    assert reason(["w", "b", "001d", "00000005", "00000006"]) == "extranonce2"  # b's extranonce2 has four bytes
    assert reason(["x", "a", "001d", "00000005", "00000006"]) == "worker"
    assert reason(["w", "a", "001d", "0000005", "00000006"]) == "malformed"
    assert reason(["w", "a"]) == "malformed" and reason(None) == "malformed"


# ---- the CPU entry against hashlib: the grouping scenarios -----------------------------------

def test_the_three_jobs_differ_in_everything_uniform():
    jref.layouts_differ()


@pytest.mark.parametrize("n", jref.BATCH_SIZES)
def test_round_robin_batches(n):
    jref.round_robin(cpu_call, n)


@pytest.mark.parametrize("counts", jref.PER_JOB_COUNTS)
def test_per_job_counts(counts):
    jref.per_job_counts(cpu_call, counts)


def test_all_on_the_last_job():
    jref.last_job_only(cpu_call)


def test_malformed_unused_job_is_refused():
    jref.malformed_unused_job(cpu_call)


def test_unknown_jobs_among_valid_entries():
    jref.unknown_jobs(cpu_call)


def test_no_jobs_and_unknown_sessions():
    jref.no_jobs_and_unknown_sessions(cpu_call)


def test_verdicts_do_not_depend_on_the_arrangement():
    jref.arrangement(cpu_call)


def test_a_verdict_is_the_pool_entrys_for_its_job():
    """verdicts[i] is bm_pool_verify_cpu's for that submission alone under its job and window."""
    jobs, sessions, subs, want = jref.large_case()
    views = jref.session_views(jobs, sessions)
    got, r = verify_jobs_submits_cpu(jobs, sessions, jref.sub_array(subs))
    assert ref.as_tuples(got) == want and ref.result_tuple(r) == ref.counts(want)
    for i in range(0, len(subs), 97):
        j = subs[i][5]
        if j >= len(jobs):
            assert ref.as_tuples(got[i:i + 1]) == [jref.INVALID_VERDICT]
            continue
        one, _ = verify_pool_submits_cpu(jobs[j].job, views[j], [subs[i][:5]], jobs[j].ntime_lo, jobs[j].ntime_hi)
        assert bytes(one[0]) == bytes(got[i])


# ---- the share set on the CPU -------------------------------------------------------------------

@pytest.mark.parametrize("scenario", [jref.set_across_batches, jref.set_identical_jobs, jref.set_repeat_across_groups,
                                      jref.set_full, jref.set_alternating], ids=lambda f: f.__name__)
def test_cpu_share_set(scenario):
    scenario(ShareSet.cpu)


def test_cpu_share_set_python_call():
    jobs, sessions = jref.open_jobs()
    with ShareSet.cpu(4) as s:
        v, r = s.verify_jobs(jobs, sessions, [(1, 2, 3, 4, 0, 0), (1, 2, 3, 4, 0, 0), (1, 2, 3, 4, 0, 9)])
        assert [x.status for x in v] == [1, 17, 4] and (r.recorded, r.duplicates, r.count, r.invalid) == (1, 1, 1, 1)
        with pytest.raises(_lib.BtcMinerError) as e:
            s.verify_jobs(jobs, sessions, [(k, 2, 3, 4, 0, 0) for k in range(10, 14)])
        assert e.value.status == _lib.BM_EFULL and s.count == 1


# ---- the C++ wrapper ------------------------------------------------------------------------------

CPP = r"""
#include <cstdio>
#include "btcminer.hpp"
int main() {
    btcminer::Job a, b;
    a.coinb1 = {1, 2, 3};
    a.extranonce1 = {9, 9};
    a.extranonce2_size = 2;
    a.coinb2 = {4, 5};
    a.nbits = 0x1d00ffff;
    b = a;
    b.coinb2 = {6};
    b.branch.assign(32, 0x11);
    std::vector<btcminer::PoolJob> jobs = {{&a, 0, 10}, {&b, 5, 5}};
    std::vector<bm_pool_session_t> ses(1);
    for (auto& x : ses[0].target) x = 0xFF;
    for (auto& x : ses[0].extranonce1) x = 7;
    bm_jobs_submit_t subs[4] = {{1, 2, 3, 4, 0, 0, 0}, {1, 2, 3, 4, 0, 1, 0}, {1, 2, 3, 4, 0, 2, 0}, {1, 2, 3, 4, 0, 0, 0}};
    std::vector<bm_job_verdict_t> v, w, one;
    bm_pool_verify_result_t r = btcminer::verify_jobs_cpu(jobs, ses, subs, 4, v);
    std::printf("%d %d %d %d\n", (int)r.n, (int)r.shares, (int)r.invalid, (int)r.ntime);
    std::printf("%u %u %u %u\n", v[0].status, v[1].status, v[2].status, v[3].status);
    bm_pool_submit_t ps[1] = {{1, 2, 3, 4, 0}};
    btcminer::verify_pool_submits_cpu(b, ses, ps, 1, one, 5, 5);
    std::printf("%d\n", std::memcmp(&one[0], &v[1], sizeof one[0]) == 0);
    btcminer::ShareSet set = btcminer::ShareSet::cpu(4);
    bm_share_set_result_t s = set.verify_jobs(jobs, ses, subs, 4, w);
    std::printf("%d %d %d %u\n", (int)s.recorded, (int)s.duplicates, (int)set.count(), w[3].status);
    try {
        btcminer::PoolJob none;
        btcminer::verify_jobs_cpu({none}, ses, subs, 4, v);
        std::printf("no error\n");
    } catch (const btcminer::Error& e) {
        std::printf("status %d kept %zu\n", e.status(), v.size());
    }
    r = btcminer::verify_jobs_cpu({}, ses, subs, 4, v);
    std::printf("%d\n", (int)r.invalid);
    return 0;
}
"""


def test_cpp_wrapper():
    """include/btcminer.hpp's verify_jobs_cpu and ShareSet::verify_jobs over a CPU set."""
    pkg_dir = os.path.dirname(_lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "wrapper.cpp"), os.path.join(d, "wrapper")
        with open(src, "w") as f:
            f.write(CPP)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                               "-L", pkg_dir, "-lbtcminer", "-Wl,-rpath," + pkg_dir, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    assert out == ["4 3 1 1", "1 9 4 1", "1", "2 1 2 17", "status -1 kept 4", "4"], out
