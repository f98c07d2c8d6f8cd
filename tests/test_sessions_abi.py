"""The session table on the CPU (no GPU): bm_target_from_difficulty_fx and the CPU
bm_sessions_t, the specification of a device table, against the pure-Python model of
tests/sessions_ref.py -- big integers, hashlib, a Python set and a dict of rows --
never against the library itself, but where a test says so.  wide_arithmetic (the rule
at full 64-bit width) and dense_changes (full and nearly full change lists) are the
scenarios a device table runs too (tests/test_gpu_sessions.py)."""
import ctypes
import io
import os
import random

import pytest

from conftest import GOLDEN
from distributed_bitcoin_minter_amd import (Ledger, SessionTable, ShareSet, VardiffPolicy, _lib, difficulty_fx_to_target,
                                            difficulty_to_target)
from distributed_bitcoin_minter_amd import pool_jobs, pool_ledger
from distributed_bitcoin_minter_amd.pool_verify import _load_json, load_sessions
import jobs_verify_ref as jref
import ledger_ref as lref
import sessions_ref as sref


def test_abi_has_the_entries():
    lib = _lib.load()
    for name in ("bm_target_from_difficulty_fx", "bm_sessions_create", "bm_sessions_create_cpu", "bm_sessions_destroy",
                 "bm_sessions_clear", "bm_sessions_count", "bm_sessions_set", "bm_sessions_get", "bm_sessions_verify_jobs",
                 "bm_sessions_retarget"):
        assert hasattr(lib, name), name
    assert lib.bm_abi_version() == 7
    assert ctypes.sizeof(_lib.SessionInit) == 24 and ctypes.sizeof(_lib.SessionState) == 32
    assert ctypes.sizeof(_lib.VardiffChange) == 56 and ctypes.sizeof(_lib.VardiffResult) == 40
    assert ctypes.sizeof(_lib.VardiffPolicyStruct) == 48


def test_target_from_difficulty_fx():
    """The listed difficulties and 200 random ones against the big-integer quotient;
    2^32 (difficulty 1) is 0xffff * 2^208; nothing saturates."""
    rng = random.Random(1)
    values = list(sref.DIFFICULTIES) + [rng.getrandbits(rng.randrange(1, 65)) or 1 for _ in range(200)]
    for d in values:
        assert difficulty_fx_to_target(d) == (0xffff << 240) // d, d
    assert difficulty_fx_to_target(1 << 32) == 0xffff << 208
    assert difficulty_fx_to_target(1) == 0xffff << 240 and difficulty_fx_to_target(sref.U64) == (0xffff << 240) // sref.U64
    f = _lib.load().bm_target_from_difficulty_fx
    buf = (ctypes.c_uint8 * 32)(*([0xA5] * 32))
    assert f(0, buf) == _lib.BM_EINVAL and bytes(buf) == b"\xa5" * 32
    assert f(1, None) == _lib.BM_EINVAL
    for bad in (0, -1, 1 << 64, 1.0, True):
        with pytest.raises(ValueError):
            difficulty_fx_to_target(bad)


def test_target_fx_equals_the_double_function_below_2_53():
    rng = random.Random(2)
    values = [1, 2, 3, 0xffff, 0x10000, 1 << 32, (1 << 32) + 1, (1 << 53) - 1, 4096, 16384]
    values += [rng.getrandbits(rng.randrange(1, 54)) or 1 for _ in range(200)]
    for d in values:
        assert d < 1 << 53
        assert difficulty_fx_to_target(d) == difficulty_to_target(d / 2.0 ** 32), d  # d / 2^32 is exact in a double


def test_creation_and_python_arguments():
    sref.creation()
    for bad in (0, -1, _lib.BM_MAX_POOL_SESSIONS + 1, 1.5, True):
        with pytest.raises(ValueError):
            SessionTable.cpu(bad)
    with SessionTable.cpu(2) as t:
        for bad in ([(b"123456789", 1, 0)], [(b"1", -1, 0)], [(b"1", 1, 1 << 32)], [(b"1", 1)]):
            with pytest.raises(ValueError):
                t.set(bad, 0)
        with pytest.raises(ValueError):
            t.set([(b"1", 1, 0)], 0, index=[0, 1])
        with pytest.raises(_lib.BtcMinerError):
            t.set([(b"1", 1, 0)], 0, index=[2])
        with pytest.raises(ValueError):
            t.retarget(0, VardiffPolicy(burst=-1))
        assert t.count == 0
    with pytest.raises(ValueError):
        t.count


@pytest.mark.parametrize("scenario", [sref.division, sref.division_by_retarget, sref.set_semantics, sref.edge_cases,
                                      sref.burst_and_clock, sref.wide_arithmetic, sref.dense_changes],
                         ids=lambda f: f.__name__)
def test_cpu_table(scenario):
    scenario(SessionTable.cpu)


def test_sequence_on_the_cpu():
    sref.sequence(SessionTable.cpu, Ledger.cpu, ShareSet.cpu)


def test_contention_on_the_cpu():
    sref.contention(SessionTable.cpu, ShareSet.cpu)


def test_refusals_leave_everything_alone():
    sref.refusals(SessionTable.cpu, Ledger.cpu, ShareSet.cpu)


def ledger_raw(ledger, share_set, jobs, ses, acc, wgt, subs):
    """bm_ledger_verify_jobs on the very arrays bm_sessions_get returned, into canary-filled arrays."""
    n, nses = len(subs), len(ses)
    out = (_lib.JobVerdict * (n + 1))()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    r = _lib.LedgerResult()
    jarr, _keep = _lib._jobs_array(jobs)
    rc = ledger._lib.bm_ledger_verify_jobs(ledger.handle, share_set.handle if share_set is not None else None, jarr,
                                           len(jarr), ses, nses, (ctypes.c_uint32 * nses)(*acc),
                                           (ctypes.c_uint64 * nses)(*wgt), jref.sub_array(subs), n, out, ctypes.byref(r))
    return rc, out, r


def equivalent(jobs, entries, batches, rows):
    """bm_sessions_verify_jobs against bm_ledger_verify_jobs on the arrays that
    bm_sessions_get returns, byte for byte: the library as its own witness here, by the
    specification's wording.  With and without a ledger and a set."""
    for with_ledger in (True, False):
        for with_set in (True, False):
            with SessionTable.cpu(len(entries) + 3) as table, Ledger.cpu(rows) as a, Ledger.cpu(rows) as b, \
                    ShareSet.cpu(4096) as sa, ShareSet.cpu(4096) as sb:
                table.set(entries, 0)
                ses, acc, wgt = table.get()
                tally = [0] * len(entries)
                for subs in batches:
                    rc, out, r = sref.raw_verify(table, a if with_ledger else None, sa if with_set else None, jobs, subs)
                    rc2, out2, r2 = ledger_raw(b, sb if with_set else None, jobs, ses, acc, wgt, subs)
                    assert rc == rc2 == _lib.BM_OK and bytes(out) == bytes(out2) and bytes(r) == bytes(r2)
                    assert sa.count == sb.count
                    assert bytes(a.read()) == (bytes(b.read()) if with_ledger else bytes(Ledger.cpu(rows).read()))
                    for s, v in zip(subs, out):
                        if s[4] < len(entries) and lref.classify(v.status) == lref.ACCEPTED:
                            tally[s[4]] += 1
                    assert [s.accepted for s in table.state()] == tally
                assert sum(tally) > 0


def test_equivalence_over_the_ledger_fixtures():
    """The pool_ledger fixtures: the workers at their difficulties as a table."""
    paths = [os.path.join(GOLDEN, "stratum_genesis_job.json"), os.path.join(GOLDEN, "stratum_second_job.json")]
    jobs, by_id, masks, size = pool_jobs.load_jobs(paths, None)
    obj = _load_json(os.path.join(GOLDEN, "stratum_ledger_sessions.json"))
    sessions, index = load_sessions(obj, size)
    names, accounts, weights = pool_ledger.account_map(obj["workers"], index, False)
    entries = [(s.extranonce1, w, a) for s, a, w in zip(sessions, accounts, weights)]
    with open(os.path.join(GOLDEN, "stratum_ledger_submits.txt")) as f:
        lines = f.read().splitlines()
    batches = []

    def record(subs):
        batches.append([tuple(s[k] for k in ("extranonce2", "ntime", "nonce", "version", "session", "job")) for s in subs])
        return pool_jobs.verify_jobs_submits_cpu(jobs, sessions, subs)

    pool_jobs.jobs_lines(lines, by_id, masks, index, record, 4)
    assert len(batches) == 3
    with SessionTable.cpu(len(entries)) as table:  # the table's targets are the fixtures'
        table.set(entries, 0)
        assert [int.from_bytes(bytes(s.target), "big") for s in table.get()[0]] == [s.target for s in sessions]
    equivalent(jobs, entries, batches, len(names))


def test_equivalence_over_a_generated_batch():
    jobs, _, subs, _ = jref.large_case()
    rng = random.Random(3)
    entries = [(rng.randbytes(8), rng.choice((0, 1, 1, 3, 1 << 16, rng.getrandbits(64) | 1)), s % 37) for s in range(500)]
    equivalent(jobs, entries, [list(subs[:2000]), list(subs[1500:3000])], 37)
