"""The ledger: the C ABI, the ctypes mirrors and the CPU entries (no GPU).
bm_ledger_verify_jobs on a CPU ledger, with a CPU set and without one, against
hashlib, a Python set and a dict of rows (tests/ledger_ref.py); the refusals with
canaries; the struct layouts against a compiled C consumer; the Python layer and the
C++ wrapper.  The calls are additive, so the ABI version stays 7."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
import distributed_bitcoin_minter_amd as pkg
from distributed_bitcoin_minter_amd import BtcMinerError, Ledger, ShareSet, _lib
import jobs_verify_ref as jref
import ledger_ref as lref
import pool_verify_ref as ref

ROW_FIELDS = ["accepted", "blocks", "above_target", "ntime", "duplicates", "invalid", "work", "best"]
RESULT_FIELDS = ["n", "shares", "blocks", "invalid", "ntime", "duplicates", "recorded", "count", "credited",
                 "unattributed", "work"]
CALLS = ("bm_ledger_create", "bm_ledger_create_cpu", "bm_ledger_destroy", "bm_ledger_clear", "bm_ledger_rows",
         "bm_ledger_read", "bm_ledger_drain", "bm_ledger_set_peel", "bm_ledger_verify_jobs")


def test_symbols_exported():
    lib = _lib.load()
    assert lib.bm_abi_version() == _lib.BM_ABI_VERSION == 7
    for name in CALLS:
        assert hasattr(lib, name), name
    names = {"Ledger", "LedgerRow", "LedgerResult", "BM_MAX_LEDGER_ROWS"}
    assert names <= set(pkg.__all__)
    assert all(getattr(pkg, n) is getattr(_lib, n) for n in names)
    assert _lib.BM_MAX_LEDGER_ROWS == 1 << 20


def test_struct_layouts_match_the_header():
    structs = {"bm_ledger_row_t": (_lib.LedgerRow, ROW_FIELDS), "bm_ledger_result_t": (_lib.LedgerResult, RESULT_FIELDS)}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "btcminer.h"', "int main(void) {"]
    for name, (_, fields) in structs.items():
        lines.append(f'printf("{name}.size %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['printf("abi %d\\n", BM_ABI_VERSION);', 'printf("max %u\\n", BM_MAX_LEDGER_ROWS);', "return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out if ln.strip()}
    assert got["abi"] == [7] and got["max"] == [1 << 20]
    assert got["bm_ledger_row_t.size"] == [ctypes.sizeof(_lib.LedgerRow)] == [64]
    assert got["bm_ledger_result_t.size"] == [ctypes.sizeof(_lib.LedgerResult)] == [88]
    for name, (mirror, fields) in structs.items():
        assert [f for f, _ in mirror._fields_] == fields
        for k, f in enumerate(fields):
            assert got[f"{name}.{f}"] == [getattr(mirror, f).offset] == [8 * k], (name, f)


# ---- the scenarios on the CPU entries ------------------------------------------------------

@pytest.mark.parametrize("n", jref.BATCH_SIZES)
def test_batch_sizes(n):
    lref.batch_sizes(Ledger.cpu, ShareSet.cpu, n)


@pytest.mark.parametrize("peel", lref.PEELS)
def test_wave_shapes(peel):
    """A CPU ledger accepts the peel setting and ignores it."""
    lref.wave_shapes(Ledger.cpu, ShareSet.cpu, peel)


@pytest.mark.parametrize("scenario", [lref.row_mapping, lref.every_class, lref.unknown_sessions, lref.best,
                                      lref.accumulation, lref.drain_and_clear, lref.refusals, lref.agreement],
                         ids=lambda f: f.__name__)
def test_cpu_ledger(scenario):
    scenario(Ledger.cpu, ShareSet.cpu)


def test_creation_refusals():
    lref.creation()
    for rows in (0, -1, _lib.BM_MAX_LEDGER_ROWS + 1, 1.5, True):
        with pytest.raises(ValueError):
            Ledger.cpu(rows)


# ---- the Python layer ------------------------------------------------------------------------

def test_python_layer():
    jobs, sessions = jref.open_jobs()
    subs = [(1, 2, 3, 4, 0, 0), (1, 2, 3, 4, 0, 0), (5, 6, 7, 8, 4, 1), (5, 6, 7, 8, 9, 1)]
    with Ledger.cpu(3) as ledger, ShareSet.cpu(8) as s:
        assert ledger.rows == 3
        v, r = ledger.verify_jobs(jobs, sessions, subs, share_set=s, accounts=[0, 1, 1, 1, 2], weights=[10, 1, 1, 1, 7])
        assert [x.status for x in v] == [1, 17, 1, 4]
        assert (r.n, r.shares, r.duplicates, r.recorded, r.count, r.credited, r.unattributed, r.work) == (4, 3, 1, 2, 2, 2, 1, 17)
        rows = ledger.read()
        assert [(x.accepted, x.duplicates, x.work, x.rejected) for x in rows] == [(1, 1, 10, 1), (0, 0, 0, 0), (1, 0, 7, 0)]
        assert rows[1].best == _lib.BM_LEDGER_NO_BEST and rows[0].best == v[0].value >> 192
        assert [x.as_tuple() for x in ledger.read(2)] == [rows[2].as_tuple()]
        assert [x.as_tuple() for x in ledger.drain(0, 1)] == [rows[0].as_tuple()]
        assert ledger.read(0, 1)[0].as_tuple() == lref.EMPTY
        v, r = ledger.verify_jobs(jobs, iter(sessions[:3]), subs[:1])  # no set, the identity, ones
        assert (r.credited, r.work, r.count) == (1, 1, 0) and ledger.read()[0].accepted == 1
        ledger.set_peel(0)
        ledger.set_peel(64)
        for bad in (65, -1, "4"):
            with pytest.raises((ValueError, BtcMinerError)):
                ledger.set_peel(bad)
        with pytest.raises(ValueError):
            ledger.verify_jobs(jobs, sessions, subs, accounts=[0, 1])
        with pytest.raises(ValueError):
            ledger.verify_jobs(jobs, sessions, subs, weights=[1] * 4 + [1 << 64])
        with pytest.raises(BtcMinerError) as e:
            ledger.verify_jobs(jobs, sessions, subs, accounts=[0, 1, 2, 3, 0])
        assert e.value.status == _lib.BM_EINVAL
        with pytest.raises(BtcMinerError):
            ledger.read(2, 2)
        ledger.clear()
        assert [x.as_tuple() for x in ledger.read()] == [lref.EMPTY] * 3
    with pytest.raises(ValueError):
        ledger.read()


# ---- the C++ wrapper ---------------------------------------------------------------------------

CPP = r"""
#include <cstdio>
#include <vector>
#include "btcminer.hpp"
int main() {
    btcminer::Job job;
    job.coinb1 = {1, 2, 3, 4}, job.coinb2 = {5, 6, 7, 8}, job.extranonce1 = {0, 0, 0, 0};
    job.extranonce2_size = 4, job.prevhash[0] = 1, job.nbits = 0x1d00ffff;
    const std::vector<btcminer::PoolJob> pj = {btcminer::PoolJob{&job, 0, 0xFFFFFFFFu}};
    std::vector<bm_pool_session_t> ses(2);
    for (auto& s : ses) for (auto& b : s.target) b = 0xFF;
    ses[1].extranonce1[0] = 9;
    std::vector<bm_jobs_submit_t> subs(3);
    subs[0].session = 0, subs[1].session = 1, subs[2].session = 1, subs[2].nonce = 5;
    const uint32_t accounts[2] = {1, 1};
    const uint64_t weights[2] = {5, 7};
    btcminer::Ledger ledger = btcminer::Ledger::cpu(2);
    btcminer::ShareSet set = btcminer::ShareSet::cpu(16);
    std::vector<bm_job_verdict_t> v;
    bm_ledger_result_t r = ledger.verify_jobs(&set, pj, ses, accounts, weights, subs.data(), subs.size(), v);
    std::vector<bm_ledger_row_t> rows = ledger.read(0, 2);
    std::printf("%llu %llu %llu %llu %llu %zu\n", (unsigned long long)r.credited, (unsigned long long)r.work,
                (unsigned long long)rows[1].accepted, (unsigned long long)rows[1].work, (unsigned long long)rows[0].accepted,
                v.size());
    r = ledger.verify_jobs(nullptr, pj, ses, nullptr, nullptr, subs.data(), 1, v);
    rows = ledger.drain(0, 1);
    std::printf("%llu %llu %llu\n", (unsigned long long)r.work, (unsigned long long)rows[0].accepted,
                (unsigned long long)ledger.read(0, 1)[0].accepted);
    ledger.set_peel(4);
    ledger.clear();
    std::printf("%llu %llu\n", (unsigned long long)ledger.rows(), (unsigned long long)ledger.read(1, 1)[0].accepted);
    try {
        ledger.read(1, 2);
    } catch (const btcminer::Error& e) {
        std::printf("refused %d\n", e.status());
    }
    return 0;
}
"""


def test_cpp_wrapper():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "ledger.cpp"), os.path.join(d, "ledger")
        with open(src, "w") as f:
            f.write(CPP)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                               "-L", libdir, "-lbtcminer", f"-Wl,-rpath,{libdir}", "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out == ["3 19 3 19 0 3", "1 1 0", "2 0", "refused -1"]
