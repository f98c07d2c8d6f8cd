"""The pool_vardiff command line: the pool_ledger fixtures' jobs and workers, and
submissions with time marks and expected lines written by
tests/golden/make_vardiff_golden.py (hashlib for the submissions, the CPU table for
the lines); here the lines are checked against the pure-Python model of
tests/sessions_ref.py; on --cpu, and on the GPU under the gpu mark."""
import io
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_golden
from distributed_bitcoin_minter_amd import pool_jobs, pool_ledger, pool_vardiff
from distributed_bitcoin_minter_amd.pool_verify import _load_json, load_sessions
import ledger_ref as lref
import sessions_ref as sref

SESSIONS = os.path.join(GOLDEN, "stratum_ledger_sessions.json")
SUBMITS = os.path.join(GOLDEN, "stratum_vardiff_submits.txt")
JOBS = [os.path.join(GOLDEN, "stratum_genesis_job.json"), os.path.join(GOLDEN, "stratum_second_job.json")]
EXPECTED = load_golden("stratum_vardiff_expected.json")
FLAGS = EXPECTED["flags"]


def run(*flags, text=None, jobs=JOBS, ctx=None):
    out = io.StringIO()
    argv = [SESSIONS, SUBMITS if text is None else "-", *jobs, *flags]
    rc = pool_vardiff.main(argv if ctx is not None else argv + ["--cpu"], out=out, ctx=ctx,
                           stdin=None if text is None else io.StringIO(text))
    return rc, out.getvalue().splitlines()


def scenarios(ctx=None):
    assert run(*FLAGS, ctx=ctx) == (0, EXPECTED["plain"])
    assert run(*FLAGS, "--batch", "3", ctx=ctx) == (0, EXPECTED["plain"])
    for flags in ((), ("--batch", "1"), ("--capacity", "24")):
        assert run(*FLAGS, "--dedup", *flags, ctx=ctx) == (0, EXPECTED["dedup"]), flags


def test_fixtures_are_what_the_generator_writes(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, "make_vardiff_golden.py"), str(tmp_path)], timeout=120,
                          env=dict(os.environ, PYTHONPATH=ROOT))
    for name in ("stratum_vardiff_submits.txt", "stratum_vardiff_expected.json"):
        assert (tmp_path / name).read_bytes() == open(os.path.join(GOLDEN, name), "rb").read(), name


@pytest.mark.parametrize("dedup", (False, True), ids=("plain", "dedup"))
def test_expected_lines_against_the_model(dedup):
    """The verdict lines, the SetDifficulty lines, the accounts and the workers' final
    difficulties, from hashlib, a Python set, a dict of rows and the rule in big integers."""
    jobs, by_id, masks, size = pool_jobs.load_jobs(JOBS, None)
    obj = _load_json(SESSIONS)
    sessions, index = load_sessions(obj, size)
    names, accounts, weights = pool_ledger.account_map(obj["workers"], index, False)
    workers = sorted(index, key=index.get)
    policy = dict(sref.POLICY, target_ms=1000, window_ms=5000, band_permille=100)
    model, ledger = sref.Model(len(sessions)), lref.Model(len(names), 64 if dedup else None)
    model.set([(s.extranonce1, w, a) for s, w, a in zip(sessions, weights, accounts)], 0)
    with open(SUBMITS) as f:
        pieces = pool_vardiff.split_at_marks(f.read().splitlines())
    assert [ms for _, ms in pieces] == [6000, 12000, None]
    want, totals = [], [0] * 5

    def verify(subs):
        tuples = [tuple(s[k] for k in ("extranonce2", "ntime", "nonce", "version", "session", "job")) for s in subs]
        verdicts, _ = model.verify(jobs, tuples, ledger, ledger.set)

        class V:
            def __init__(self, value, status):
                self.value, self.status = value, status
        return [V(h, st) for h, st in verdicts], None

    for held, ms in pieces:
        text, counts = pool_jobs.jobs_lines(held, by_id, masks, index, verify, dedup=dedup)
        want += text
        totals = [x + y for x, y in zip(totals, counts)]
        if ms is not None:
            changes, _ = model.retarget(ms, policy, len(sessions))
            want += ["SetDifficulty %s %d/4294967296" % (workers[s], new) for s, _, new, _ in changes]
    closing = "Verified %d Accepted %d Blocks %d Rejected %d" % tuple(totals[:4])
    want.append(closing + (" Duplicates %d" % totals[4] if dedup else ""))
    rows = [type("Row", (), dict(zip(("accepted", "blocks", "above_target", "ntime", "duplicates", "invalid", "work", "best"), r),
                                 rejected=sum(r[2:6])))() for r in ledger.table()]
    want += [pool_ledger.account_line(name, row) for name, row in zip(names, rows)]
    want += ["Worker %s Difficulty %d/4294967296 Retargets %d" % (w, st[0], st[3]) for w, st in zip(workers, model.states)]
    assert EXPECTED["dedup" if dedup else "plain"] == want
    # what the fixture is there to show
    assert "SetDifficulty farm.1 8192/4294967296" in want and sum(ln.startswith("Reject above-target") for ln in want) == 2
    assert ("Reject duplicate" in " ".join(want)) == dedup


def test_cli_on_the_cpu():
    scenarios()


def test_time_marks_and_defaults():
    # no marks: pool_ledger's lines, then the workers at their starting difficulties
    with open(SUBMITS) as f:
        plain = "".join(ln for ln in f if not ln.startswith("@"))
    rc, got = run(text=plain)
    assert rc == 0 and not any(ln.startswith("SetDifficulty") for ln in got)
    assert got[-4:] == ["Worker satoshi.1 Difficulty 4294967296/4294967296 Retargets 0",
                        "Worker farm.1 Difficulty 4096/4294967296 Retargets 0",
                        "Worker farm.2 Difficulty 16384/4294967296 Retargets 0",
                        "Worker solo.1 Difficulty 4096/4294967296 Retargets 0"]
    # the default window is 60 s: a mark at 59999 changes nothing, one at 60000 quarters the idle workers
    assert not any(ln.startswith("SetDifficulty") for ln in run(text="@59999\n")[1])
    assert run(text="@60000\n")[1][:4] == ["SetDifficulty satoshi.1 1073741824/4294967296", "SetDifficulty farm.1 1024/4294967296",
                                          "SetDifficulty farm.2 4096/4294967296", "SetDifficulty solo.1 1024/4294967296"]
    assert run("--start-ms", "1", text="@60000\n")[1][0].startswith("Verified 0")
    assert run("--min-fx", "2048", "--max-down", "2", text="@60000\n")[1][1] == "SetDifficulty farm.1 2048/4294967296"


def test_cli_errors(capsys):
    assert pool_vardiff.main([]) == 2 and pool_vardiff.main([SESSIONS, SUBMITS]) == 2
    for flags in (("--capacity", "4"), ("--target-ms", "0"), ("--target-ms", str(1 << 32)), ("--max-up", "0"), ("--max-down", "0"),
                  ("--band-permille", "1001"), ("--min-fx", "0"), ("--min-fx", "9", "--max-fx", "8"), ("--batch", "0")):
        assert run(*flags)[0] == 2, flags
    for mark in ("@", "@12x", "@-5", "@" + str(1 << 64)):
        assert run(text=mark + "\n")[0] == 2, mark
    capsys.readouterr()
    assert run(*FLAGS, "--dedup", "--capacity", "23") == (3, [])  # 24 distinct accepted hashes
    assert "full" in capsys.readouterr().err


def test_cli_as_a_module():
    cmd = [sys.executable, "-m", "distributed_bitcoin_minter_amd.pool_vardiff", SESSIONS, SUBMITS, *JOBS, "--cpu", "--dedup", *FLAGS]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.splitlines() == EXPECTED["dedup"], r.stderr


@pytest.mark.gpu
def test_cli_on_the_gpu(gpu_ctx):
    scenarios(gpu_ctx)
