"""The pool_ledger command line: the two live jobs of the pool_jobs fixtures, and
sessions, submissions and expected lines written by
tests/golden/make_ledger_golden.py with hashlib only; on --cpu, and on the GPU under
the gpu mark."""
import io
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_golden
from distributed_bitcoin_minter_amd import pool_ledger

SESSIONS = os.path.join(GOLDEN, "stratum_ledger_sessions.json")
SUBMITS = os.path.join(GOLDEN, "stratum_ledger_submits.txt")
JOBS = [os.path.join(GOLDEN, "stratum_genesis_job.json"), os.path.join(GOLDEN, "stratum_second_job.json")]
EXPECTED = load_golden("stratum_ledger_expected.json")


def run(*flags, text=None, jobs=JOBS, ctx=None):
    out = io.StringIO()
    argv = [SESSIONS, SUBMITS if text is None else "-", *jobs, *flags]
    rc = pool_ledger.main(argv if ctx is not None else argv + ["--cpu"], out=out, ctx=ctx,
                          stdin=None if text is None else io.StringIO(text))
    return rc, out.getvalue().splitlines()


def scenarios(ctx=None):
    assert run(ctx=ctx) == (0, EXPECTED["plain"])
    assert run("--batch", "1", ctx=ctx) == (0, EXPECTED["plain"])
    for flags in ((), ("--batch", "1"), ("--batch", "4", "--capacity", "6")):
        assert run("--dedup", *flags, ctx=ctx) == (0, EXPECTED["dedup"]), flags
    assert run("--dedup", "--by-worker", "--batch", "3", ctx=ctx) == (0, EXPECTED["dedup_by_worker"])
    assert run("--dedup", "--ntime-slack", "60", ctx=ctx) == (0, EXPECTED["slack60"])
    assert run(jobs=JOBS[::-1], ctx=ctx) == (0, EXPECTED["plain"])


def test_fixtures_are_what_the_generator_writes(tmp_path):
    """The committed fixtures are make_ledger_golden.py's output, byte for byte, and
    hold what the cases need."""
    names = ("stratum_ledger_sessions.json", "stratum_ledger_submits.txt", "stratum_ledger_expected.json")
    work = tmp_path / "golden"
    work.mkdir()
    for name in ("make_ledger_golden.py", "make_jobs_golden.py", "stratum_genesis_job.json", "stratum_second_job.json"):
        (work / name).write_bytes(open(os.path.join(GOLDEN, name), "rb").read())
    subprocess.check_call([sys.executable, str(work / "make_ledger_golden.py")], timeout=120)
    for name in names:
        assert (work / name).read_bytes() == open(os.path.join(GOLDEN, name), "rb").read(), name
    dedup = EXPECTED["dedup"]
    kinds = [ln.split()[0] + " " + ln.split()[1] for ln in dedup if ln.startswith("Reject")]
    assert {"Reject duplicate", "Reject above-target", "Reject job", "Reject malformed"} <= set(kinds)
    accounts = [ln.split() for ln in dedup if ln.startswith("Account")]
    assert [a[1] for a in accounts] == ["farm", "satoshi", "solo"]
    farm = dict(zip(accounts[0][2::2], accounts[0][3::2]))
    # farm.1 at 2^-20 twice and farm.2 at 2^-18 once: a per-submission sum, not weight x count
    assert farm["Accepted"] == "3" and farm["Work"] == str(2 * 4096 + 16384) and farm["Duplicate"] == "2"
    assert farm["AboveTarget"] == "1" and farm["Rejected"] == "3"
    satoshi = dict(zip(accounts[1][2::2], accounts[1][3::2]))
    assert satoshi["Blocks"] == "1" and satoshi["Work"] == str(1 << 32) and satoshi["Best"] == "000000000019d668"


def test_cli_on_the_cpu():
    scenarios()


def test_account_lines():
    """--by-worker splits the shared account; the plain run pays the repeats."""
    plain = [ln for ln in EXPECTED["plain"] if ln.startswith("Account")]
    split = [ln for ln in run("--dedup", "--by-worker")[1] if ln.startswith("Account")]
    assert [ln.split()[1] for ln in split] == ["farm.1", "farm.2", "satoshi.1", "solo.1"]
    assert [ln.split()[3] for ln in split] == ["2", "1", "1", "2"]
    assert [ln.split()[17] for ln in split] == [str(2 * 4096), str(16384), str(1 << 32), str(2 * 4096)]
    assert plain[0].split()[1:4] == ["farm", "Accepted", "5"] and plain[0].split()[16:18] == ["Work", str(3 * 4096 + 2 * 16384)]
    assert run(text="") == (0, ["Verified 0 Accepted 0 Blocks 0 Rejected 0"] +
                            ["Account %s Accepted 0 Blocks 0 Rejected 0 AboveTarget 0 Ntime 0 Duplicate 0 Extranonce2 0 Work 0 Best -" % a
                             for a in ("farm", "satoshi", "solo")])
    # an extranonce2 of the wrong size is rejected before hashing and belongs to no account
    bad = '["solo.1","second","010000","495fab47","00000000","00000000"]'
    got = run(text=bad + "\n")[1]
    assert got[0] == "Reject extranonce2 " + bad and got[-1].split()[14:16] == ["Extranonce2", "0"]


def test_cli_errors(capsys):
    assert pool_ledger.main([]) == 2 and pool_ledger.main([SESSIONS, SUBMITS]) == 2
    assert run("--capacity", "4")[0] == 2                      # goes with --dedup
    for flags in (("--dedup", "--capacity", "0"), ("--batch", "0"), ("--ntime-slack", "-1")):
        assert run(*flags)[0] == 2, flags
    assert run(jobs=[JOBS[0] + ".missing"])[0] == 2
    capsys.readouterr()
    # a set too small for the six distinct accepted hashes: status 3, a message, nothing printed
    for flags in (("--capacity", "5"), ("--capacity", "5", "--batch", "1")):
        assert run("--dedup", *flags) == (3, [])
        assert "full" in capsys.readouterr().err


def test_cli_as_a_module():
    cmd = [sys.executable, "-m", "distributed_bitcoin_minter_amd.pool_ledger", SESSIONS, SUBMITS, *JOBS, "--cpu", "--dedup"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.splitlines() == EXPECTED["dedup"], r.stderr


@pytest.mark.gpu
def test_cli_on_the_gpu(gpu_ctx):
    scenarios(gpu_ctx)
