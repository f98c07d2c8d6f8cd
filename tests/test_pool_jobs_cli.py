"""The pool_jobs command line: two live jobs (the genesis job and
tests/golden/stratum_second_job.json), submissions and expected lines written by
tests/golden/make_jobs_golden.py with hashlib only; on --cpu, and on the GPU under
the gpu mark."""
import io
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_golden
from distributed_bitcoin_minter_amd import pool_jobs

SESSIONS = os.path.join(GOLDEN, "stratum_jobs_sessions.json")
SUBMITS = os.path.join(GOLDEN, "stratum_jobs_submits.txt")
JOBS = [os.path.join(GOLDEN, "stratum_genesis_job.json"), os.path.join(GOLDEN, "stratum_second_job.json")]
EXPECTED = load_golden("stratum_jobs_expected.json")


def run(*flags, text=None, jobs=JOBS, sessions=SESSIONS, ctx=None):
    out = io.StringIO()
    argv = [sessions, SUBMITS if text is None else "-", *jobs, *flags]
    rc = pool_jobs.main(argv if ctx is not None else argv + ["--cpu"], out=out, ctx=ctx,
                        stdin=None if text is None else io.StringIO(text))
    return rc, out.getvalue().splitlines()


def scenarios(ctx=None):
    assert run(ctx=ctx) == (0, EXPECTED["plain"])
    assert run("--batch", "1", ctx=ctx) == (0, EXPECTED["plain"])
    assert run("--batch", "3", ctx=ctx) == (0, EXPECTED["plain"])
    assert run("--ntime-slack", "60", ctx=ctx) == (0, EXPECTED["slack60"])
    assert run("--ntime-slack", "0x64", ctx=ctx) == (0, EXPECTED["plain"])
    for flags in ((), ("--batch", "1"), ("--batch", "3", "--capacity", "4")):
        assert run("--dedup", *flags, ctx=ctx) == (0, EXPECTED["dedup"]), flags
    # the job files' order does not matter: the id picks the job
    assert run(jobs=JOBS[::-1], ctx=ctx) == (0, EXPECTED["plain"])
    # one job file: the other job's submissions are `Reject job`
    got = run(jobs=JOBS[:1], ctx=ctx)[1]
    assert [ln.split()[0:2] for ln in got[:3]] == [["Reject", "job"], ["Block", EXPECTED["plain"][1].split()[1]], ["Reject", "job"]]
    assert got[-1] == "Verified 8 Accepted 2 Blocks 2 Rejected 6"


def test_fixtures_are_what_the_generator_writes(tmp_path):
    """The committed fixtures are make_jobs_golden.py's output, byte for byte."""
    names = ("stratum_second_job.json", "stratum_jobs_sessions.json", "stratum_jobs_submits.txt", "stratum_jobs_expected.json")
    work = tmp_path / "golden"
    work.mkdir()
    for name in ("make_jobs_golden.py", "stratum_genesis_job.json", "stratum_genesis_sessions.json"):
        (work / name).write_bytes(open(os.path.join(GOLDEN, name), "rb").read())
    subprocess.check_call([sys.executable, str(work / "make_jobs_golden.py")], timeout=120)
    for name in names:
        assert (work / name).read_bytes() == open(os.path.join(GOLDEN, name), "rb").read(), name
    second = load_golden("stratum_second_job.json")
    assert second["notify"][0] == "second" and len(second["notify"][4]) == 1
    assert sum(ln.startswith("Accept") for ln in EXPECTED["plain"]) == 4
    assert all(ln.split()[-1].startswith("000") for ln in EXPECTED["plain"] if ln.startswith("Accept"))  # 12 zero bits


def test_cli_on_the_cpu():
    scenarios()


def test_cli_reasons(tmp_path):
    lines = open(SUBMITS).read().splitlines()
    good = json.loads(lines[0])

    def with_(i, v):
        return json.dumps(good[:i] + [v] + good[i + 1:], separators=(",", ":"))

    text = "\n".join([with_(0, "nobody"), with_(2, "00"), with_(5, "00000001"), "hello", "", with_(1, 5), lines[0],
                      "Shares 1 Best 00 001d 5 00000001", "Accept " + lines[2] + " 00"]) + "\n"
    want = ["Reject worker " + with_(0, "nobody"), "Reject extranonce2 " + with_(2, "00"),
            "Reject version-bits " + with_(5, "00000001"), "Reject malformed hello", "Reject job " + with_(1, 5),
            EXPECTED["plain"][0], EXPECTED["plain"][2], "Verified 7 Accepted 2 Blocks 0 Rejected 5"]
    assert run(text=text) == (0, want)
    assert run("--dedup", text=text) == (0, want[:-1] + [want[-1] + " Duplicates 0"])
    assert run(text="") == (0, ["Verified 0 Accepted 0 Blocks 0 Rejected 0"])
    assert run("--dedup", text="") == (0, ["Verified 0 Accepted 0 Blocks 0 Rejected 0 Duplicates 0"])


def test_cli_errors(tmp_path, capsys):
    assert pool_jobs.main([]) == 2 and pool_jobs.main([SESSIONS, SUBMITS]) == 2
    assert run("--capacity", "4")[0] == 2                      # goes with --dedup
    for flags in (("--dedup", "--capacity", "0"), ("--batch", "0"), ("--batch", "x"), ("--ntime-slack", "-1"),
                  ("--ntime-slack", str(1 << 32)), ("--dedup", "--capacity", str((1 << 24) + 1))):
        assert run(*flags)[0] == 2, flags
    assert run(jobs=[JOBS[0] + ".missing"])[0] == 2
    assert run(jobs=JOBS + JOBS[:1])[0] == 2                   # a repeated id
    assert run(jobs=JOBS[:1] * 65)[0] == 2
    assert run(sessions=SESSIONS + ".missing")[0] == 2
    assert pool_jobs.main([SESSIONS, str(tmp_path / "missing.txt"), *JOBS, "--cpu"]) == 2
    other = dict(load_golden("stratum_second_job.json"), extranonce1="ffffff")
    path = tmp_path / "other.json"
    path.write_text(json.dumps(other))
    assert run(jobs=[JOBS[0], str(path)])[0] == 2              # another extranonce1 size
    # a set too small for the four distinct accepted hashes: status 3, a message, nothing printed
    capsys.readouterr()
    for flags in (("--capacity", "3"), ("--capacity", "3", "--batch", "1")):
        assert run("--dedup", *flags) == (3, [])
        assert "full" in capsys.readouterr().err


def test_cli_as_a_module_prints_what_the_readme_says():
    lines = open(SUBMITS).read().splitlines()
    cmd = [sys.executable, "-m", "distributed_bitcoin_minter_amd.pool_jobs", SESSIONS, "-", *JOBS, "--cpu"]
    r = subprocess.run(cmd, input=lines[1] + "\n" + lines[0] + "\n", capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.splitlines() == EXPECTED["readme"], r.stderr


@pytest.mark.gpu
def test_cli_on_the_gpu(gpu_ctx):
    scenarios(gpu_ctx)
