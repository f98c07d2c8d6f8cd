"""The stratum_verify command line (no GPU): over a stand-in context that answers
with hashlib (tests/verify_ref.py), and with --cpu over bm_job_verify_cpu.  The
round trip of stratum_job's output for the README's genesis example, each reject
reason, the input forms and the argument errors."""
import collections
import io
import json
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT
from distributed_bitcoin_minter_amd import stratum_job, stratum_verify
import verify_ref as ref

JOB_PATH = os.path.join(GOLDEN, "stratum_genesis_job.json")
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
GENESIS_PARAMS = '["satoshi.1","genesis","001d","495fab29","7c2bac1d","00000000"]'
DIFF1 = 0xffff << 208
Verdict = collections.namedtuple("Verdict", "value status")


class _MinerContext:
    """stratum_job's side: search_job_shares finds the genesis share, as the README's example does."""

    def search_job_shares(self, job, versions, en2_lo, en2_hi, lo, hi, target, cap):
        assert (en2_lo, en2_hi, lo, hi) == (29, 29, 2083236608, 2083237119) and versions == [1]
        share = {"hash": GENESIS_HASH, "extranonce2": 29, "extranonce2_size": 2, "ntime": job.ntime,
                 "nonce": 2083236893, "version_index": 0, "version": 1, "is_block": True}
        return 1, [share], (GENESIS_HASH, 29, 2083236893, 0)


class _PoolContext:
    """stratum_verify's side: verify_submits by hashlib."""

    def __init__(self):
        self.calls = []

    def verify_submits(self, job, submits, target):
        subs = [(s["extranonce2"], s["ntime"], s["nonce"], s["version"]) for s in submits]
        self.calls.append((subs, target))
        return [Verdict(*ref.verdict(job, target, s)) for s in subs], None


def run(text, *flags, ctx=None):
    out = io.StringIO()
    rc = stratum_verify.main([JOB_PATH, "-", *flags], out=out, ctx=ctx, stdin=io.StringIO(text))
    return rc, out.getvalue().splitlines()


def test_round_trip_of_the_readme_example():
    mined = io.StringIO()
    argv = [JOB_PATH, "--versions", "1", "--extranonce2", "29", "29", "2083236608", "2083237119"]
    assert stratum_job.main(argv, out=mined, ctx=_MinerContext()) == 0
    assert mined.getvalue().splitlines() == ["Block %s %064x" % (GENESIS_PARAMS, GENESIS_HASH),
                                             "Shares 1 Best %064x 001d 2083236893 00000001" % GENESIS_HASH]
    want = ["Block %s %064x" % (GENESIS_PARAMS, GENESIS_HASH), "Verified 1 Accepted 1 Blocks 1 Rejected 0"]
    pool = _PoolContext()
    assert run(mined.getvalue(), ctx=pool) == (0, want)
    assert pool.calls == [([(29, 0x495fab29, 2083236893, 1)], DIFF1)]  # one batch, at the difficulty's target
    assert run(mined.getvalue(), "--cpu") == (0, want)                  # the library's CPU entry agrees
    # its own Block line verifies again
    assert run(want[0] + "\n", "--cpu") == (0, want)


def test_every_verdict_and_reject_reason():
    good = json.loads(GENESIS_PARAMS)

    def with_(i, v):
        return json.dumps(good[:i] + [v] + good[i + 1:], separators=(",", ":"))

    above = with_(4, "7c2bac1e")           # the next nonce: a hash above the target
    rolled = with_(5, "00002000")          # inside the mask, another header
    lines = [
        GENESIS_PARAMS,                    # a bare array
        "Submit " + GENESIS_PARAMS + " 00ff",   # the keyword and the trailing hash are ignored
        "  Block   " + GENESIS_PARAMS,
        json.dumps(good[:5]),              # five params: the job's own version (JSON's default spacing)
        above,
        rolled,
        with_(2, "1d"),
        with_(2, "001g"),
        with_(5, "00000001"),
        with_(1, "other"),
        with_(3, "495fab2"),
        json.dumps(good[:4]),
        '{"a":1}',
        "[1,2",
        "hello",
        "",
        "Shares 3 Best 00 001d 5 00000001",
    ]
    block = "Block %s %064x" % (GENESIS_PARAMS, GENESIS_HASH)
    want = [
        block, block, block,
        "Block %s %064x" % (json.dumps(good[:5], separators=(",", ":")), GENESIS_HASH),
        "Reject above-target " + above,
        "Reject above-target " + rolled,
        "Reject extranonce2 " + with_(2, "1d"),
        "Reject extranonce2 " + with_(2, "001g"),
        "Reject version-bits " + with_(5, "00000001"),
        "Reject job-id " + with_(1, "other"),
        "Reject malformed " + with_(3, "495fab2"),
        "Reject malformed " + json.dumps(good[:4], separators=(",", ":")),
        'Reject malformed {"a":1}',
        "Reject malformed [1,2",
        "Reject malformed hello",
        "Verified 15 Accepted 4 Blocks 4 Rejected 11",
    ]
    pool = _PoolContext()
    assert run("\n".join(lines) + "\n", ctx=pool) == (0, want)
    assert len(pool.calls) == 1 and len(pool.calls[0][0]) == 6  # only what parses is hashed, in one batch
    assert run("\n".join(lines) + "\n", "--cpu") == (0, want)
    assert run("", "--cpu") == (0, ["Verified 0 Accepted 0 Blocks 0 Rejected 0"])


def test_accept_without_block(tmp_path):
    """A share that meets the difficulty but not nbits prints Accept; the job file's mask is the one applied."""
    with open(JOB_PATH) as f:
        obj = json.load(f)
    obj["difficulty"] = 2.0 ** -40          # every hash is a share
    obj["version_mask"] = "00002000"
    path = tmp_path / "job.json"
    path.write_text(json.dumps(obj))
    good = json.loads(GENESIS_PARAMS)
    other = json.dumps(good[:4] + ["00000005", "00002000"], separators=(",", ":"))
    outside = json.dumps(good[:4] + ["00000005", "00004000"], separators=(",", ":"))
    job = stratum_job.load_job(obj)[0]
    h, status = ref.verdict(job, ref.U256, (29, 0x495fab29, 5, 0x2001))
    assert status == 1
    out = io.StringIO()
    src = tmp_path / "subs.txt"
    src.write_text(other + "\n" + outside + "\n")
    assert stratum_verify.main([str(path), str(src), "--cpu"], out=out) == 0
    assert out.getvalue().splitlines() == ["Accept %s %064x" % (other, h), "Reject version-bits " + outside,
                                           "Verified 2 Accepted 1 Blocks 0 Rejected 1"]


def test_argument_errors_exit_2(tmp_path):
    assert stratum_verify.main([]) == 2
    assert stratum_verify.main([JOB_PATH + ".missing", "-", "--cpu"], stdin=io.StringIO("")) == 2
    assert stratum_verify.main([JOB_PATH, str(tmp_path / "missing.txt"), "--cpu"]) == 2
    assert stratum_verify.main([JOB_PATH, "-", "--gpu"]) == 2
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.stratum_verify", JOB_PATH, "--cpu"],
                       input="Block %s\n" % GENESIS_PARAMS, capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Verified 1 Accepted 1 Blocks 1 Rejected 0", r.stderr
