"""The stratum_job command line over a stand-in context (no GPU): the job file,
the argument checks, the Submit / Block / Shares lines, and the halving of an
over-full piece, extranonce2 range first, then the nonce range."""
import io
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from distributed_bitcoin_minter_amd import _lib, stratum_job

JOB_PATH = os.path.join(GOLDEN, "stratum_genesis_job.json")
GENESIS_HASH = 0x000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f
U32 = (1 << 32) - 1
U256 = (1 << 256) - 1


class _FakeContext:
    """search_job_shares over a fixed set of (hash, extranonce2, nonce, index)
    shares, all or nothing; a share is a block at or below the job's nbits."""

    def __init__(self, shares, block_target=_lib.DIFF1_TARGET):
        self.shares, self.calls = sorted(shares, key=lambda s: s[1:]), []
        self.block_target = block_target

    def search_job_shares(self, job, versions, en2_lo, en2_hi, lo, hi, target, cap):
        self.calls.append((en2_lo, en2_hi, lo, hi))
        assert en2_hi - en2_lo < _lib.BM_MAX_JOB_HEADERS
        got = [s for s in self.shares if en2_lo <= s[1] <= en2_hi and lo <= s[2] <= hi and s[0] <= target]
        best = min(got, key=lambda s: (s[0] >> 192,) + s[1:]) if got else (U256 - 1, en2_lo, lo, 0)
        out = [{"hash": h, "extranonce2": e, "extranonce2_size": job.extranonce2_size, "ntime": job.ntime, "nonce": n,
                "version_index": i, "version": versions[i], "is_block": h <= self.block_target} for h, e, n, i in got]
        return len(got), (out if len(got) <= cap else None), best


def _job():
    return stratum_job.parse_args([JOB_PATH])[0]


def test_parse_args():
    job, versions, mask, worker, target, en2_lo, en2_hi, lower, upper, cap = stratum_job.parse_args([JOB_PATH])
    assert (job.job_id, job.extranonce2_size, job.version, job.nbits, job.ntime) == ("genesis", 2, 1, 0x1d00ffff,
                                                                                     0x495fab29)
    assert versions == [1, 0x2001, 0x4001, 0x6001] and mask == 0x1fffe000 and worker == "satoshi.1"
    assert target == 0xffff << 208 and (en2_lo, en2_hi, lower, upper, cap) == (0, 0, 0, U32, 65536)
    got = stratum_job.parse_args([JOB_PATH, "--versions", "2", "--extranonce2", "28", "0x1e", "--cap", "2", "5", "77"])
    assert got[1] == [1, 0x2001] and got[5:] == (28, 30, 5, 77, 2)
    bad = [
        [],
        [JOB_PATH + ".missing"],
        [JOB_PATH, "--versions", "0"],
        [JOB_PATH, "--versions", "65"],
        [JOB_PATH, "--versions", "two"],
        [JOB_PATH, "--extranonce2", "0"],
        [JOB_PATH, "--extranonce2", "0", "65536"],       # past the 2-byte field
        [JOB_PATH, "--extranonce2", "-1", "5"],
        [JOB_PATH, "--extranonce2", "0", "1g"],
        [JOB_PATH, "--cap", "0"],
        [JOB_PATH, "--cap", str((1 << 20) + 1)],
        [JOB_PATH, "--cap", "3"],                        # below the 4 default versions
        [JOB_PATH, "-1"],
        [JOB_PATH, "0", "4294967296"],
    ]
    for argv in bad:
        with pytest.raises((ValueError, SystemExit)):
            stratum_job.parse_args(argv)
        assert stratum_job.main(argv) == 2, argv


def test_job_file_checks(tmp_path):
    with open(JOB_PATH) as f:
        good = json.load(f)

    def run(obj):
        p = tmp_path / "job.json"
        p.write_text(obj if isinstance(obj, str) else json.dumps(obj))
        return stratum_job.parse_args([str(p)])

    assert run(good)[4] == 0xffff << 208
    no_mask = {k: v for k, v in good.items() if k not in ("version_mask", "worker")}
    got = run(no_mask)
    assert got[1] == [1] and got[2] is None and got[3] == ""
    with pytest.raises(ValueError):
        p = tmp_path / "job.json"
        p.write_text(json.dumps(no_mask))
        stratum_job.parse_args([str(p), "--versions", "2"])
    assert run(dict(good, difficulty=0.5))[4] == 0xffff << 209
    for bad in ("{", "[1]", {k: v for k, v in good.items() if k != "notify"},
                {k: v for k, v in good.items() if k != "difficulty"}, dict(good, difficulty=0), dict(good, difficulty="1"),
                dict(good, extranonce2_size=0), dict(good, extranonce2_size=9), dict(good, extranonce1="f"),
                dict(good, notify=good["notify"][:8]), dict(good, notify="x"), dict(good, version_mask="xyz"),
                dict(good, version_mask="100000000"), dict(good, version_mask="2000"),  # holds 2 versions, 4 asked for
                dict(good, worker=5)):
        with pytest.raises(ValueError):
            run(bad)


def test_enumerate_halves_extranonce2_then_nonces():
    job = _job()
    vs = [1, 0x2001]
    shares = [(5 << 200, 28, 7, 0), (4 << 200, 28, 7, 1), (6 << 200, 28, 900, 0), (3 << 200, 29, 100, 1),
              (9 << 200, 30, 4000, 0), (2 << 200, 30, 4001, 1), (2 << 200, 31, 5, 0)]
    ctx = _FakeContext(shares)
    got, best = stratum_job.enumerate_shares(ctx, job, vs, 1 << 255, 28, 31, 0, 4095, cap=2)
    assert [(s["hash"], s["extranonce2"], s["nonce"], s["version_index"]) for s in got] == ctx.shares
    assert best == (2 << 200, 30, 4001, 1)  # the earlier extranonce2 of the two equal hashes
    assert ctx.calls[0] == (28, 31, 0, 4095) and ctx.calls[1] == (28, 29, 0, 4095) and ctx.calls[2] == (28, 28, 0, 4095)
    assert ctx.calls[3] == (28, 28, 0, 2047)  # one extranonce2 left: the nonce range is halved
    assert all(a <= b and c <= d for a, b, c, d in ctx.calls)
    # two shares at one nonce fit a cap of 2 (the number of versions): the halving ends
    assert sum(1 for c in ctx.calls if c[:2] == (28, 28)) > 2
    # empty ranges scan nothing
    assert stratum_job.enumerate_shares(ctx, job, vs, 0, 5, 4, 0, 10) == ([], (U256, 5, U32, 0))
    assert stratum_job.enumerate_shares(ctx, job, vs, 0, 4, 5, 10, 0) == ([], (U256, 4, U32, 0))
    # more extranonce2 values than one library call takes: pieces of 4096
    ctx = _FakeContext([(1 << 200, 5000, 3, 0), (7 << 200, 2, 3, 1)])
    got, best = stratum_job.enumerate_shares(ctx, job, vs, 1 << 255, 0, 9999, 0, 10)
    assert ctx.calls == [(0, 4095, 0, 10), (4096, 8191, 0, 10), (8192, 9999, 0, 10)]
    assert [s["extranonce2"] for s in got] == [2, 5000] and best == (1 << 200, 5000, 3, 0)
    # a single (extranonce2, nonce) that still does not fit is an error, not a loop
    ctx = _FakeContext([(1, 1, 1, 0), (2, 1, 1, 1)])
    with pytest.raises(RuntimeError):
        stratum_job.enumerate_shares(ctx, job, vs, 1 << 255, 1, 1, 1, 1, cap=1)


def test_main_prints_submit_block_and_shares():
    # the genesis block itself, a plain share just below the difficulty-1 target and a hash above it
    # (the stand-in calls only the genesis hash a block, so that both kinds of line show)
    shares = [(GENESIS_HASH, 29, 2083236893, 0), ((0xffff << 208) - 5, 29, 17, 2), ((1 << 224) - 1, 30, 99, 3)]
    ctx = _FakeContext(shares, GENESIS_HASH)
    out = io.StringIO()
    argv = [JOB_PATH, "--extranonce2", "28", "30", "--cap", "4"]
    assert stratum_job.main(argv, out=out, ctx=ctx) == 0
    lines = out.getvalue().splitlines()
    assert lines == [
        'Submit ["satoshi.1","genesis","001d","495fab29","00000011","00004000"] %064x' % ((0xffff << 208) - 5),
        'Block ["satoshi.1","genesis","001d","495fab29","7c2bac1d","00000000"] %064x' % GENESIS_HASH,
        "Shares 2 Best %064x 001d 2083236893 00000001" % GENESIS_HASH,
    ]  # the third hash is above the difficulty-1 target
    assert ctx.calls == [(28, 30, 0, U32)]
    for ln in lines[:2]:
        word, params, h = ln.split(" ")
        assert json.loads(params)[0] == "satoshi.1" and len(h) == 64
    # the defaults spelled out give the same output
    out2 = io.StringIO()
    assert stratum_job.main([JOB_PATH, "--extranonce2", "28", "30", "--versions", "4", "--cap", "4", "0", str(U32)],
                            out=out2, ctx=_FakeContext(shares, GENESIS_HASH)) == 0
    assert out2.getvalue() == out.getvalue()
    # six shares against a cap of 4: the halving path through main
    halved = _FakeContext(shares + [((0xffff << 208) - k, 29, 20 + k, 1) for k in range(4)], GENESIS_HASH)
    out3 = io.StringIO()
    assert stratum_job.main(argv, out=out3, ctx=halved) == 0
    got = out3.getvalue().splitlines()
    assert len(halved.calls) > 1 and got[-1].startswith("Shares 6 Best %064x 001d 2083236893" % GENESIS_HASH)
    assert [ln.split(" ")[0] for ln in got] == ["Submit"] * 5 + ["Block", "Shares"]
    nonces = [int(json.loads(ln.split(" ")[1])[4], 16) for ln in got[:-1]]
    assert nonces == sorted(nonces) == [17, 20, 21, 22, 23, 2083236893]
    # nothing found: the empty answer
    out4 = io.StringIO()
    assert stratum_job.main([JOB_PATH, "5", "4"], out=out4, ctx=_FakeContext([])) == 0
    assert out4.getvalue() == "Shares 0 Best %064x 0000 %d 00000001\n" % (U256, U32)


def test_cli_argument_errors_exit_2():
    r = subprocess.run([sys.executable, "-m", "distributed_bitcoin_minter_amd.stratum_job", JOB_PATH, "--versions", "8",
                        "--cap", "7"], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 2 and "--cap" in r.stderr and r.stdout == ""
