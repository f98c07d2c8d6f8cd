#!/usr/bin/env python3
"""Writes the fixtures of the pool_vardiff command line (tests/test_pool_vardiff_cli.py
and the README's example).  The jobs and the workers are the pool_ledger fixtures'
(stratum_genesis_job.json, stratum_second_job.json, stratum_ledger_sessions.json); the
submissions are found here with hashlib only, and the expected lines are what
pool_vardiff prints for them with the CPU table (the built library is needed for that
part); tests/test_pool_vardiff_cli.py checks them against the pure-Python model of
tests/sessions_ref.py.

  stratum_vardiff_submits.txt    farm.1 (difficulty 2^-20) finds 12 shares and solo.1 6
                                 in the first six seconds and satoshi.1 the genesis
                                 block; "@6000"; farm.1 goes on at its old difficulty
                                 (two shares that miss the raised target) and at the new
                                 one, with a duplicate; "@12000"; one last share
  stratum_vardiff_expected.json  what pool_vardiff prints for them with FLAGS, plain
                                 and with --dedup

    python3 tests/golden/make_vardiff_golden.py [DIR]     (DIR: where to write; default: beside this file)
"""
import io
import json
import os
import sys

from make_jobs_golden import header_hash, params, text

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FLAGS = ["--target-ms", "1000", "--window-ms", "5000", "--band-permille", "100"]
JOBS = ["stratum_genesis_job.json", "stratum_second_job.json"]


def target_fx(fx):
    return (0xffff << 240) // fx


def main(dest=HERE):
    with open(os.path.join(HERE, "stratum_genesis_job.json")) as f:
        genesis = json.load(f)
    with open(os.path.join(HERE, "stratum_second_job.json")) as f:
        second = json.load(f)
    with open(os.path.join(HERE, "stratum_ledger_sessions.json")) as f:
        workers = {w: bytes.fromhex(v["extranonce1"]) for w, v in json.load(f)["workers"].items()}
    ntime2 = int(second["notify"][7], 16)
    cursor = {}

    def find(worker, extranonce2, meets, misses=None):
        """The next nonce whose hash is at or below T(meets) and, with `misses`, above T(misses)."""
        nonce = cursor.get((worker, extranonce2), 0)
        while True:
            h = header_hash(second, workers[worker], extranonce2, ntime2, nonce, 1)
            nonce += 1
            if h <= target_fx(meets) and (misses is None or h > target_fx(misses)):
                cursor[(worker, extranonce2)] = nonce
                return params(worker, second, extranonce2, ntime2, nonce - 1)

    block = params("satoshi.1", genesis, 29, int(genesis["notify"][7], 16), 2083236893)
    first = [find("farm.1", 0, 4096) for _ in range(12)] + [find("solo.1", 0, 4096) for _ in range(6)] + [block]
    # farm.1 is at 8192 now: two shares of its old difficulty only, four of the new one, one of them twice
    old = [find("farm.1", 1, 4096, misses=8192) for _ in range(2)]
    new = [find("farm.1", 1, 8192) for _ in range(4)]
    lines = first[:7] + ["hello"] + first[7:] + ["@6000"] + old[:1] + new[:2] + old[1:] + new[2:] + new[:1] + ["@12000"]
    lines += [find("solo.1", 1, 4096)]
    with open(os.path.join(dest, "stratum_vardiff_submits.txt"), "w") as f:
        f.write("".join((text(p) if isinstance(p, list) else p) + "\n" for p in lines))

    sys.path.insert(0, ROOT)
    from distributed_bitcoin_minter_amd import pool_vardiff

    def run(*flags):
        out = io.StringIO()
        argv = [os.path.join(HERE, "stratum_ledger_sessions.json"), os.path.join(dest, "stratum_vardiff_submits.txt")]
        argv += [os.path.join(HERE, j) for j in JOBS] + ["--cpu"] + FLAGS + list(flags)
        assert pool_vardiff.main(argv, out=out) == 0
        return out.getvalue().splitlines()

    with open(os.path.join(dest, "stratum_vardiff_expected.json"), "w") as f:
        json.dump({"flags": FLAGS, "plain": run(), "dedup": run("--dedup")}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:2])
