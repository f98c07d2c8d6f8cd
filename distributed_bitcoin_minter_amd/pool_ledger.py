"""Pool-side share accounting over several live jobs:
``pool_ledger SESSIONS.json FILE|- JOB.json [JOB.json ...] [--cpu] [--dedup] [--capacity N] [--batch B] [--ntime-slack S] [--by-worker]``.

``pool_jobs`` with the last stage of a pool behind it: every hashed submission is
also credited to its worker's account in a ledger (``bm_ledger_verify_jobs``: one
call verifies a batch, de-duplicates it with ``--dedup`` and credits it; ``--cpu``:
the CPU ledger, no GPU needed).  The arguments, the output lines, the closing line
and exit status 3 on a full share set are ``pool_jobs``'s.

The account of a worker is its name up to the first ``.``, so ``satoshi.1`` and
``satoshi.2`` share a row; ``--by-worker`` gives every worker a row of its own.  A
share weighs ``floor(difficulty * 2^32)`` of its worker, at least 1, so an account's
``Work`` reads as expected hashes.  After the closing line comes one line per account,
in name order:

    Account <name> Accepted a Blocks b Rejected r AboveTarget x Ntime y Duplicate z Extranonce2 w Work W Best <16 hex digits or ->

``Rejected`` is the sum of the four reasons after it; ``Best`` is the lowest accepted
hash's first eight bytes.  Lines rejected before hashing (``malformed``, ``worker``,
``job``, ...) belong to no account.
"""
import argparse
import sys
from fractions import Fraction

from ._lib import (BM_EFULL, BM_LEDGER_NO_BEST, BM_MAX_JOB_SUBMITS, BM_MAX_LEDGER_ROWS, BM_MAX_SHARE_SET, U32_MAX, U64_MAX,
                   BtcMinerError, Ledger, ShareSet)
from .pool_jobs import jobs_lines, load_jobs
from .pool_verify import _load_json, load_sessions
from .stratum_job import _bound


def account_map(workers, index, by_worker):
    """(account names in name order, accounts[] by session, weights[] by session)
    from SESSIONS.json's workers and load_sessions' index."""
    def account(worker):
        return worker if by_worker else worker.split(".", 1)[0]

    names = sorted({account(w) for w in workers})
    row = {name: k for k, name in enumerate(names)}
    accounts, weights = [0] * len(index), [1] * len(index)
    for worker, s in index.items():
        accounts[s] = row[account(worker)]
        weights[s] = min(U64_MAX, max(1, int(Fraction(workers[worker]["difficulty"]) * (1 << 32))))
    return names, accounts, weights


def account_line(name, row):
    best = "-" if row.best == BM_LEDGER_NO_BEST else "%016x" % row.best
    return ("Account %s Accepted %d Blocks %d Rejected %d AboveTarget %d Ntime %d Duplicate %d Extranonce2 %d Work %d Best %s"
            % (name, row.accepted, row.blocks, row.rejected, row.above_target, row.ntime, row.duplicates, row.invalid,
               row.work, best))


def main(argv=None, out=None, ctx=None, stdin=None):
    """ctx: a context to use instead of a new one-GPU Context (tests); stdin:
    the stream that ``-`` reads (default sys.stdin)."""
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="pool_ledger",
                                 description="verify the mining.submit params of many workers against several live Stratum "
                                             "jobs and credit them to accounts")
    ap.add_argument("sessions", help="the workers' extranonce1 and difficulty (JSON)")
    ap.add_argument("file", help="submissions, one per line (-: standard input)")
    ap.add_argument("jobs", nargs="+", help="the job files (JSON), one per live job")
    ap.add_argument("--cpu", action="store_true", help="verify and credit on the CPU: no GPU needed")
    ap.add_argument("--ntime-slack", default=None, metavar="S", help="each job's window is [its ntime, its ntime + S]")
    ap.add_argument("--dedup", action="store_true", help="reject duplicate shares through one share set for all jobs")
    ap.add_argument("--capacity", default=None, metavar="N", help="with --dedup: hashes the set holds (default: the input's lines)")
    ap.add_argument("--batch", default=None, metavar="B", help="lines per library call (default: all in one batch)")
    ap.add_argument("--by-worker", action="store_true", help="one account per worker, not per name before the first '.'")
    try:
        a = ap.parse_intermixed_args(argv)
    except SystemExit as e:  # argparse has printed its message
        return e.code if isinstance(e.code, int) else 2
    try:
        slack = None if a.ntime_slack is None else _bound(a.ntime_slack, "the slack", U32_MAX)
        jobs, by_id, masks, size = load_jobs(a.jobs, slack)
        obj = _load_json(a.sessions)
        sessions, index = load_sessions(obj, size)
        names, accounts, weights = account_map(obj["workers"], index, a.by_worker)
        if len(names) > BM_MAX_LEDGER_ROWS:
            raise ValueError(f"at most {BM_MAX_LEDGER_ROWS} accounts, got {len(names)}")
        if a.capacity is not None and not a.dedup:
            raise ValueError("--capacity goes with --dedup")
        capacity = None if a.capacity is None else _bound(a.capacity, "the capacity", BM_MAX_SHARE_SET)
        batch = None if a.batch is None else _bound(a.batch, "the batch", BM_MAX_JOB_SUBMITS)
        if capacity == 0 or batch == 0:
            raise ValueError("the capacity and the batch are at least 1")
        if a.file == "-":
            lines = (stdin or sys.stdin).read().splitlines()
        else:
            try:
                with open(a.file) as f:
                    lines = f.read().splitlines()
            except OSError as e:
                raise ValueError(f"{a.file}: {e}") from None
        if a.dedup and capacity is None:
            capacity = max(1, len(lines))
            if capacity > BM_MAX_SHARE_SET:
                raise ValueError(f"the input has more than {BM_MAX_SHARE_SET} lines: a share set holds no more")
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2

    def run(context):
        rows = max(1, len(names))
        with (Ledger.cpu(rows) if context is None else Ledger(context, rows)) as ledger:
            share_set = None
            if a.dedup:
                share_set = ShareSet.cpu(capacity) if context is None else ShareSet(context, capacity)
            try:
                got, counts = jobs_lines(lines, by_id, masks, index,
                                         lambda subs: ledger.verify_jobs(jobs, sessions, subs, share_set, accounts, weights),
                                         batch, dedup=a.dedup)
                return got, counts, [account_line(name, row) for name, row in zip(names, ledger.read())]
            finally:
                if share_set is not None:
                    share_set.close()

    try:
        if a.cpu:
            got, counts, tallies = run(None)
        elif ctx is not None:
            got, counts, tallies = run(ctx)
        else:
            from ._lib import Context
            with Context(num_gpus=1) as own:
                got, counts, tallies = run(own)
    except BtcMinerError as e:
        if e.status != BM_EFULL:
            raise
        print(f"the share set is full: more than {capacity} distinct accepted hashes (--capacity)", file=sys.stderr)
        return 3
    for ln in got:
        print(ln, file=out)
    if a.dedup:
        print("Verified %d Accepted %d Blocks %d Rejected %d Duplicates %d" % counts, file=out)
    else:
        print("Verified %d Accepted %d Blocks %d Rejected %d" % counts[:4], file=out)
    for ln in tallies:
        print(ln, file=out)
    out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
