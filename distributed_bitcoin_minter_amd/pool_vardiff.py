"""Pool-side share accounting with variable difficulty over several live jobs:
``pool_vardiff SESSIONS.json FILE|- JOB.json [JOB.json ...] [--cpu] [--dedup] [--capacity N] [--batch B] [--ntime-slack S] [--by-worker] [policy options]``.

``pool_ledger`` with the sessions in a session table (``bm_sessions_t``: on the GPU
the workers' extranonce1, targets, accounts and weights stay on the device between
calls) and a vardiff step on top.  The arguments, the verdict lines, the closing line,
the ``Account`` lines and exit status 3 on a full share set are ``pool_ledger``'s.  A
worker starts at the difficulty SESSIONS.json gives it, in units of 2^-32:
``floor(difficulty * 2^32)``, at least 1; its share target is
``floor(0xffff * 2^240 / that)`` and its window starts at ``--start-ms``.

The submissions file may carry lines ``@<ms>``, a decimal time in milliseconds.  At
each one the submissions read so far are verified through the table
(``bm_sessions_verify_jobs``: verify, de-duplicate, credit and tally in one call) and
their lines printed; then the table is retargeted at that time
(``bm_sessions_retarget``) and every changed worker prints, in the workers' order,

    SetDifficulty <worker> <new_fx>/4294967296

which is what a pool would send as ``mining.set_difficulty``.  A retarget takes effect
with the next submission read: there is no grace period for shares of jobs sent
before it, so a few above-target rejects may follow a raise.  After the ``Account``
lines comes one line per worker, in SESSIONS.json's order:

    Worker <name> Difficulty <fx>/4294967296 Retargets r

The policy (``bm_vardiff_policy_t``; all integer arithmetic):

    --target-ms T       a share should take T ms                       (default 10000)
    --window-ms W       a worker is evaluated once W ms have passed    (default 60000)
    --burst B           or once it has B accepted shares; 0: off       (default 0)
    --band-permille P   a change within old * P / 1000 is none         (default 250)
    --max-up U          one step multiplies by at most U               (default 4)
    --max-down D        one step divides by at most D                  (default 4)
    --min-fx, --max-fx  the difficulty stays in [min, max], in 2^-32   (default 1, 2^64 - 1)
    --start-ms S        the time the workers connected                 (default 0)
"""
import argparse
import sys

from ._lib import (BM_EFULL, BM_MAX_JOB_SUBMITS, BM_MAX_LEDGER_ROWS, BM_MAX_POOL_SESSIONS, BM_MAX_SHARE_SET, U32_MAX,
                   U64_MAX, BtcMinerError, Ledger, SessionTable, ShareSet, VardiffPolicy)
from .pool_jobs import jobs_lines, load_jobs
from .pool_ledger import account_line, account_map
from .pool_verify import _load_json, load_sessions
from .stratum_job import _bound

FX_ONE = 1 << 32


def split_at_marks(lines):
    """[(lines, ms or None)]: the input cut after each ``@<ms>`` line; the last piece
    has no time.  ValueError for a mark that is no decimal time."""
    pieces, held = [], []
    for line in lines:
        text = line.strip()
        if not text.startswith("@"):
            held.append(line)
            continue
        if not text[1:].isdigit() or int(text[1:]) > U64_MAX:
            raise ValueError(f"{text!r}: a time mark is @ and a decimal number of milliseconds below 2^64")
        pieces.append((held, int(text[1:])))
        held = []
    pieces.append((held, None))
    return pieces


def main(argv=None, out=None, ctx=None, stdin=None):
    """ctx: a context to use instead of a new one-GPU Context (tests); stdin:
    the stream that ``-`` reads (default sys.stdin)."""
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="pool_vardiff",
                                 description="verify the mining.submit params of many workers against several live Stratum "
                                             "jobs through a session table, credit them and retarget the workers")
    ap.add_argument("sessions", help="the workers' extranonce1 and starting difficulty (JSON)")
    ap.add_argument("file", help="submissions and @<ms> time marks, one per line (-: standard input)")
    ap.add_argument("jobs", nargs="+", help="the job files (JSON), one per live job")
    ap.add_argument("--cpu", action="store_true", help="the CPU table, ledger and set: no GPU needed")
    ap.add_argument("--ntime-slack", default=None, metavar="S", help="each job's window is [its ntime, its ntime + S]")
    ap.add_argument("--dedup", action="store_true", help="reject duplicate shares through one share set for all jobs")
    ap.add_argument("--capacity", default=None, metavar="N", help="with --dedup: hashes the set holds (default: the input's lines)")
    ap.add_argument("--batch", default=None, metavar="B", help="lines per library call (default: all up to a time mark)")
    ap.add_argument("--by-worker", action="store_true", help="one account per worker, not per name before the first '.'")
    ap.add_argument("--target-ms", default="10000", metavar="T")
    ap.add_argument("--window-ms", default="60000", metavar="W")
    ap.add_argument("--burst", default="0", metavar="B")
    ap.add_argument("--band-permille", default="250", metavar="P")
    ap.add_argument("--max-up", default="4", metavar="U")
    ap.add_argument("--max-down", default="4", metavar="D")
    ap.add_argument("--min-fx", default="1")
    ap.add_argument("--max-fx", default=str(U64_MAX))
    ap.add_argument("--start-ms", default="0", metavar="S")
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
        if len(names) > BM_MAX_LEDGER_ROWS or len(sessions) > BM_MAX_POOL_SESSIONS:
            raise ValueError(f"at most {BM_MAX_LEDGER_ROWS} accounts and {BM_MAX_POOL_SESSIONS} workers")
        if a.capacity is not None and not a.dedup:
            raise ValueError("--capacity goes with --dedup")
        capacity = None if a.capacity is None else _bound(a.capacity, "the capacity", BM_MAX_SHARE_SET)
        batch = None if a.batch is None else _bound(a.batch, "the batch", BM_MAX_JOB_SUBMITS)
        if capacity == 0 or batch == 0:
            raise ValueError("the capacity and the batch are at least 1")
        policy = VardiffPolicy(target_ms=_bound(a.target_ms, "the target time", U32_MAX),
                               window_ms=_bound(a.window_ms, "the window", U64_MAX),
                               min_difficulty_fx=_bound(a.min_fx, "the lowest difficulty", U64_MAX),
                               max_difficulty_fx=_bound(a.max_fx, "the highest difficulty", U64_MAX),
                               burst=_bound(a.burst, "the burst", U32_MAX),
                               band_permille=_bound(a.band_permille, "the band", 1000),
                               max_up=_bound(a.max_up, "the step up", U32_MAX), max_down=_bound(a.max_down, "the step down", U32_MAX))
        if policy.target_ms < 1 or policy.max_up < 1 or policy.max_down < 1:
            raise ValueError("the target time and the steps are at least 1")
        if not 1 <= policy.min_difficulty_fx <= policy.max_difficulty_fx:
            raise ValueError("the lowest difficulty is at least 1 and at most the highest")
        start = _bound(a.start_ms, "the start time", U64_MAX)
        if a.file == "-":
            lines = (stdin or sys.stdin).read().splitlines()
        else:
            try:
                with open(a.file) as f:
                    lines = f.read().splitlines()
            except OSError as e:
                raise ValueError(f"{a.file}: {e}") from None
        pieces = split_at_marks(lines)
        if a.dedup and capacity is None:
            capacity = max(1, len(lines))
            if capacity > BM_MAX_SHARE_SET:
                raise ValueError(f"the input has more than {BM_MAX_SHARE_SET} lines: a share set holds no more")
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    workers = sorted(index, key=index.get)  # by session

    def run(context):
        rows = max(1, len(names))
        table = SessionTable.cpu(max(1, len(sessions))) if context is None else SessionTable(context, max(1, len(sessions)))
        ledger = Ledger.cpu(rows) if context is None else Ledger(context, rows)
        share_set = None
        if a.dedup:
            share_set = ShareSet.cpu(capacity) if context is None else ShareSet(context, capacity)
        try:
            table.set([(s.extranonce1, w, acc) for s, w, acc in zip(sessions, weights, accounts)], start)
            got, totals = [], [0] * 5
            for held, ms in pieces:
                text, counts = jobs_lines(held, by_id, masks, index,
                                          lambda subs: table.verify_jobs(jobs, subs, ledger, share_set), batch, dedup=a.dedup)
                got += text
                totals = [x + y for x, y in zip(totals, counts)]
                if ms is not None:
                    changes, _result = table.retarget(ms, policy)
                    got += ["SetDifficulty %s %d/%d" % (workers[c.session], c.new_fx, FX_ONE) for c in changes]
            tallies = [account_line(name, row) for name, row in zip(names, ledger.read())]
            state = table.state() if sessions else []
            tallies += ["Worker %s Difficulty %d/%d Retargets %d" % (w, s.difficulty_fx, FX_ONE, s.retargets)
                        for w, s in zip(workers, state)]
            return got, tuple(totals), tallies
        finally:
            if share_set is not None:
                share_set.close()
            ledger.close()
            table.close()

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
