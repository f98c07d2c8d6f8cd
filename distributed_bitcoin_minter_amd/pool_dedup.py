"""Pool-side share verification with duplicate detection:
``pool_dedup JOB.json SESSIONS.json [FILE|-] [--cpu] [--ntime-window LO HI] [--capacity N] [--batch B]``.

``pool_verify`` with a share set kept across the invocation: JOB.json,
SESSIONS.json, FILE and the reasons are ``pool_verify``'s, and every hashed
submission also goes through one set of header hashes (``bm_share_set_verify`` on
a device set; ``--cpu``: on a host set, no GPU needed).  A share or block whose
hash the set already holds -- from an earlier line, whichever worker sent it -- is
a duplicate.  The input is fed to the set in batches of ``--batch B`` lines (default:
one batch; a library call takes 2^20 submissions at most), so a duplicate may be
caught inside one call or across two; the answers are the same.  ``--capacity N``
is the set's size in hashes (default: the input's lines, at least 1).

The output is ``pool_verify``'s lines, with one more reject,

    Reject duplicate <params>          an accepted hash seen before: not counted as accepted

(after ``extranonce2`` and ``ntime``, before ``Block`` and ``Accept``), then

    Verified <n> Accepted <a> Blocks <b> Rejected <r> Duplicates <d>

A set too small for the input's distinct accepted hashes prints a message to
standard error and exits with status 3, with nothing on standard output.  vardiff
is the caller's.
"""
import argparse
import json
import sys

from ._lib import (BIP320_MASK, BM_EFULL, BM_MAX_JOB_SUBMITS, BM_MAX_SHARE_SET, U32_MAX, BtcMinerError, ShareSet,
                   parse_pool_submit)
from .pool_verify import _load_json, _reason, load_sessions
from .stratum_job import _bound, load_job
from .stratum_verify import parse_line


def dedup_lines(lines, job, sessions, index, mask, window, share_set, batch=None):
    """The output lines (without the closing count) and (n, accepted, blocks,
    rejected, duplicates) for the input lines, through share_set.verify in batches
    of `batch` lines (None: one batch), each of 2^20 submissions at most."""
    rows = []      # per submission line: ("reject", reason, text) or ("hash", params text, index into verdicts)
    verdicts = []
    pending = []   # the submissions of the current batch
    held = 0       # its lines

    def flush():
        nonlocal held
        if pending:
            got, _result = share_set.verify(job, sessions, pending, window[0], window[1])
            verdicts.extend((v.value, v.status) for v in got)
        del pending[:]
        held = 0

    for line in lines:
        try:
            params = parse_line(line)
        except ValueError as e:
            rows.append(("reject", _reason(e), line.strip()))
            params = None
        else:
            if params is None:
                continue
            text = json.dumps(params, separators=(",", ":"))
            try:
                sub = parse_pool_submit(params, job, index, mask)
            except ValueError as e:
                rows.append(("reject", _reason(e), text))
            else:
                rows.append(("hash", text, len(verdicts) + len(pending)))
                pending.append(sub)
        held += 1
        if (batch is not None and held >= batch) or len(pending) >= BM_MAX_JOB_SUBMITS:
            flush()
    flush()
    out, accepted, blocks, duplicates = [], 0, 0, 0
    for kind, a, b in rows:
        if kind == "reject":
            out.append(f"Reject {a} {b}")
            continue
        value, status = verdicts[b]
        if status & 4:     # BM_SUBMIT_INVALID
            out.append(f"Reject extranonce2 {a}")
        elif status & 8:   # BM_SUBMIT_NTIME: outside the window, whatever the hash
            out.append(f"Reject ntime {a}")
        elif status & 16:  # BM_SUBMIT_DUPLICATE
            out.append(f"Reject duplicate {a}")
            duplicates += 1
        elif status & 2:   # BM_SUBMIT_BLOCK
            out.append(f"Block {a} {value:064x}")
            accepted, blocks = accepted + 1, blocks + 1
        elif status & 1:   # BM_SUBMIT_SHARE
            out.append(f"Accept {a} {value:064x}")
            accepted += 1
        else:
            out.append(f"Reject above-target {a}")
    return out, (len(rows), accepted, blocks, len(rows) - accepted, duplicates)


def main(argv=None, out=None, ctx=None, stdin=None):
    """ctx: a context to use instead of a new one-GPU Context (tests); stdin:
    the stream that ``-`` reads (default sys.stdin)."""
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="pool_dedup",
                                 description="verify the mining.submit params of many workers against one Stratum job "
                                             "and reject duplicate shares")
    ap.add_argument("job", help="the job file (JSON)")
    ap.add_argument("sessions", help="the workers' extranonce1 and difficulty (JSON)")
    ap.add_argument("file", nargs="?", default="-", help="submissions, one per line (default -: standard input)")
    ap.add_argument("--cpu", action="store_true", help="verify on the CPU (a host share set): no GPU needed")
    ap.add_argument("--ntime-window", nargs=2, default=None, metavar=("LO", "HI"),
                    help="reject an ntime outside LO..HI, inclusive (decimal, or hex with 0x)")
    ap.add_argument("--capacity", default=None, metavar="N", help="hashes the set holds (default: the input's lines)")
    ap.add_argument("--batch", default=None, metavar="B", help="lines per call on the set (default: all in one batch)")
    try:
        a = ap.parse_args(argv)
    except SystemExit as e:  # argparse has printed its message
        return e.code if isinstance(e.code, int) else 2
    try:
        job, _target, mask, _worker = load_job(_load_json(a.job))
        if not 1 <= len(job.extranonce1) <= 8:
            raise ValueError(f"{a.job}: extranonce1 must be 1..8 bytes for a pool, got {len(job.extranonce1)}")
        sessions, index = load_sessions(_load_json(a.sessions), len(job.extranonce1))
        window = (0, U32_MAX)
        if a.ntime_window is not None:
            window = (_bound(a.ntime_window[0], "the window's LO", U32_MAX),
                      _bound(a.ntime_window[1], "the window's HI", U32_MAX))
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
        if capacity is None:
            capacity = max(1, len(lines))
            if capacity > BM_MAX_SHARE_SET:
                raise ValueError(f"the input has more than {BM_MAX_SHARE_SET} lines: a share set holds no more")
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    mask = mask if mask is not None else BIP320_MASK

    def run(make_set):
        with make_set() as share_set:
            return dedup_lines(lines, job, sessions, index, mask, window, share_set, batch)

    try:
        if a.cpu:
            got, counts = run(lambda: ShareSet.cpu(capacity))
        elif ctx is not None:
            got, counts = run(lambda: ShareSet(ctx, capacity))
        else:
            from ._lib import Context
            with Context(num_gpus=1) as own:
                got, counts = run(lambda: ShareSet(own, capacity))
    except BtcMinerError as e:
        if e.status != BM_EFULL:
            raise
        print(f"the share set is full: more than {capacity} distinct accepted hashes (--capacity)", file=sys.stderr)
        return 3
    for ln in got:
        print(ln, file=out)
    print("Verified %d Accepted %d Blocks %d Rejected %d Duplicates %d" % counts, file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
