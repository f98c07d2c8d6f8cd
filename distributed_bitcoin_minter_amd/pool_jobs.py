"""Pool-side share verification over several live jobs:
``pool_jobs SESSIONS.json FILE|- JOB.json [JOB.json ...] [--cpu] [--ntime-slack S] [--dedup] [--capacity N] [--batch B]``.

``pool_verify`` for a pool between two blocks: it has sent several jobs (a new
``mining.notify`` every few tens of seconds, ``clean_jobs`` false) and all of them
are still valid, so the submissions it reads mix their ids.  Each JOB.json is
``stratum_job``'s job file; ``notify[0]`` is the job's id and ``notify[7]`` its
ntime.  As in ``pool_verify`` a job file's ``extranonce1`` only fixes the size of
every worker's extranonce1 (the same in all job files here) and its ``difficulty``
and ``worker`` are not used; SESSIONS.json and FILE are ``pool_verify``'s.  Up to 64
job files.

The second param of a submission, the job id, picks the job; the first, the worker's
name, picks the session.  Every well-formed submission is rebuilt and hashed under
its own job in one batch whatever the mix (``bm_jobs_verify_gpu``: the host groups
the batch by job, one GPU lane per submission; ``--cpu``: ``bm_jobs_verify_cpu``, no
GPU needed).  ``--ntime-slack S`` gives each job the window ``[ntime, ntime + S]``
of its own ntime (decimal, or hex with 0x; no window without the option).  The
output is ``pool_verify``'s lines and closing line, with one more reject,

    Reject job <params>                an id no job file holds

(in place of ``job-id``).  With ``--dedup`` every hashed submission also goes
through one share set for all the jobs (``bm_share_set_verify_jobs``; the key is the
header hash, which separates jobs), and the lines, the closing line, ``--capacity N``
and exit status 3 are ``pool_dedup``'s.  ``--batch B`` feeds the input in batches of
B lines (default: one batch; a library call takes 2^20 submissions at most).
"""
import argparse
import json
import sys

from ._lib import (BIP320_MASK, BM_EFULL, BM_MAX_JOB_SUBMITS, BM_MAX_POOL_JOBS, BM_MAX_SHARE_SET, U32_MAX, BtcMinerError,
                   PoolJob, ShareSet, parse_jobs_submit, verify_jobs_submits_cpu)
from .pool_verify import REASONS as POOL_REASONS
from .pool_verify import _load_json, load_sessions
from .stratum_job import _bound, load_job
from .stratum_verify import parse_line

REASONS = POOL_REASONS + ("job",)


def _reason(err):
    word = str(err).split(":", 1)[0]
    return word if word in REASONS else "malformed"


def load_jobs(paths, slack):
    """(jobs, jobs_by_id, masks by id, extranonce1 size) from the job files, each
    job's window [ntime, ntime + slack] (none for slack None); ValueError for a bad
    file, a repeated id, too many files or differing extranonce1 sizes."""
    if len(paths) > BM_MAX_POOL_JOBS:
        raise ValueError(f"at most {BM_MAX_POOL_JOBS} job files, got {len(paths)}")
    jobs, by_id, masks, size = [], {}, {}, None
    for path in paths:
        job, _target, mask, _worker = load_job(_load_json(path))
        if not 1 <= len(job.extranonce1) <= 8:
            raise ValueError(f"{path}: extranonce1 must be 1..8 bytes for a pool, got {len(job.extranonce1)}")
        if size is not None and len(job.extranonce1) != size:
            raise ValueError(f"{path}: extranonce1 has {len(job.extranonce1)} bytes, the other job files' has {size}")
        size = len(job.extranonce1)
        if job.job_id in by_id:
            raise ValueError(f"{path}: the job id {job.job_id!r} is another job file's")
        by_id[job.job_id] = (len(jobs), job)
        masks[job.job_id] = mask if mask is not None else BIP320_MASK
        window = (0, U32_MAX) if slack is None else (job.ntime, min(U32_MAX, job.ntime + slack))
        jobs.append(PoolJob(job, *window))
    return jobs, by_id, masks, size


def jobs_lines(lines, by_id, masks, index, verify, batch=None, dedup=False):
    """The output lines (without the closing count) and (n, accepted, blocks,
    rejected, duplicates) for the input lines; verify(submits) -> (verdicts,
    result) is called per batch of `batch` lines (None: one batch), each of 2^20
    submissions at most."""
    rows = []      # per submission line: ("reject", reason, text) or ("hash", params text, index into verdicts)
    verdicts = []
    pending = []   # the submissions of the current batch
    held = 0       # its lines

    def flush():
        nonlocal held
        if pending:
            got, _result = verify(pending)
            verdicts.extend((v.value, v.status) for v in got)
        del pending[:]
        held = 0

    for line in lines:
        try:
            params = parse_line(line)
        except ValueError as e:
            rows.append(("reject", _reason(e), line.strip()))
        else:
            if params is None:
                continue
            text = json.dumps(params, separators=(",", ":"))
            job_id = params[1] if len(params) > 1 and isinstance(params[1], str) else None
            try:
                sub = parse_jobs_submit(params, by_id, index, masks.get(job_id, BIP320_MASK))
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
        elif status & 8:   # BM_SUBMIT_NTIME: outside its job's window, whatever the hash
            out.append(f"Reject ntime {a}")
        elif dedup and status & 16:  # BM_SUBMIT_DUPLICATE
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
    ap = argparse.ArgumentParser(prog="pool_jobs",
                                 description="verify the mining.submit params of many workers against several live Stratum jobs")
    ap.add_argument("sessions", help="the workers' extranonce1 and difficulty (JSON)")
    ap.add_argument("file", help="submissions, one per line (-: standard input)")
    ap.add_argument("jobs", nargs="+", help="the job files (JSON), one per live job")
    ap.add_argument("--cpu", action="store_true", help="verify on the CPU: no GPU needed")
    ap.add_argument("--ntime-slack", default=None, metavar="S", help="each job's window is [its ntime, its ntime + S]")
    ap.add_argument("--dedup", action="store_true", help="reject duplicate shares through one share set for all jobs")
    ap.add_argument("--capacity", default=None, metavar="N", help="with --dedup: hashes the set holds (default: the input's lines)")
    ap.add_argument("--batch", default=None, metavar="B", help="lines per library call (default: all in one batch)")
    try:
        a = ap.parse_intermixed_args(argv)
    except SystemExit as e:  # argparse has printed its message
        return e.code if isinstance(e.code, int) else 2
    try:
        slack = None if a.ntime_slack is None else _bound(a.ntime_slack, "the slack", U32_MAX)
        jobs, by_id, masks, size = load_jobs(a.jobs, slack)
        sessions, index = load_sessions(_load_json(a.sessions), size)
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
        if not a.dedup:
            verify = verify_jobs_submits_cpu if context is None else context.verify_jobs_submits
            return jobs_lines(lines, by_id, masks, index, lambda subs: verify(jobs, sessions, subs), batch)
        with (ShareSet.cpu(capacity) if context is None else ShareSet(context, capacity)) as share_set:
            return jobs_lines(lines, by_id, masks, index, lambda subs: share_set.verify_jobs(jobs, sessions, subs), batch,
                              dedup=True)

    try:
        if a.cpu:
            got, counts = run(None)
        elif ctx is not None:
            got, counts = run(ctx)
        else:
            from ._lib import Context
            with Context(num_gpus=1) as own:
                got, counts = run(own)
    except BtcMinerError as e:
        if e.status != BM_EFULL:
            raise
        print(f"the share set is full: more than {capacity} distinct accepted hashes (--capacity)", file=sys.stderr)
        return 3
    for ln in got:
        print(ln, file=out)
    if a.dedup:
        print("Verified %d Accepted %d Blocks %d Rejected %d Duplicates %d" % counts, file=out, flush=True)
    else:
        print("Verified %d Accepted %d Blocks %d Rejected %d" % counts[:4], file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
