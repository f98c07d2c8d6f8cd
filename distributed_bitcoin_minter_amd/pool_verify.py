"""Pool-side share verification across workers:
``pool_verify JOB.json SESSIONS.json [FILE|-] [--cpu] [--ntime-window LO HI]``.

``stratum_verify`` for a pool: the same job went to every connection, and each
connection (worker) has its own extranonce1 and its own difficulty.  JOB.json is
``stratum_job``'s job file; its ``extranonce1`` only fixes the SIZE of every
worker's extranonce1 here, and its ``difficulty`` and ``worker`` are not used.
SESSIONS.json names the workers:

    {"workers": {"name": {"extranonce1": hex, "difficulty": d}, ...}}

FILE (default ``-``, standard input) holds one submission per line in any of
``stratum_verify``'s input forms; the first param, the worker's name, picks the
session.  Every well-formed submission of a known worker is rebuilt and hashed in
one batch (``bm_pool_verify_gpu``, one GPU lane per submission; ``--cpu``:
``bm_pool_verify_cpu``, no GPU needed), under its worker's extranonce1 and
against its worker's target.  The output is ``stratum_verify``'s:

    Accept <params> <64-hex hash>      the hash meets the worker's share target
    Block <params> <64-hex hash>       the hash meets the job's nbits
    Reject <reason> <params>

with its reasons and two more: ``worker`` (a name SESSIONS.json does not hold) and
``ntime`` (hashed, but ntime lies outside ``--ntime-window LO HI``, inclusive,
decimal or hex with 0x; no window without the option), then

    Verified <n> Accepted <a> Blocks <b> Rejected <r>

Duplicate detection and vardiff are the caller's.
"""
import argparse
import json
import sys

from ._lib import (BIP320_MASK, BM_MAX_JOB_SUBMITS, U32_MAX, PoolSession, _hex_bytes, difficulty_to_target,
                   parse_pool_submit, verify_pool_submits_cpu)
from .stratum_job import _bound, load_job
from .stratum_verify import REASONS as VERIFY_REASONS
from .stratum_verify import parse_line

REASONS = VERIFY_REASONS + ("worker", "ntime")


def load_sessions(obj, size):
    """(sessions, index by worker name) from the decoded SESSIONS.json, every
    extranonce1 of size bytes; ValueError for a missing or malformed field."""
    if not isinstance(obj, dict) or not isinstance(obj.get("workers"), dict):
        raise ValueError('the sessions file must hold {"workers": {name: {"extranonce1": hex, "difficulty": d}}}')
    sessions, index = [], {}
    for name, w in obj["workers"].items():
        if not isinstance(w, dict) or "extranonce1" not in w or "difficulty" not in w:
            raise ValueError(f"worker {name!r} needs an extranonce1 and a difficulty")
        en1 = _hex_bytes(w["extranonce1"], f"worker {name!r}: extranonce1", size)
        index[name] = len(sessions)
        sessions.append(PoolSession(en1, difficulty_to_target(w["difficulty"])))
    return sessions, index


def _reason(err):
    word = str(err).split(":", 1)[0]
    return word if word in REASONS else "malformed"


def verify_lines(lines, job, sessions, index, mask, window, verify):
    """The output lines (without the closing count) and (n, accepted, blocks,
    rejected) for the input lines; verify(job, sessions, submits, lo, hi) is
    Context.verify_pool_submits or verify_pool_submits_cpu."""
    rows = []      # per submission line: ("reject", reason, text) or ("hash", params text, index into subs)
    subs = []
    for line in lines:
        try:
            params = parse_line(line)
        except ValueError as e:
            rows.append(("reject", _reason(e), line.strip()))
            continue
        if params is None:
            continue
        text = json.dumps(params, separators=(",", ":"))
        try:
            sub = parse_pool_submit(params, job, index, mask)
        except ValueError as e:
            rows.append(("reject", _reason(e), text))
            continue
        rows.append(("hash", text, len(subs)))
        subs.append(sub)
    verdicts = []
    for lo in range(0, len(subs), BM_MAX_JOB_SUBMITS):  # a library call takes 2^20 submissions at most
        got, _result = verify(job, sessions, subs[lo:lo + BM_MAX_JOB_SUBMITS], window[0], window[1])
        verdicts.extend((v.value, v.status) for v in got)
    out, accepted, blocks = [], 0, 0
    for kind, a, b in rows:
        if kind == "reject":
            out.append(f"Reject {a} {b}")
            continue
        value, status = verdicts[b]
        if status & 4:    # BM_SUBMIT_INVALID (parse_pool_submit lets none through; a stand-in verifier might)
            out.append(f"Reject extranonce2 {a}")
        elif status & 8:  # BM_SUBMIT_NTIME: outside the window, whatever the hash
            out.append(f"Reject ntime {a}")
        elif status & 2:  # BM_SUBMIT_BLOCK
            out.append(f"Block {a} {value:064x}")
            accepted, blocks = accepted + 1, blocks + 1
        elif status & 1:  # BM_SUBMIT_SHARE
            out.append(f"Accept {a} {value:064x}")
            accepted += 1
        else:
            out.append(f"Reject above-target {a}")
    return out, (len(rows), accepted, blocks, len(rows) - accepted)


def _load_json(path):
    try:
        with open(path) as f:
            return json.load(f)
    except (OSError, json.JSONDecodeError) as e:
        raise ValueError(f"{path}: {e}") from None


def main(argv=None, out=None, ctx=None, stdin=None):
    """ctx: a context to use instead of a new one-GPU Context (tests); stdin:
    the stream that ``-`` reads (default sys.stdin)."""
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="pool_verify",
                                 description="verify the mining.submit params of many workers against one Stratum job")
    ap.add_argument("job", help="the job file (JSON)")
    ap.add_argument("sessions", help="the workers' extranonce1 and difficulty (JSON)")
    ap.add_argument("file", nargs="?", default="-", help="submissions, one per line (default -: standard input)")
    ap.add_argument("--cpu", action="store_true", help="verify on the CPU (bm_pool_verify_cpu): no GPU needed")
    ap.add_argument("--ntime-window", nargs=2, default=None, metavar=("LO", "HI"),
                    help="reject an ntime outside LO..HI, inclusive (decimal, or hex with 0x)")
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
        if a.file == "-":
            lines = (stdin or sys.stdin).read().splitlines()
        else:
            try:
                with open(a.file) as f:
                    lines = f.read().splitlines()
            except OSError as e:
                raise ValueError(f"{a.file}: {e}") from None
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    mask = mask if mask is not None else BIP320_MASK
    if a.cpu:
        got, counts = verify_lines(lines, job, sessions, index, mask, window, verify_pool_submits_cpu)
    elif ctx is not None:
        got, counts = verify_lines(lines, job, sessions, index, mask, window, ctx.verify_pool_submits)
    else:
        from ._lib import Context
        with Context(num_gpus=1) as own:
            got, counts = verify_lines(lines, job, sessions, index, mask, window, own.verify_pool_submits)
    for ln in got:
        print(ln, file=out)
    print("Verified %d Accepted %d Blocks %d Rejected %d" % counts, file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
