"""Pool-side share verification: ``stratum_verify JOB.json [FILE|-] [--cpu]``.

JOB.json is ``stratum_job``'s job file (what the pool sent: ``notify``,
``extranonce1``, ``extranonce2_size``, ``difficulty`` and, optionally,
``version_mask`` and ``worker``).  FILE (default ``-``, standard input) holds one
submission per line: either the bare JSON array of ``mining.submit``'s params

    ["worker","job id","extranonce2","ntime","nonce","version bits"]

(five params without version rolling) or a ``Submit ...`` / ``Block ...`` line as
``stratum_job`` prints it; the keyword and whatever follows the array (the hash)
are ignored on input, and so are blank lines and ``stratum_job``'s closing
``Shares ...`` line, so

    stratum_job JOB.json ... | stratum_verify JOB.json -

round-trips.  Every well-formed submission is rebuilt and hashed in one batch by
the library's verifier (``bm_job_verify_gpu``, one GPU lane per submission;
``--cpu``: ``bm_job_verify_cpu``, no GPU needed) at the target of the job's
difficulty.  Prints, in input order,

    Accept <params> <64-hex hash>      the hash meets the share target
    Block <params> <64-hex hash>       the hash meets the job's nbits
    Reject <reason> <params>

with the reasons ``above-target`` (hashed, but above the share target),
``extranonce2`` (not 2 * extranonce2_size hex digits), ``version-bits`` (bits
outside the negotiated mask), ``job-id`` (another job's id) and ``malformed``
(not a JSON array of 5 or 6 params, or a field that is not 8 hex digits; the
line is echoed in place of the params), then

    Verified <n> Accepted <a> Blocks <b> Rejected <r>

where a counts the Accept and the Block lines and b the Block lines alone.
Duplicate detection, an ntime window and vardiff are the caller's.
"""
import argparse
import json
import sys

from ._lib import BIP320_MASK, BM_MAX_JOB_SUBMITS, parse_submit, verify_submits_cpu
from .stratum_job import load_job

KEYWORDS = ("Submit", "Block", "Accept")
REASONS = ("above-target", "extranonce2", "version-bits", "job-id", "malformed")


def parse_line(line):
    """The params list of one input line, or None for a line to skip (blank, or
    stratum_job's closing ``Shares`` line); ValueError("malformed: ...") for
    anything that holds no JSON array."""
    text = line.strip()
    if not text or text.split(None, 1)[0] == "Shares":
        return None
    word = text.split(None, 1)[0]
    if word in KEYWORDS:
        text = text[len(word):].lstrip()
    if not text.startswith("["):
        raise ValueError("malformed: no JSON array of params")
    try:
        params, _end = json.JSONDecoder().raw_decode(text)  # whatever follows the array is ignored
    except json.JSONDecodeError as e:
        raise ValueError(f"malformed: {e}") from None
    if not isinstance(params, list):
        raise ValueError("malformed: no JSON array of params")
    return params


def _reason(err):
    word = str(err).split(":", 1)[0]
    return word if word in REASONS else "malformed"


def verify_lines(lines, job, target, mask, verify):
    """The output lines (without the closing count) and (n, accepted, blocks,
    rejected) for the input lines; verify(job, submits, target) is
    Context.verify_submits or verify_submits_cpu."""
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
            sub = parse_submit(params, job, mask)
        except ValueError as e:
            rows.append(("reject", _reason(e), text))
            continue
        rows.append(("hash", text, len(subs)))
        subs.append(sub)
    verdicts = []
    for lo in range(0, len(subs), BM_MAX_JOB_SUBMITS):  # a library call takes 2^20 submissions at most
        got, _result = verify(job, subs[lo:lo + BM_MAX_JOB_SUBMITS], target)
        verdicts.extend((v.value, v.status) for v in got)
    out, accepted, blocks = [], 0, 0
    for kind, a, b in rows:
        if kind == "reject":
            out.append(f"Reject {a} {b}")
            continue
        value, status = verdicts[b]
        if status & 4:    # BM_SUBMIT_INVALID (parse_submit lets none through; a stand-in verifier might)
            out.append(f"Reject extranonce2 {a}")
        elif status & 2:  # BM_SUBMIT_BLOCK
            out.append(f"Block {a} {value:064x}")
            accepted, blocks = accepted + 1, blocks + 1
        elif status & 1:  # BM_SUBMIT_SHARE
            out.append(f"Accept {a} {value:064x}")
            accepted += 1
        else:
            out.append(f"Reject above-target {a}")
    return out, (len(rows), accepted, blocks, len(rows) - accepted)


def main(argv=None, out=None, ctx=None, stdin=None):
    """ctx: a context to use instead of a new one-GPU Context (tests); stdin:
    the stream that ``-`` reads (default sys.stdin)."""
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="stratum_verify",
                                 description="verify mining.submit params against a Stratum job")
    ap.add_argument("job", help="the job file (JSON)")
    ap.add_argument("file", nargs="?", default="-", help="submissions, one per line (default -: standard input)")
    ap.add_argument("--cpu", action="store_true", help="verify on the CPU (bm_job_verify_cpu): no GPU needed")
    try:
        a = ap.parse_args(argv)
    except SystemExit as e:  # argparse has printed its message
        return e.code if isinstance(e.code, int) else 2
    try:
        try:
            with open(a.job) as f:
                obj = json.load(f)
        except (OSError, json.JSONDecodeError) as e:
            raise ValueError(f"{a.job}: {e}") from None
        job, target, mask, _worker = load_job(obj)
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
        got, counts = verify_lines(lines, job, target, mask, verify_submits_cpu)
    elif ctx is not None:
        got, counts = verify_lines(lines, job, target, mask, ctx.verify_submits)
    else:
        from ._lib import Context
        with Context(num_gpus=1) as own:
            got, counts = verify_lines(lines, job, target, mask, own.verify_submits)
    for ln in got:
        print(ln, file=out)
    print("Verified %d Accepted %d Blocks %d Rejected %d" % counts, file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
