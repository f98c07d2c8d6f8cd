"""Stratum job mining:
``stratum_job JOB.json [--versions N] [--extranonce2 LO HI] [--cap N] [LOWER [UPPER]]``.

JOB.json is what a pool sent, as one JSON object::

    {"notify": [job_id, prevhash, coinb1, coinb2, [branch...], version, nbits, ntime, clean_jobs],
     "extranonce1": "hex", "extranonce2_size": n, "difficulty": d,
     "version_mask": "1fffe000", "worker": "name"}

``notify`` holds the nine params of ``mining.notify`` as sent (prevhash
word-swapped; version, nbits and ntime big-endian hex), ``extranonce1`` and
``extranonce2_size`` are ``mining.subscribe``'s answer, ``difficulty`` is
``mining.set_difficulty``'s.  ``version_mask`` (BIP 310) and ``worker`` are
optional.  Scans every extranonce2 of [LO, HI] (default 0 0; hex or decimal),
each under N rolled versions (default 4 inside the mask; 1, the job's own
version, without one), over the nonces [LOWER, UPPER] (default [0, 2^32-1])
with the library's job call (``bm_search_job_shares_gpu``), at the target of
the difficulty.

A piece that holds more than ``--cap`` shares (default 65536) is halved, first
its extranonce2 range, then its nonce range, and both halves are scanned again.
Prints

    Submit <mining.submit params as JSON> <64-hex hash>

per share, ascending by (extranonce2, nonce, rolling order of the version), with
``Block`` in place of ``Submit`` when the hash also meets the job's ``nbits``,
then

    Shares <count> Best <64-hex hash> <extranonce2 hex> <nonce> <version as 8 hex digits>

the best share of everything scanned (the minimum of the hash's top 64 bits,
then the smallest extranonce2, nonce and version index) with its full hash.
"""
import argparse
import json
import sys

from ._lib import (BIP320_MASK, BM_MAX_HEADER_VERSIONS, BM_MAX_JOB_HEADERS, U32_MAX, U256_MAX, Job,
                   difficulty_to_target, roll_versions, submit_params)
from .header_shares import MAX_CAP, _count

DEFAULT_CAP = 65536
DEFAULT_VERSIONS = 4


def load_job(obj):
    """(Job, target int, mask or None, worker) from the decoded JOB.json;
    ValueError for a missing or malformed field."""
    if not isinstance(obj, dict):
        raise ValueError("the job file must hold one JSON object")
    for key in ("notify", "extranonce1", "extranonce2_size", "difficulty"):
        if key not in obj:
            raise ValueError(f"the job file has no {key!r}")
    if not isinstance(obj["notify"], list):
        raise ValueError("notify must be the list of mining.notify's params")
    job = Job.from_notify(obj["notify"], obj["extranonce1"], obj["extranonce2_size"])
    target = difficulty_to_target(obj["difficulty"])
    mask = None
    if obj.get("version_mask") is not None:
        text = obj["version_mask"]
        if not isinstance(text, str) or not 1 <= len(text) <= 8:
            raise ValueError(f"version_mask must be up to 8 hex digits, got {text!r}")
        try:
            mask = int(text, 16)
        except ValueError:
            raise ValueError(f"version_mask must be up to 8 hex digits, got {text!r}") from None
    worker = obj.get("worker", "")
    if not isinstance(worker, str):
        raise ValueError("worker must be a string")
    return job, target, mask, worker


def _bound(text, what, hi):
    try:
        v = int(text, 16) if text.lower().startswith("0x") else int(text, 10)
    except ValueError:
        raise ValueError(f"{what} must be a number, got {text!r}") from None
    if not 0 <= v <= hi:
        raise ValueError(f"{what} must be in 0..{hi}, got {text!r}")
    return v


def parse_args(argv):
    """(job, versions, mask, worker, target, en2_lo, en2_hi, lower, upper, cap);
    ValueError for a bad job file, count, bound or cap, and for a cap below the
    number of versions."""
    ap = argparse.ArgumentParser(prog="stratum_job", description="every share of a Stratum job, as mining.submit params")
    ap.add_argument("job", help="the job file (JSON)")
    ap.add_argument("--versions", default=None, help="version fields to roll (1..%d)" % BM_MAX_HEADER_VERSIONS)
    ap.add_argument("--extranonce2", nargs=2, default=["0", "0"], metavar=("LO", "HI"),
                    help="the extranonce2 values to scan, inclusive (decimal, or hex with 0x)")
    ap.add_argument("--cap", default=str(DEFAULT_CAP), help="shares per library call, at most (1..%d)" % MAX_CAP)
    ap.add_argument("lower", nargs="?", default="0")
    ap.add_argument("upper", nargs="?", default=str(U32_MAX))
    a = ap.parse_intermixed_args(argv)
    try:
        with open(a.job) as f:
            obj = json.load(f)
    except (OSError, json.JSONDecodeError) as e:
        raise ValueError(f"{a.job}: {e}") from None
    job, target, mask, worker = load_job(obj)
    nver = _count(a.versions, "--versions", BM_MAX_HEADER_VERSIONS) if a.versions is not None else (
        DEFAULT_VERSIONS if mask is not None else 1)
    if mask is None and nver > 1:
        raise ValueError("the job has no version_mask: --versions must be 1")
    versions = roll_versions(job.version, nver, mask) if mask is not None else [job.version]
    top = (1 << (8 * job.extranonce2_size)) - 1
    en2_lo, en2_hi = (_bound(t, "--extranonce2", top) for t in a.extranonce2)
    lower, upper = _bound(a.lower, "LOWER", U32_MAX), _bound(a.upper, "UPPER", U32_MAX)
    cap = _count(a.cap, "--cap", MAX_CAP)
    if cap < len(versions):  # one nonce can hold a share per version: halving could not end
        raise ValueError(f"--cap must be at least the number of versions ({len(versions)}), got {cap}")
    return job, versions, mask, worker, target, en2_lo, en2_hi, lower, upper, cap


def enumerate_shares(ctx, job, versions, target: int, en2_lo: int, en2_hi: int, lower: int, upper: int,
                     cap: int = DEFAULT_CAP):
    """(shares, best) of a job over [en2_lo, en2_hi] x [lower, upper]: shares
    is every share dict of Context.search_job_shares, ascending by (extranonce2,
    nonce, index); best is (hash, extranonce2, nonce, index).  A piece with more
    than `cap` shares is halved, its extranonce2 range first, then its nonce
    range, and both halves are scanned again."""
    best = (U256_MAX, en2_lo, U32_MAX, 0)
    shares = []
    if en2_lo > en2_hi or lower > upper:
        return shares, best
    # pieces still to scan, lowest on top, so the shares come out ascending;
    # a library call takes BM_MAX_JOB_HEADERS extranonce2 values at most
    todo = [(a, min(a + BM_MAX_JOB_HEADERS - 1, en2_hi), lower, upper)
            for a in range(en2_lo, en2_hi + 1, BM_MAX_JOB_HEADERS)][::-1]
    first = True
    while todo:
        ea, eb, a, b = todo.pop()
        count, got, low = ctx.search_job_shares(job, versions, ea, eb, a, b, target, cap)
        if got is None:
            if ea < eb:
                mid = ea + (eb - ea) // 2
                todo.append((mid + 1, eb, a, b))
                todo.append((ea, mid, a, b))
            elif a < b:
                mid = a + (b - a) // 2
                todo.append((ea, eb, mid + 1, b))
                todo.append((ea, eb, a, mid))
            else:
                raise RuntimeError(f"{count} shares reported for extranonce2 {ea}, nonce {a} under "
                                   f"{len(versions)} versions")
            continue
        shares.extend(got)
        # the library's order: the hash's top 64 bits, then extranonce2, nonce, index
        low = tuple(low)
        if first or (low[0] >> 192, low[1], low[2], low[3]) < (best[0] >> 192, best[1], best[2], best[3]):
            best, first = low, False
    return shares, best


def main(argv=None, out=None, ctx=None):
    """ctx: a context to use instead of a new one-GPU Context (tests)."""
    out = out or sys.stdout
    try:
        job, versions, mask, worker, target, en2_lo, en2_hi, lower, upper, cap = parse_args(argv)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    except SystemExit as e:  # argparse has printed its message
        return e.code if isinstance(e.code, int) else 2
    if ctx is not None:
        shares, best = enumerate_shares(ctx, job, versions, target, en2_lo, en2_hi, lower, upper, cap)
    else:
        from ._lib import Context
        with Context(num_gpus=1) as own:
            shares, best = enumerate_shares(own, job, versions, target, en2_lo, en2_hi, lower, upper, cap)
    submit_mask = mask if mask is not None else BIP320_MASK
    for s in shares:
        params = json.dumps(submit_params(worker, job.job_id, s, submit_mask), separators=(",", ":"))
        print("Block" if s["is_block"] else "Submit", params, f"{s['hash']:064x}", file=out)
    print("Shares", len(shares), "Best", f"{best[0]:064x}", "%0*x" % (2 * job.extranonce2_size, best[1]), best[2],
          f"{versions[best[3]]:08x}", file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
