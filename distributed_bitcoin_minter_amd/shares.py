"""Share enumeration: ``shares MSG BITS LOWER UPPER [--cap N]``.

Lists every nonce n in [LOWER, UPPER] whose ``Hash(MSG, n)`` starts with at
least BITS zero bits, i.e. is at most ``2^(64-BITS) - 1``, with the library's
hit enumeration (``bm_search_hits_gpu``), in steps of 2^32 nonces.  A step
that holds more than N hits (default 4096) is halved and both halves are
scanned again; a single nonce holds at most one hit, so this ends.  Prints

    Share <hash> <nonce>

per hit in ascending nonce order, then

    Shares <count> Min <minHash> <nonce>

the number of hits and the range's minimum (the lexicographic min over the
steps).
"""
import argparse
import sys

from .pow import STEP, U64_MAX, _u64, parse_args as _pow_args, target_for_bits

DEFAULT_CAP = 4096
MAX_CAP = 1 << 22  # BM_MAX_HITS


def parse_args(argv):
    """(msg bytes, bits, lower, upper, cap); ValueError for a bad BITS, bound
    or cap.  MSG, BITS, LOWER and UPPER are pow's, with UPPER required."""
    ap = argparse.ArgumentParser(prog="shares", description="every nonce whose hash has BITS leading zero bits")
    ap.add_argument("message")
    ap.add_argument("bits")
    ap.add_argument("lower")
    ap.add_argument("upper")
    ap.add_argument("--cap", default=str(DEFAULT_CAP), help="hits per library call, at most (1..%d)" % MAX_CAP)
    a = ap.parse_args(argv)
    msg, bits, lower, upper = _pow_args([a.message, a.bits, a.lower, a.upper])
    cap = _u64(a.cap, "--cap")
    if not 1 <= cap <= MAX_CAP:
        raise ValueError(f"--cap must be in 1..{MAX_CAP}, got {a.cap!r}")
    return msg, bits, lower, upper, cap


def enumerate_hits(ctx, msg: bytes, bits: int, lower: int, upper: int, cap: int = DEFAULT_CAP, step: int = STEP):
    """(hits, (min hash, its nonce)) over [lower, upper]: hits is every
    (hash, nonce) at or below the target, ascending by nonce.  One
    search_hits per `step` nonces; a piece with more than `cap` hits is
    halved and both halves are scanned again."""
    target = target_for_bits(bits)
    best = (U64_MAX, U64_MAX)
    hits = []
    lo = lower
    while lo <= upper:
        hi = min(upper, lo + step - 1)
        # pieces still to scan, lowest on top, so the hits come out ascending
        todo = [(lo, hi)]
        while todo:
            a, b = todo.pop()
            count, got, low = ctx.search_hits(msg, a, b, target, cap)
            if got is None:
                if a == b:
                    raise RuntimeError(f"{count} hits reported for the single nonce {a}")
                mid = a + (b - a) // 2
                todo.append((mid + 1, b))
                todo.append((a, mid))
                continue
            hits.extend(got)
            best = min(best, tuple(low))
        if hi == U64_MAX:
            break
        lo = hi + 1
    return hits, best


def main(argv=None, out=None, ctx=None):
    """ctx: a context to use instead of a new one-GPU Context (tests)."""
    out = out or sys.stdout
    try:
        msg, bits, lower, upper, cap = parse_args(argv)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    if ctx is not None:
        hits, best = enumerate_hits(ctx, msg, bits, lower, upper, cap)
    else:
        from ._lib import Context
        with Context(num_gpus=1) as own:
            hits, best = enumerate_hits(own, msg, bits, lower, upper, cap)
    for h, n in hits:
        print("Share", h, n, file=out)
    print("Shares", len(hits), "Min", best[0], best[1], file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
