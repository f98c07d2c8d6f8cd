"""Proof-of-work search: ``pow MSG BITS [LOWER [UPPER]]``.

Finds the first nonce n in [LOWER, UPPER] (default [0, 2^64-1]) whose
``Hash(MSG, n)`` starts with at least BITS zero bits, i.e. is at most
``2^(64-BITS) - 1``, with the library's target search
(``bm_search_target_gpu``), in steps of 2^32 nonces, and prints

    Found <hash> <nonce>

or, when no nonce of the range meets the target,

    NotFound <minHash> <nonce>

the range's minimum (the lexicographic min over the steps), which is what
the request client's ``Result`` line would hold.
"""
import argparse
import re
import sys

U64_MAX = (1 << 64) - 1
STEP = 1 << 32


def target_for_bits(bits: int) -> int:
    """The largest hash with `bits` leading zero bits: 2^(64-bits) - 1."""
    if not 0 <= bits <= 64:
        raise ValueError(f"BITS must be in 0..64, got {bits}")
    return (1 << (64 - bits)) - 1


def _u64(text, what):
    """An unsigned 64-bit decimal, as Go's strconv.ParseUint(s, 10, 64)."""
    if not re.fullmatch(r"[0-9]+", text, flags=re.ASCII) or len(text.lstrip("0")) > 20:
        raise ValueError(f"{what} must be an unsigned 64-bit integer, got {text!r}")
    v = int(text.lstrip("0") or "0")
    if v > U64_MAX:
        raise ValueError(f"{what} must be an unsigned 64-bit integer, got {text!r}")
    return v


def parse_args(argv):
    """(msg bytes, bits, lower, upper); ValueError for a bad BITS or bound."""
    ap = argparse.ArgumentParser(prog="pow", description="first nonce whose hash has BITS leading zero bits")
    ap.add_argument("message")
    ap.add_argument("bits")
    ap.add_argument("lower", nargs="?", default="0")
    ap.add_argument("upper", nargs="?", default=str(U64_MAX))
    a = ap.parse_args(argv)
    if not re.fullmatch(r"[0-9]{1,3}", a.bits, flags=re.ASCII):
        raise ValueError(f"BITS must be in 0..64, got {a.bits!r}")
    bits = int(a.bits)
    target_for_bits(bits)
    return a.message.encode(), bits, _u64(a.lower, "LOWER"), _u64(a.upper, "UPPER")


def search(ctx, msg: bytes, bits: int, lower: int, upper: int, step: int = STEP):
    """(found, hash, nonce) over [lower, upper], one target search per `step`
    nonces until the first hit or the end of the range."""
    target = target_for_bits(bits)
    best = (U64_MAX, U64_MAX)
    lo = lower
    while lo <= upper:
        hi = min(upper, lo + step - 1)
        found, h, n = ctx.search_target(msg, lo, hi, target)
        if found:
            return True, h, n
        best = min(best, (h, n))
        lo = hi + 1
    return False, best[0], best[1]


def main(argv=None, out=None):
    out = out or sys.stdout
    try:
        msg, bits, lower, upper = parse_args(argv)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    from ._lib import Context
    with Context(num_gpus=1) as ctx:
        found, h, n = search(ctx, msg, bits, lower, upper)
    print("Found" if found else "NotFound", h, n, file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
