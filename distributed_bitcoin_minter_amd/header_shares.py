"""Block-header share enumeration:
``header_shares HEADERHEX (--target HEX | --zero-bits N) [--cap N] [--ntime-rolls R] [LOWER [UPPER]]``.

HEADERHEX is an 80-byte block header in hex (160 digits; its last four bytes,
the nonce field, are ignored).  Lists every nonce n in [LOWER, UPPER] (default
[0, 2^32-1]) whose double SHA-256 of the header, read as a little-endian
256-bit integer, is at most the share target, with the library's header hit
enumeration (``bm_search_header_hits_gpu``): what a pool miner submits.  The
share target is ``--target`` (a 256-bit number in hex, up to 64 digits) or
``--zero-bits N`` (the hash starts with at least N zero bits).

``--ntime-rolls R`` (default 1) scans the range under R successive values of
the header's time field (bytes 68..71, little-endian), starting at the
header's own.  A library call takes one header; the rolling happens here.  A
piece that holds more than ``--cap`` hits (default 4096) is halved and both
halves are scanned again; a single nonce holds at most one hit, so this ends.
Prints

    Share <64-hex hash> <ntime> <nonce>

per hit, ascending by (ntime, nonce), with ``Block`` in place of ``Share``
when the hash also meets the header's own ``bits`` target, then

    Shares <count> Best <64-hex hash> <ntime> <nonce>

the number of hits and the best share of everything scanned (the minimum of
the hash's top 64 bits; the earliest ntime, then the smallest nonce, on equal
top bits) with its full hash.
"""
import argparse
import sys

from .mine import U32_MAX, U256_MAX, header_bits, parse_args as _mine_args

DEFAULT_CAP = 4096
MAX_CAP = 1 << 20  # BM_MAX_HEADER_HITS
MAX_ROLLS = 1 << 16
NTIME_AT = 68  # the time field: header[68:72], little-endian


def _count(text, what, hi):
    if not (text.isascii() and text.isdigit() and len(text) <= 10) or not 1 <= int(text) <= hi:
        raise ValueError(f"{what} must be in 1..{hi}, got {text!r}")
    return int(text)


def parse_args(argv):
    """(header bytes, target int, lower, upper, cap, rolls); ValueError for a
    bad header, target, bound, cap or roll count.  HEADERHEX, --target,
    --zero-bits, LOWER and UPPER are mine's, with a target required."""
    ap = argparse.ArgumentParser(prog="header_shares",
                                 description="every nonce whose block-header hash meets a share target")
    ap.add_argument("header", help="the 80-byte block header, 160 hex digits")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--target", help="256-bit share target in hex")
    g.add_argument("--zero-bits", help="leading zero bits of the hash instead of a target")
    ap.add_argument("--cap", default=str(DEFAULT_CAP), help="hits per library call, at most (1..%d)" % MAX_CAP)
    ap.add_argument("--ntime-rolls", default="1", help="successive values of the time field to scan (1..%d)" % MAX_ROLLS)
    ap.add_argument("lower", nargs="?", default="0")
    ap.add_argument("upper", nargs="?", default=str(U32_MAX))
    a = ap.parse_intermixed_args(argv)  # LOWER and UPPER may follow the options
    opt = ["--target=" + a.target] if a.target is not None else ["--zero-bits=" + a.zero_bits]
    header, target, lower, upper = _mine_args([a.header] + opt + [a.lower, a.upper])
    return header, target, lower, upper, _count(a.cap, "--cap", MAX_CAP), _count(a.ntime_rolls, "--ntime-rolls",
                                                                                 MAX_ROLLS)


def header_ntime(header: bytes) -> int:
    return int.from_bytes(header[NTIME_AT:NTIME_AT + 4], "little")


def with_ntime(header: bytes, ntime: int) -> bytes:
    return header[:NTIME_AT] + (ntime & U32_MAX).to_bytes(4, "little") + header[NTIME_AT + 4:]


def block_target(header: bytes):
    """The header's own target (its bits field), or None when that field is
    no usable target."""
    from ._lib import bits_to_target
    try:
        return bits_to_target(header_bits(header))
    except ValueError:
        return None


def enumerate_hits(ctx, header: bytes, target: int, lower: int, upper: int, cap: int = DEFAULT_CAP):
    """(hits, (best hash, its nonce)) of one header over [lower, upper]: hits
    is every (hash, nonce) at or below the target, ascending by nonce.  A
    piece with more than `cap` hits is halved and both halves are scanned
    again."""
    best = (U256_MAX, U32_MAX)
    hits = []
    # pieces still to scan, lowest on top, so the hits come out ascending
    todo = [(lower, upper)] if lower <= upper else []
    while todo:
        a, b = todo.pop()
        count, got, low = ctx.search_header_hits(header, a, b, target, cap)
        if got is None:
            if a == b:
                raise RuntimeError(f"{count} hits reported for the single nonce {a}")
            mid = a + (b - a) // 2
            todo.append((mid + 1, b))
            todo.append((a, mid))
            continue
        hits.extend(got)
        # the library's order: the hash's top 64 bits, then the nonce
        best = min(best, tuple(low), key=lambda s: (s[0] >> 192, s[1]))
    return hits, best


def main(argv=None, out=None, ctx=None):
    """ctx: a context to use instead of a new one-GPU Context (tests)."""
    out = out or sys.stdout
    try:
        header, target, lower, upper, cap, rolls = parse_args(argv)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    except SystemExit as e:  # argparse has printed its message
        return e.code if isinstance(e.code, int) else 2

    def run(c):
        found = []
        for r in range(rolls):
            ntime = (header_ntime(header) + r) & U32_MAX
            hits, best = enumerate_hits(c, with_ntime(header, ntime), target, lower, upper, cap)
            found.append((ntime, hits, best))
        return found

    if ctx is not None:
        found = run(ctx)
    else:
        from ._lib import Context
        with Context(num_gpus=1) as own:
            found = run(own)
    own_target = block_target(header)
    total = 0
    for ntime, hits, _ in found:
        for h, n in hits:
            is_block = own_target is not None and h <= own_target
            print("Block" if is_block else "Share", f"{h:064x}", ntime, n, file=out)
        total += len(hits)
    ntime, _, best = min(found, key=lambda f: (f[2][0] >> 192, f[0], f[2][1]))
    print("Shares", total, "Best", f"{best[0]:064x}", ntime, best[1], file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
