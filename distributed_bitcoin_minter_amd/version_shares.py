"""Version-rolling share enumeration:
``version_shares HEADERHEX (--target HEX | --zero-bits N) [--versions N] [--mask HEX] [--cap N] [LOWER [UPPER]]``.

HEADERHEX, the target options, LOWER and UPPER are ``header_shares``'s;
``--versions`` (default 4) and ``--mask`` are ``mine_versions``'s: the header's
own version field is rolled into N version fields inside the mask (default
1fffe000, BIP 320's).  Lists every (nonce, version) pair of [LOWER, UPPER]
(default [0, 2^32-1]) whose double SHA-256 of the header under that version is
at most the share target, with the library's version-rolling share enumeration
(``bm_search_header_versions_hits_gpu``): what a pool miner with version
rolling on submits.

A piece that holds more than ``--cap`` hits (default 65536) is halved and both
halves are scanned again.  A single nonce can hold one hit per version, so a
``--cap`` below the number of versions is refused.  Prints

    Share <64-hex hash> <nonce> <version as 8 hex digits>

per hit, ascending by (nonce, rolling order of the version), with ``Block`` in
place of ``Share`` when the hash also meets the header's own ``bits`` target,
then

    Shares <count> Best <64-hex hash> <nonce> <version as 8 hex digits>

the number of hits and the best share of everything scanned (the minimum of
the hash's top 64 bits, then the smallest nonce, then the earliest version)
with its full hash.
"""
import argparse
import sys

from .header_shares import MAX_CAP, _count, block_target
from .mine import U32_MAX, U256_MAX
from .mine_versions import DEFAULT_MASK, MAX_VERSIONS, parse_args as _versions_args

DEFAULT_CAP = 65536
DEFAULT_VERSIONS = 4


def parse_args(argv):
    """(header bytes, versions list, target int, lower, upper, cap); ValueError
    for a bad header, count, mask, target, bound or cap, and for a cap below
    the number of versions."""
    ap = argparse.ArgumentParser(prog="version_shares",
                                 description="every (nonce, version) pair whose block-header hash meets a share target")
    ap.add_argument("header", help="the 80-byte block header, 160 hex digits")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--target", help="256-bit share target in hex")
    g.add_argument("--zero-bits", help="leading zero bits of the hash instead of a target")
    ap.add_argument("--versions", default=str(DEFAULT_VERSIONS), help="version fields to roll (1..%d)" % MAX_VERSIONS)
    ap.add_argument("--mask", default="%08x" % DEFAULT_MASK, help="the version bits to roll in, in hex")
    ap.add_argument("--cap", default=str(DEFAULT_CAP), help="hits per library call, at most (1..%d)" % MAX_CAP)
    ap.add_argument("lower", nargs="?", default="0")
    ap.add_argument("upper", nargs="?", default=str(U32_MAX))
    a = ap.parse_intermixed_args(argv)  # LOWER and UPPER may follow the options
    opt = ["--target=" + a.target] if a.target is not None else ["--zero-bits=" + a.zero_bits]
    header, versions, target, lower, upper = _versions_args(
        [a.header, "--versions=" + a.versions, "--mask=" + a.mask] + opt + [a.lower, a.upper])
    cap = _count(a.cap, "--cap", MAX_CAP)
    if cap < len(versions):  # one nonce can hold a hit per version: halving could not end
        raise ValueError(f"--cap must be at least the number of versions ({len(versions)}), got {cap}")
    return header, versions, target, lower, upper, cap


def enumerate_hits(ctx, header: bytes, versions, target: int, lower: int, upper: int, cap: int = DEFAULT_CAP):
    """(hits, (best hash, its nonce, its version index)) of one header under
    `versions` over [lower, upper]: hits is every (hash, nonce, index) at or
    below the target, ascending by (nonce, index).  A piece with more than
    `cap` hits is halved and both halves are scanned again."""
    best = (U256_MAX, U32_MAX, 0)
    hits = []
    # pieces still to scan, lowest on top, so the hits come out ascending
    todo = [(lower, upper)] if lower <= upper else []
    while todo:
        a, b = todo.pop()
        count, got, low = ctx.search_header_versions_hits(header, versions, a, b, target, cap)
        if got is None:
            if a == b:
                raise RuntimeError(f"{count} hits reported for the single nonce {a} under {len(versions)} versions")
            mid = a + (b - a) // 2
            todo.append((mid + 1, b))
            todo.append((a, mid))
            continue
        hits.extend(got)
        # the library's order: the hash's top 64 bits, then the nonce, then the index
        best = min(best, tuple(low), key=lambda s: (s[0] >> 192, s[1], s[2]))
    return hits, best


def main(argv=None, out=None, ctx=None):
    """ctx: a context to use instead of a new one-GPU Context (tests)."""
    out = out or sys.stdout
    try:
        header, versions, target, lower, upper, cap = parse_args(argv)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    except SystemExit as e:  # argparse has printed its message
        return e.code if isinstance(e.code, int) else 2
    if ctx is not None:
        hits, best = enumerate_hits(ctx, header, versions, target, lower, upper, cap)
    else:
        from ._lib import Context
        with Context(num_gpus=1) as own:
            hits, best = enumerate_hits(own, header, versions, target, lower, upper, cap)
    own_target = block_target(header)
    for h, n, vi in hits:
        is_block = own_target is not None and h <= own_target
        print("Block" if is_block else "Share", f"{h:064x}", n, f"{versions[vi]:08x}", file=out)
    print("Shares", len(hits), "Best", f"{best[0]:064x}", best[1], f"{versions[best[2]]:08x}", file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
