"""Version-rolling block-header search:
``mine_versions HEADERHEX --versions N [--mask HEX] [--target HEX | --zero-bits N] [LOWER [UPPER]]``.

HEADERHEX, the target options, LOWER and UPPER are ``mine``'s.  The header's
own version field (bytes 0..3, little-endian) is rolled into N version fields
inside ``--mask`` (default 1fffe000, the bits BIP 320 leaves to the miner: the
i-th version is the header's with the bits of i deposited into the mask's bit
positions, lowest first), and the range is searched under all of them in one
library call (``bm_search_header_versions_gpu``).  Prints

    Found <64-hex hash> <nonce> <version as 8 hex digits>

for the smallest nonce at which any of the versions meets the target (the
earliest version in rolling order when several do), or

    NotFound <64-hex hash> <nonce> <version as 8 hex digits>

with the best share of everything scanned (the minimum of the hash's top 64
bits, then the smallest nonce, then the earliest version).
"""
import argparse
import re
import sys

from .mine import U32_MAX, parse_args as _mine_args

MAX_VERSIONS = 64  # BM_MAX_HEADER_VERSIONS
DEFAULT_MASK = 0x1fffe000


def header_version(header: bytes) -> int:
    return int.from_bytes(header[0:4], "little")


def parse_args(argv):
    """(header bytes, versions list, target int, lower, upper); ValueError for
    a bad header, count, mask, target or bound."""
    ap = argparse.ArgumentParser(prog="mine_versions",
                                 description="first nonce at which any rolled version of a block header meets a target")
    ap.add_argument("header", help="the 80-byte block header, 160 hex digits")
    ap.add_argument("--versions", required=True, help="version fields to roll (1..%d)" % MAX_VERSIONS)
    ap.add_argument("--mask", default="%08x" % DEFAULT_MASK, help="the version bits to roll in, in hex")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--target", help="256-bit target in hex (default: the header's bits field)")
    g.add_argument("--zero-bits", help="leading zero bits of the hash instead of a target")
    ap.add_argument("lower", nargs="?", default="0")
    ap.add_argument("upper", nargs="?", default=str(U32_MAX))
    a = ap.parse_intermixed_args(argv)  # LOWER and UPPER may follow the options
    opt = ["--target=" + a.target] if a.target is not None else []
    opt += ["--zero-bits=" + a.zero_bits] if a.zero_bits is not None else []
    header, target, lower, upper = _mine_args([a.header] + opt + [a.lower, a.upper])
    if not re.fullmatch(r"[0-9]{1,3}", a.versions, flags=re.ASCII) or not 1 <= int(a.versions) <= MAX_VERSIONS:
        raise ValueError(f"--versions must be in 1..{MAX_VERSIONS}, got {a.versions!r}")
    if not re.fullmatch(r"(0[xX])?[0-9a-fA-F]{1,8}", a.mask, flags=re.ASCII):
        raise ValueError(f"--mask must be a 32-bit number in hex, got {a.mask!r}")
    from ._lib import roll_versions
    versions = roll_versions(header_version(header), int(a.versions), int(a.mask, 16))  # ValueError: mask too small
    return header, versions, target, lower, upper


def main(argv=None, out=None, ctx=None):
    """ctx: a context to use instead of a new one-GPU Context (tests)."""
    out = out or sys.stdout
    try:
        header, versions, target, lower, upper = parse_args(argv)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    except SystemExit as e:  # argparse has printed its message
        return e.code if isinstance(e.code, int) else 2
    if ctx is not None:
        found, h, n, vi = ctx.search_header_versions(header, versions, lower, upper, target)
    else:
        from ._lib import Context
        with Context(num_gpus=1) as own:
            found, h, n, vi = own.search_header_versions(header, versions, lower, upper, target)
    print("Found" if found else "NotFound", f"{h:064x}", n, f"{versions[vi]:08x}", file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
