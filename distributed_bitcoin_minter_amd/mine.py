"""Bitcoin block-header search: ``mine HEADERHEX [--target HEX | --zero-bits N] [LOWER [UPPER]]``.

HEADERHEX is an 80-byte block header in hex (160 digits; its last four bytes,
the nonce field, are ignored).  Finds the first nonce n in [LOWER, UPPER]
(default [0, 2^32-1]) whose double SHA-256 of the header, read as a
little-endian 256-bit integer, is at most the target, with the library's
header search (``bm_search_header_gpu``), and prints

    Found <64-hex hash> <nonce>

or, when no nonce of the range meets the target,

    NotFound <64-hex hash> <nonce>

the range's best share (the minimum of the hash's top 64 bits, the smallest
nonce on equal top bits) with its full hash.

The target is the header's own ``bits`` field unless ``--target`` (a 256-bit
number in hex, up to 64 digits) or ``--zero-bits N`` (the hash starts with at
least N zero bits: target 2^(256-N) - 1) says otherwise.
"""
import argparse
import re
import sys

U32_MAX = (1 << 32) - 1
U256_MAX = (1 << 256) - 1
HEADER_BYTES = 80


def target_for_zero_bits(bits: int) -> int:
    """The largest 256-bit hash with `bits` leading zero bits."""
    if not 0 <= bits <= 256:
        raise ValueError(f"--zero-bits must be in 0..256, got {bits}")
    return (1 << (256 - bits)) - 1


def header_bits(header: bytes) -> int:
    """The compact target field of a header (bytes 72..75, little-endian)."""
    return int.from_bytes(header[72:76], "little")


def _u32(text, what):
    if not re.fullmatch(r"[0-9]{1,10}", text, flags=re.ASCII) or int(text) > U32_MAX:
        raise ValueError(f"{what} must be an unsigned 32-bit integer, got {text!r}")
    return int(text)


def parse_args(argv):
    """(header bytes, target int, lower, upper); ValueError for a bad header,
    target or bound."""
    ap = argparse.ArgumentParser(prog="mine", description="first nonce whose block-header hash meets a target")
    ap.add_argument("header", help="the 80-byte block header, 160 hex digits")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--target", help="256-bit target in hex (default: the header's bits field)")
    g.add_argument("--zero-bits", help="leading zero bits of the hash instead of a target")
    ap.add_argument("lower", nargs="?", default="0")
    ap.add_argument("upper", nargs="?", default=str(U32_MAX))
    a = ap.parse_intermixed_args(argv)  # LOWER and UPPER may follow the options
    if not re.fullmatch(r"[0-9a-fA-F]{%d}" % (2 * HEADER_BYTES), a.header, flags=re.ASCII):
        raise ValueError(f"HEADERHEX must be {2 * HEADER_BYTES} hex digits ({HEADER_BYTES} bytes)")
    header = bytes.fromhex(a.header)
    if a.target is not None:
        if not re.fullmatch(r"(0[xX])?[0-9a-fA-F]{1,64}", a.target, flags=re.ASCII):
            raise ValueError(f"--target must be a 256-bit number in hex, got {a.target!r}")
        target = int(a.target, 16)
    elif a.zero_bits is not None:
        if not re.fullmatch(r"[0-9]{1,3}", a.zero_bits, flags=re.ASCII):
            raise ValueError(f"--zero-bits must be in 0..256, got {a.zero_bits!r}")
        target = target_for_zero_bits(int(a.zero_bits))
    else:
        from ._lib import bits_to_target
        try:
            target = bits_to_target(header_bits(header))
        except ValueError as e:
            raise ValueError(f"the header's bits field is not a usable target ({e}); give --target") from None
    return header, target, _u32(a.lower, "LOWER"), _u32(a.upper, "UPPER")


def main(argv=None, out=None, ctx=None):
    """ctx: a context to use instead of a new one-GPU Context (tests)."""
    out = out or sys.stdout
    try:
        header, target, lower, upper = parse_args(argv)
    except ValueError as e:
        print(e, file=sys.stderr)
        return 2
    if ctx is not None:
        found, h, n = ctx.search_header(header, lower, upper, target)
    else:
        from ._lib import Context
        with Context(num_gpus=1) as own:
            found, h, n = own.search_header(header, lower, upper, target)
    print("Found" if found else "NotFound", f"{h:064x}", n, file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
