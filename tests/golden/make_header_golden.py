#!/usr/bin/env python3
"""Writes header_vectors.json: two public Bitcoin block headers with their
nonce, bits and hash, and a few window facts about them, all from hashlib.

    python tests/golden/make_header_golden.py
"""
import hashlib
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))

HEADERS = {
    "genesis": ("01000000" + "00" * 32 + "3ba3edfd7a7b12b27ac72c3e67768f617fc81bc3888a51323a9fb8aa4b1e5e4a"
                + "29ab5f49" + "ffff001d" + "1dac2b7c"),
    "block125552": ("0100000081cd02ab7e569e8bcd9317e2fe99f2de44d49ab2b8851ba4a308000000000000"
                    "e320b6c2fffc8d750423db8b1eb942ae710e951ed797f7affc8892b0f1fc122b"
                    "c7f5d74d" "f2b9441a" "42a14695"),
}


def H(header: bytes, nonce: int) -> int:
    d = hashlib.sha256(hashlib.sha256(header[:76] + struct.pack("<I", nonce)).digest()).digest()
    return int.from_bytes(d, "little")


def bits_to_target(nbits: int) -> int:
    mant, exp = nbits & 0x7FFFFF, nbits >> 24
    return mant >> (8 * (3 - exp)) if exp < 3 else mant << (8 * (exp - 3))


def first_with_zero_bits(header, lo, hi, bits):
    t = (1 << (256 - bits)) - 1
    return next((n for n in range(lo, hi + 1) if H(header, n) <= t), None)


def main():
    out = {"headers": []}
    for name, hx in HEADERS.items():
        header = bytes.fromhex(hx)
        assert len(header) == 80
        nonce = struct.unpack("<I", header[76:])[0]
        bits = struct.unpack("<I", header[72:76])[0]
        target = bits_to_target(bits)
        h = H(header, nonce)
        assert h <= target
        lo, hi = nonce - (1 << 16), nonce + (1 << 16)
        hits = [n for n in range(lo, hi + 1) if H(header, n) <= target]
        assert hits == [nonce], hits
        out["headers"].append({"name": name, "header": hx, "nonce": nonce, "bits": bits,
                               "target": f"{target:064x}", "hash": f"{h:064x}",
                               "window": [lo, hi], "window_hits": hits})
    g = bytes.fromhex(HEADERS["genesis"])
    low = [(H(g, n), n) for n in range(1 << 16)]
    hmin, nmin = min(low)
    top_lo, top_hi = (1 << 32) - (1 << 16), (1 << 32) - 1
    out["genesis_windows"] = {
        "low": {"range": [0, (1 << 16) - 1], "first_12_bits": first_with_zero_bits(g, 0, 65535, 12),
                "first_16_bits": first_with_zero_bits(g, 0, 65535, 16), "min_hash": f"{hmin:064x}",
                "min_nonce": nmin},
        "top": {"range": [top_lo, top_hi], "first_12_bits": first_with_zero_bits(g, top_lo, top_hi, 12)},
    }
    with open(os.path.join(HERE, "header_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
