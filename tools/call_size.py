#!/usr/bin/env python3
"""What one call costs at each size: GH/s
of whole calls over ranges of 2^24 .. 2^34 nonces, on one device and on a
context of N slots (default 8) all on GPU 0 -- the latter adds what an
N-device context adds per call (N submission threads, N plans, the combine;
host copies here, since RCCL refuses one GPU twice), not N GPUs' work.

Every range is 'bradfitz' starting at 10^10 (11-digit nonces, one layout
throughout, <19, 1>: the same loop as C2's <18, 1> one byte later), so the
curve isolates the per-call cost.  Each size is called at least `--reps`
times and for at least `--min-s` seconds; the rate is nonces / mean wall time
per call (host wall clock around the synchronous call).  `eff` is that rate
over the largest size's on the same context.

    python tools/call_size.py [--slots 8] [--min-bits 24] [--max-bits 34] [--out f.json] [--lib other.so]

--kind picks the entry point (default search, bm_search_gpu): target and hits
scan the same range with a target nothing meets (a full scan); the four header
kinds scan nonces [0, 2^bits - 1] of the genesis header at target 0 (header,
header_versions: a full scan) or 2^244 - 1 (the enumerations: about one hit in
2^12, cap 2^20), the version-rolling ones under 7 versions.  --bits lists the
sizes instead of a min..max run.

The server sizes jobs from this: a job of about 0.3 s is within 1% of the
asymptotic rate."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distributed_bitcoin_minter_amd import Context  # noqa: E402

MSG = b"bradfitz"
LO = 10 ** 10
GENESIS = bytes.fromhex("0100000000000000000000000000000000000000000000000000000000000000000000003ba3edfd7a7b12b27ac7"
                        "2c3e67768f617fc81bc3888a51323a9fb8aa4b1e5e4a29ab5f49ffff001d1dac2b7c")
VERSIONS7 = [0x20000000, 0x20002000, 1, 0x3FFFE000, 0, 0x20002000, 0xFFFFFFFF]
H_SOME = (1 << 244) - 1
HITS_CAP = 1 << 20

# kind -> one call over n nonces
KINDS = {
    "search": lambda c, n: c.search(MSG, LO, LO + n - 1),
    "target": lambda c, n: c.search_target(MSG, LO, LO + n - 1, 0),
    "hits": lambda c, n: c.search_hits(MSG, LO, LO + n - 1, 0, 4096),
    "header": lambda c, n: c.search_header(GENESIS, 0, n - 1, 0),
    "header_hits": lambda c, n: c.search_header_hits(GENESIS, 0, n - 1, H_SOME, HITS_CAP),
    "header_versions": lambda c, n: c.search_header_versions(GENESIS, VERSIONS7, 0, n - 1, 0),
    "header_versions_hits": lambda c, n: c.search_header_versions_hits(GENESIS, VERSIONS7, 0, n - 1, H_SOME, HITS_CAP),
}


def curve(ctx, call, bits, reps, min_s):
    out = []
    for b in bits:
        n = 1 << b
        call(ctx, n)  # warm (first launch of the layout, plan caches)
        k, t = 0, time.perf_counter()
        while k < reps or time.perf_counter() - t < min_s:
            call(ctx, n)
            k += 1
        dt = (time.perf_counter() - t) / k
        out.append({"bits": b, "nonces": n, "calls": k, "ms_per_call": round(dt * 1e3, 4),
                    "GHs": round(n / dt / 1e9, 3)})
        print(json.dumps(out[-1]), flush=True)
    top = out[-1]["GHs"]
    for e in out:
        e["eff"] = round(e["GHs"] / top, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--min-bits", type=int, default=24)
    ap.add_argument("--max-bits", type=int, default=34)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B)")
    ap.add_argument("--kind", default="search", choices=sorted(KINDS))
    ap.add_argument("--bits", type=int, nargs="+", default=None, help="these sizes, not min-bits..max-bits")
    a = ap.parse_args()
    bits = sorted(a.bits) if a.bits else list(range(a.min_bits, a.max_bits + 1))
    if "header" in a.kind and bits[-1] > 32:
        ap.error("a header nonce has 32 bits")
    call = KINDS[a.kind]
    res = {"kind": a.kind, "msg": MSG.decode(), "lower": LO, "note": __doc__.split("\n\n")[0],
           "lib": a.lib or "libbtcminer.so"}
    kw = {"lib_path": os.path.abspath(a.lib)} if a.lib else {}
    with Context(devices=[0], **kw) as c:
        print("== one device", flush=True)
        res["one_device"] = curve(c, call, bits, a.reps, a.min_s)
    with Context(devices=[0] * a.slots, **kw) as c:
        print(f"== {a.slots} slots on GPU 0 (host combine)", flush=True)
        res[f"slots_{a.slots}_on_gpu0"] = curve(c, call, bits, a.reps, a.min_s)
        st = c.last_stats()
        res["start_threads"] = st.start_threads
    for name in ("one_device", f"slots_{a.slots}_on_gpu0"):
        print(name, " ".join(f"2^{e['bits']}:{e['eff']:.3f}" for e in res[name]), flush=True)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
