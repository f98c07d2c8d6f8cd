#!/usr/bin/env python3
"""Measure the block-header search (bm_search_header_gpu) on one GPU.

    python tools/bench_header.py [--rounds 10] [--warmup 2] [--ops N] [--lib PATH ...]
                                 [--out profiles/header/bench_header.json]

Medians of host wall time around synchronous calls, alternated in one process:
  scan      a not-found scan of the genesis header over [0, 2^32-1] with
            target 0 (every nonce hashed twice), against bm_search_gpu on C2
            ("bradfitz", [0, 2^32-1]): GH/s of both, and -- with --ops, the
            executed VALU ops per nonce read off the inner loop's ISA
            (tools/check_inner.py -v) -- the ratio of the measured rate to
            the prediction  C2 rate x 1,254 / ops.
  control   C2 against C2: the run's own A/B noise.
  genesis   the time to find the genesis nonce from 0 at the header's own
            target, against the ideal  2083236893 / scan rate.
  libs      with --lib (repeatable): the same scan through other builds of
            the library (e.g. another occupancy, or the priority pass),
            alternated with this one.
Every answer is checked: C2 against the committed golden, the scan's best
share against bm_header_hash_gpu, genesis against its known nonce.  No torch."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C2_OPS = 1254  # executed VALU lane-ops per nonce of C2's inner loop


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ops", type=int, default=None, help="VALU ops per nonce of the header kernel's inner loop (check_inner.py row hdrv1)")
    ap.add_argument("--lib", action="append", default=[], help="another build of the library to alternate with")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    from distributed_bitcoin_minter_amd import Context, bits_to_target
    gold = json.load(open(os.path.join(ROOT, "tests/golden/full_range.json")))
    c2 = next(c for c in gold["cases"] if c["config"] == "C2")
    msg, lo, hi = bytes.fromhex(c2["msg_hex"]), c2["lower"], c2["upper"]
    c2_gold = (c2["hash"], c2["nonce"])
    g = next(h for h in json.load(open(os.path.join(ROOT, "tests/golden/header_vectors.json")))["headers"]
             if h["name"] == "genesis")
    header, g_target = bytes.fromhex(g["header"]), bits_to_target(g["bits"])
    n = 1 << 32
    out = {"tool": "bench_header", "rounds": a.rounds, "warmup": a.warmup, "ops_per_nonce": a.ops}

    def med(xs):
        return round(statistics.median(xs), 3)

    with Context(devices=[0]) as ctx:
        def c2_search():
            assert ctx.search(msg, lo, hi) == c2_gold

        def scan(c=ctx):
            found, h, nn = c.search_header(header, 0, n - 1, 0)
            assert not found
            return h, nn

        def genesis():
            assert ctx.search_header(header, 0, n - 1, g_target) == (True, int(g["hash"], 16), g["nonce"])

        for _ in range(a.warmup):
            c2_search()
            best = scan()
            genesis()
        assert ctx.header_hash_many(header, [best[1]]) == [best[0]]
        out["best_share"] = {"hash": f"{best[0]:064x}", "nonce": best[1]}

        t_a, t_b = [], []
        for _ in range(a.rounds):
            t_a.append(timed(c2_search)[1])
            t_b.append(timed(c2_search)[1])
        out["control"] = {"ms": [med(t_a), med(t_b)], "ratio": round(med(t_a) / med(t_b), 5),
                          "round_ratio_min_max": [round(min(x / y for x, y in zip(t_a, t_b)), 5),
                                                  round(max(x / y for x, y in zip(t_a, t_b)), 5)]}

        t_c2, t_scan, t_gen = [], [], []
        for _ in range(a.rounds):
            t_c2.append(timed(c2_search)[1])
            t_scan.append(timed(scan)[1])
            t_gen.append(timed(genesis)[1])
        c2_ghs, scan_ghs = n / med(t_c2) / 1e6, n / med(t_scan) / 1e6
        out["scan"] = {"c2_ms": med(t_c2), "c2_GHs": round(c2_ghs, 3), "ms": med(t_scan), "GHs": round(scan_ghs, 3),
                       "ms_all": [round(x, 3) for x in t_scan], "c2_ms_all": [round(x, 3) for x in t_c2]}
        if a.ops:
            pred = c2_ghs * C2_OPS / a.ops
            out["scan"].update(predicted_GHs=round(pred, 3), measured_over_predicted=round(scan_ghs / pred, 4))
        ideal = g["nonce"] / scan_ghs / 1e6
        out["genesis"] = {"ms": med(t_gen), "ideal_ms": round(ideal, 3), "ratio": round(med(t_gen) / ideal, 4),
                          "ms_all": [round(x, 3) for x in t_gen]}
        genesis()
        out["genesis"]["dispatched"] = ctx.last_target_stats().nonces_dispatched

        if a.lib:
            out["libs"] = {}
            others = [(p, Context(devices=[0], lib_path=p)) for p in a.lib]
            try:
                for _, c in others:
                    for _ in range(a.warmup):
                        assert scan(c) == best
                rows = {p: [] for p, _ in others}
                base = []
                for _ in range(a.rounds):
                    base.append(timed(scan)[1])
                    for p, c in others:
                        rows[p].append(timed(lambda: scan(c))[1])
                out["libs"]["this"] = {"ms": med(base), "GHs": round(n / med(base) / 1e6, 3)}
                for p, xs in rows.items():
                    out["libs"][os.path.basename(p)] = {
                        "ms": med(xs), "GHs": round(n / med(xs) / 1e6, 3), "ratio_to_this": round(med(base) / med(xs), 5),
                        "round_ratio_min_max": [round(min(b / x for b, x in zip(base, xs)), 5),
                                                round(max(b / x for b, x in zip(base, xs)), 5)]}
            finally:
                for _, c in others:
                    c.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
