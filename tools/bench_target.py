#!/usr/bin/env python3
"""Measure the target search (bm_search_target_gpu) on one GPU.

    python tools/bench_target.py [--rounds 10] [--warmup 2] [--out profiles/target/bench_target.json]

Prints one JSON object:
  notfound_ratio  C2 ("bradfitz", [0, 2^32-1]) with T = min - 1 (nothing to
                  find, the whole range is scanned) through search_target,
                  against search on the same context, alternating: the median
                  rate of each (GH/s, host wall time) and their ratio.  The
                  inner loops are the same instruction stream; read the ratio
                  against the ~0.3% A/B noise of an unchanged control
                  (profiles/r06/ab_nbv2_tight.log).
  found_c2_ms     C2 with T = the minimum: wall and span time and the nonces
                  dispatched, next to the full scan's time from the same run
                  and the ideal, 0.379 x that time (the hit's place in the range).
  easy_ms         targets of 16, 24 and 32 leading zero bits from lower = 0, in steps of
                  2^32 nonces as the pow CLI takes them:
                  time to the first hit and nonces dispatched (the per-call floor).
Every answer is checked against the committed golden / the library's own
bm_hash_gpu.  No torch."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def pow_search(ctx, msg, T, step=1 << 32):
    """As the pow CLI: one target search per 2^32 nonces from 0 until the
    first hit -> (result, ms, nonces dispatched over the steps)."""
    lo, ms, disp = 0, 0.0, 0
    while True:
        r, t = timed(lambda: ctx.search_target(msg, lo, lo + step - 1, T))
        ms += t
        disp += ctx.last_target_stats().nonces_dispatched
        if r[0]:
            return r, ms, disp
        lo += step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    from distributed_bitcoin_minter_amd import Context
    c2 = next(c for c in json.load(open(os.path.join(ROOT, "tests/golden/full_range.json")))["cases"]
              if c["config"] == "C2")
    msg, lo, hi = bytes.fromhex(c2["msg_hex"]), c2["lower"], c2["upper"]
    gold = (c2["hash"], c2["nonce"])
    n = hi - lo + 1
    out = {"tool": "bench_target", "config": "C2", "rounds": a.rounds, "warmup": a.warmup}
    with Context(devices=[0]) as ctx:
        ctx.set_timing(True)
        for _ in range(a.warmup):
            assert ctx.search(msg, lo, hi) == gold
            assert ctx.search_target(msg, lo, hi, gold[0] - 1) == (False,) + gold

        # not found: the same scan through both entry points, alternating
        t_search, t_target = [], []
        for _ in range(a.rounds):
            r, ms = timed(lambda: ctx.search(msg, lo, hi))
            assert r == gold
            t_search.append(ms)
            r, ms = timed(lambda: ctx.search_target(msg, lo, hi, gold[0] - 1))
            assert r == (False,) + gold and ctx.last_target_stats().nonces_dispatched == n
            t_target.append(ms)
        ms_s, ms_t = statistics.median(t_search), statistics.median(t_target)
        out["notfound_ratio"] = {
            "search_GHs": round(n / ms_s / 1e6, 3), "target_GHs": round(n / ms_t / 1e6, 3),
            "ratio": round(ms_s / ms_t, 5), "search_ms": [round(x, 3) for x in t_search],
            "target_ms": [round(x, 3) for x in t_target]}

        # found at 0.379 of the range
        walls, spans, disp = [], [], []
        for _ in range(a.rounds):
            r, ms = timed(lambda: ctx.search_target(msg, lo, hi, gold[0]))
            assert r == (True,) + gold
            walls.append(ms)
            spans.append(ctx.last_stats().span_ms)
            disp.append(ctx.last_target_stats().nonces_dispatched)
        frac = (gold[1] - lo + 1) / n
        out["found_c2_ms"] = {
            "wall_ms": round(statistics.median(walls), 3), "span_ms": round(statistics.median(spans), 3),
            "nonces_dispatched": int(statistics.median(disp)), "dispatched_min_max": [min(disp), max(disp)],
            "hit_fraction": round(frac, 4), "full_scan_ms": round(ms_s, 3), "ideal_ms": round(frac * ms_s, 3)}

        # easy targets: the per-call floor
        easy = {}
        for bits in (16, 24, 32):
            T = (1 << (64 - bits)) - 1
            ts, ds, ans = [], [], None
            for _ in range(a.rounds):
                r, ms, d = pow_search(ctx, msg, T)
                assert r[0] and r[1] <= T and ctx.hash_many(msg, [r[2]]) == [r[1]] and (ans is None or ans == r)
                ans = r
                ts.append(ms)
                ds.append(d)
            easy[str(bits)] = {"ms": round(statistics.median(ts), 3), "nonce": ans[2], "hash": ans[1],
                               "nonces_dispatched": int(statistics.median(ds))}
        out["easy_ms"] = easy
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
