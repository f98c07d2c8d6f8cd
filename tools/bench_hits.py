#!/usr/bin/env python3
"""Measure the hit enumeration (bm_search_hits_gpu) on one GPU.

    python tools/bench_hits.py [--rounds 10] [--warmup 2] [--out profiles/hits/bench_hits.json]

C2 ("bradfitz", [0, 2^32-1]) on one context, medians of host wall time.
Prints one JSON object:
  control   search against search, alternating: the run's own A/B noise
            (ratio of the medians, and the spread of the per-round ratios).
  sparse    search_hits at 32 and 24 leading zero bits (about 1 and 256 hits)
            against search, alternating: the same scan plus the rare hits, so
            the ratio should sit within the control's noise.
  density   16, 12 and 10 zero bits: time, count and the ratio to search.
            Every hit is one atomic on one word, so dense targets are bound by
            that atomic, not by hashing; 10 bits is where this
            tool stops.
  walk      16 bits: one search_hits call against the walk it replaces, one
            search_target call per hit from the previous hit + 1 (one round).
Every minimum is checked against the committed golden, every list against the
library's own bm_hash_gpu (and the 16-bit list against the walk).  The timed
calls go through the C ABI with a buffer made beforehand, so no Python list
building is timed.  No torch."""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    from distributed_bitcoin_minter_amd import Context, _lib
    c2 = next(c for c in json.load(open(os.path.join(ROOT, "tests/golden/full_range.json")))["cases"]
              if c["config"] == "C2")
    msg, lo, hi = bytes.fromhex(c2["msg_hex"]), c2["lower"], c2["upper"]
    gold = (c2["hash"], c2["nonce"])
    n = hi - lo + 1
    cap = _lib.BM_MAX_HITS
    buf = (_lib.Result * cap)()
    out = {"tool": "bench_hits", "config": "C2", "rounds": a.rounds, "warmup": a.warmup, "cap": cap}

    def target(bits):
        return (1 << (64 - bits)) - 1

    with Context(devices=[0]) as ctx:
        lib, h = ctx._lib, ctx.handle

        def hits(T, use_cap=cap):
            r = _lib.HitsResult()
            _lib.check(lib.bm_search_hits_gpu(h, msg, len(msg), lo, hi, T, buf if use_cap else None, use_cap,
                                              ctypes.byref(r)), "bm_search_hits_gpu")
            assert (r.hash, r.nonce) == gold
            return r.count, r.stored

        def search():
            assert ctx.search(msg, lo, hi) == gold

        def verify(count, stored, T):
            """The stored entries: ascending, each hash the library's own and <= T."""
            assert stored in (0, count)
            step = max(1, stored // 4096)  # a sample of a long list, all of a short one
            idx = list(range(0, stored, step))
            nonces = [buf[i].nonce for i in idx]
            assert ctx.hash_many(msg, nonces) == [buf[i].hash for i in idx]
            assert all(buf[i].hash <= T for i in idx)
            assert all(buf[i].nonce < buf[i + 1].nonce for i in range(0, stored - 1, step))

        def against_search(f):
            """f and search, alternating -> medians, ratio and the per-round ratios' spread."""
            t_s, t_f, last = [], [], None
            for _ in range(a.rounds):
                _, ms = timed(search)
                t_s.append(ms)
                last, ms = timed(f)
                t_f.append(ms)
            ms_s, ms_f = statistics.median(t_s), statistics.median(t_f)
            per_round = [s / x for s, x in zip(t_s, t_f)]
            return last, {"search_ms": round(ms_s, 3), "ms": round(ms_f, 3), "search_GHs": round(n / ms_s / 1e6, 3),
                          "GHs": round(n / ms_f / 1e6, 3), "ratio": round(ms_s / ms_f, 5),
                          "round_ratio_min_max": [round(min(per_round), 5), round(max(per_round), 5)],
                          "search_ms_all": [round(x, 3) for x in t_s], "ms_all": [round(x, 3) for x in t_f]}

        for _ in range(a.warmup):
            search()
            hits(target(32))

        _, out["control"] = against_search(search)

        out["sparse"] = {}
        for bits in (32, 24):
            (count, stored), row = against_search(lambda: hits(target(bits)))
            verify(count, stored, target(bits))
            out["sparse"][str(bits)] = dict(row, count=count, stored=stored)

        out["density"] = {}
        for bits in (16, 12, 10):
            (count, stored), row = against_search(lambda: hits(target(bits)))
            verify(count, stored, target(bits))
            (count0, _), ms0 = timed(lambda: hits(target(bits), 0))
            assert count0 == count
            out["density"][str(bits)] = dict(row, count=count, stored=stored, count_only_ms=round(ms0, 3),
                                             hits_per_s=round(count / row["ms"] * 1e3))

        # the walk a hits call replaces: one target search per hit
        T = target(16)
        (count, stored), ms_one = timed(lambda: hits(T))
        assert stored == count
        listed = [(buf[i].hash, buf[i].nonce) for i in range(stored)]

        def walk():
            got, at = [], lo
            while at <= hi:
                found, hh, nn = ctx.search_target(msg, at, hi, T)
                if not found:
                    break
                got.append((hh, nn))
                at = nn + 1
            return got
        walked, ms_walk = timed(walk)
        assert walked == listed
        out["walk"] = {"bits": 16, "hits": count, "hits_call_ms": round(ms_one, 3), "walk_ms": round(ms_walk, 1),
                       "walk_calls": len(walked) + 1, "walk_ms_per_call": round(ms_walk / (len(walked) + 1), 4)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
