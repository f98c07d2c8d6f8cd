#!/usr/bin/env python3
"""Measure bm_search_header_hits_gpu on one GPU (DESIGN.md section 4,
"Block-header share enumeration"): medians of --rounds rounds after --warmup, the variants
of a comparison alternating inside each round (their order reversed every
second round), in one process.

  control     search_header at target 0 against itself over [0, 2^32-1]: the
              per-round ratio range is the noise band for everything below
  sparse      search_header_hits at 32 and 24 zero bits against search_header
              at target 0 (both full scans)
  density     16, 12 and 8 zero bits, with entries and in count mode (a range
              that keeps the count below BM_MAX_HEADER_HITS, and the full range)
  walk        at 16 zero bits: one enumeration call against search_header
              called from hit to hit (--walk-bits: over [0, 2^B-1], once)
  back2back   four consecutive calls over [0, 2^32-1] with ntime rolled against
              four times the single call's median
  parent      (--parent-lib) bm_search_header_gpu, bm_search_gpu (C2) and
              bm_search_header_hits_gpu (32, 24, 16, 12 zero bits) of this
              tree's library against another build's, alternating

Writes profiles/header_hits/bench_header_hits.json and README.md (and
ab_parent.log with --parent-lib; --only-parent: ab_parent.log and
ab_parent.json alone)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distributed_bitcoin_minter_amd import _lib  # noqa: E402
from distributed_bitcoin_minter_amd.header_shares import with_ntime, header_ntime  # noqa: E402

GENESIS = bytes.fromhex("0100000000000000000000000000000000000000000000000000000000000000000000003ba3edfd7a7b12b27ac72c3e"
                        "67768f617fc81bc3888a51323a9fb8aa4b1e5e4a29ab5f49ffff001d1dac2b7c")
U32 = (1 << 32) - 1
OUT = os.path.join(ROOT, "profiles", "header_hits")
HITS_AB_BITS = (32, 24, 16, 12)  # the parent A/B of bm_search_header_hits_gpu: zero bits of its targets


def zero_bits(z):
    return (1 << (256 - z)) - 1


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def alternate(variants, rounds, warmup):
    """variants: {name: callable}.  Per-round times (ms) of each, the variants
    run one after the other inside every round, in reverse order in every
    second round (what runs right before a call is then the same for all on
    average)."""
    ms = {k: [] for k in variants}
    last = {}
    for r in range(warmup + rounds):
        for k, f in (list(variants.items()) if r % 2 == 0 else reversed(list(variants.items()))):
            t, last[k] = timed(f)
            if r >= warmup:
                ms[k].append(t)
    return ms, last


def summary(ms):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def ratios(ms, a, b):
    """Per-round a / b: (median, min, max)."""
    r = [x / y for x, y in zip(ms[a], ms[b])]
    return {"median": statistics.median(r), "min": min(r), "max": max(r)}


class RawLib:
    """Another build's bm_search_header_gpu / bm_search_gpu through plain
    ctypes (it need not export this tree's newer entry points)."""

    def __init__(self, path):
        lib = ctypes.CDLL(path, mode=os.RTLD_NOW | os.RTLD_LOCAL)
        vp, P = ctypes.c_void_p, ctypes.POINTER
        lib.bm_ctx_create.argtypes = [ctypes.c_int, P(vp)]
        lib.bm_ctx_destroy.argtypes = [vp]
        lib.bm_search_gpu.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64,
                                      P(_lib.Result)]
        lib.bm_search_header_gpu.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p,
                                             P(_lib.HeaderResult)]
        lib.bm_search_header_hits_gpu.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p,
                                                  P(_lib.HeaderHit), ctypes.c_size_t, P(_lib.HeaderHitsResult)]
        self.lib, self.h = lib, vp()
        self.buf = (_lib.HeaderHit * _lib.BM_MAX_HEADER_HITS)()
        _lib.check(lib.bm_ctx_create(1, ctypes.byref(self.h)), "bm_ctx_create")

    def search(self, msg, lo, hi):
        r = _lib.Result()
        _lib.check(self.lib.bm_search_gpu(self.h, msg, len(msg), lo, hi, ctypes.byref(r)), "bm_search_gpu")
        return r.hash, r.nonce

    def search_header(self, header, lo, hi, target):
        r = _lib.HeaderResult()
        _lib.check(self.lib.bm_search_header_gpu(self.h, header, lo, hi, target.to_bytes(32, "big"), ctypes.byref(r)),
                   "bm_search_header_gpu")
        return bool(r.found), int.from_bytes(bytes(r.hash), "big"), r.nonce

    def hits(self, header, lo, hi, target):
        """(count, stored, best share, the first and the last entry)."""
        r = _lib.HeaderHitsResult()
        _lib.check(self.lib.bm_search_header_hits_gpu(self.h, header, lo, hi, target.to_bytes(32, "big"), self.buf,
                                                      len(self.buf), ctypes.byref(r)), "bm_search_header_hits_gpu")
        ends = [(bytes(self.buf[i].hash), self.buf[i].nonce) for i in ((0, r.stored - 1) if r.stored else ())]
        return r.count, r.stored, (int.from_bytes(bytes(r.hash), "big"), r.nonce), ends

    def close(self):
        self.lib.bm_ctx_destroy(self.h)


def parent_ab(a, ctx, header0, res):
    """Unchanged paths, this tree's library (ctx) against --parent-lib's; fills
    res["parent"] and writes ab_parent.log."""
    full = (0, U32)
    if not a.parent_lib:
        return 0
    old = RawLib(a.parent_lib)
    try:
        msg = b"bradfitz"
        ms, last = alternate({"header_new": header0, "header_parent": lambda: old.search_header(GENESIS, *full, 0),
                              "c2_new": lambda: ctx.search(msg, *full),
                              "c2_parent": lambda: old.search(msg, *full)}, a.rounds, a.warmup)
        assert last["header_new"] == last["header_parent"] and last["c2_new"] == last["c2_parent"]
        res["parent"] = dict(summary(ms), ratio_header=ratios(ms, "header_new", "header_parent"),
                             ratio_c2=ratios(ms, "c2_new", "c2_parent"))
        # bm_search_header_hits_gpu, both libraries through the same plain ctypes
        # path: the sparse full scans, and the entry path over the density rows' ranges
        new = RawLib(os.path.join(ROOT, "distributed_bitcoin_minter_amd", "libbtcminer.so"))
        try:
            for z in HITS_AB_BITS:
                hi = min(U32, (1 << (19 + z)) - 1)
                ms, last = alternate({"new": lambda: new.hits(GENESIS, 0, hi, zero_bits(z)),
                                      "parent": lambda: old.hits(GENESIS, 0, hi, zero_bits(z))}, a.rounds, a.warmup)
                assert last["new"] == last["parent"], z
                s = summary(ms)
                res["parent"].update({f"hits_{z}_new": s["new"], f"hits_{z}_parent": s["parent"],
                                      f"ratio_hits_{z}": ratios(ms, "new", "parent"),
                                      f"hits_{z}_range": [0, hi], f"hits_{z}_count": last["new"][0]})
        finally:
            new.close()
    finally:
        old.close()
    with open(os.path.join(a.out, "ab_parent.log"), "w") as f:
        f.write("this tree's library against the parent commit's, alternating in one process, "
                f"{a.rounds} rounds after {a.warmup} warm-up; per-round new / parent\n")
        for k in ("header", "c2") + tuple(f"hits_{z}" for z in HITS_AB_BITS):
            r = res["parent"]["ratio_" + k]
            f.write(f"{k}: new {res['parent'][k + '_new']['median_ms']:.2f} ms, parent "
                    f"{res['parent'][k + '_parent']['median_ms']:.2f} ms, ratio median {r['median']:.4f} "
                    f"[{r['min']:.4f}, {r['max']:.4f}]\n")
        c = res["control"]["ratio"]
        f.write(f"control (search_header against itself): ratio median {c['median']:.4f} "
                f"[{c['min']:.4f}, {c['max']:.4f}]\n")
    print("parent", json.dumps(res["parent"]), flush=True)
    if a.only_parent:
        with open(os.path.join(a.out, "ab_parent.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--walk-bits", type=int, default=32, help="the walk covers [0, 2^B-1] (0: skip it)")
    ap.add_argument("--parent-lib", default=None, help="libbtcminer.so of the parent commit, for the A/B")
    ap.add_argument("--only-parent", action="store_true", help="the control and the parent A/B only")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = {"rounds": a.rounds, "warmup": a.warmup, "header": "genesis"}
    cap = _lib.BM_MAX_HEADER_HITS

    with _lib.Context(num_gpus=1) as ctx:
        full = (0, U32)

        def header0():
            return ctx.search_header(GENESIS, *full, 0)

        # the library call alone, into one buffer made once: (count, stored, best share)
        buf = (_lib.HeaderHit * cap)()

        def hits(header, lo, hi, target, c=cap):
            r = _lib.HeaderHitsResult()
            _lib.check(ctx._lib.bm_search_header_hits_gpu(ctx.handle, header, lo, hi, target.to_bytes(32, "big"),
                                                          buf if c else None, c, ctypes.byref(r)),
                       "bm_search_header_hits_gpu")
            return r.count, r.stored, (int.from_bytes(bytes(r.hash), "big"), r.nonce)

        # control
        ms, _ = alternate({"a": header0, "b": header0}, a.rounds, a.warmup)
        res["control"] = dict(summary(ms), ratio=ratios(ms, "a", "b"))
        print("control", json.dumps(res["control"]), flush=True)

        # sparse cost
        if a.only_parent:
            return parent_ab(a, ctx, header0, res)
        ms, last = alternate({"header_t0": header0,
                              "hits_32": lambda: hits(GENESIS, *full, zero_bits(32)),
                              "hits_24": lambda: hits(GENESIS, *full, zero_bits(24))},
                             a.rounds, a.warmup)
        res["sparse"] = dict(summary(ms), ratio_32=ratios(ms, "hits_32", "header_t0"),
                             ratio_24=ratios(ms, "hits_24", "header_t0"),
                             count_32=last["hits_32"][0], count_24=last["hits_24"][0])
        assert last["hits_32"][2] == last["hits_24"][2] == last["header_t0"][1:]
        print("sparse", json.dumps(res["sparse"]), flush=True)

        # density: a range that keeps about 2^19 hits, and the full range
        res["density"] = []
        for z in (16, 12, 8):
            for hi in sorted({min(U32, (1 << (19 + z)) - 1), U32}):
                ms, last = alternate({"header_t0": lambda: ctx.search_header(GENESIS, 0, hi, 0),
                                      "entries": lambda: hits(GENESIS, 0, hi, zero_bits(z)),
                                      "count_mode": lambda: hits(GENESIS, 0, hi, zero_bits(z), 0)},
                                     a.rounds, a.warmup)
                count, stored, _ = last["entries"]
                assert last["count_mode"][0] == count
                row = dict(summary(ms), zero_bits=z, nonce_hi=hi, count=count, stored=stored,
                           ratio_entries=ratios(ms, "entries", "header_t0"), ratio_count=ratios(ms, "count_mode", "header_t0"))
                res["density"].append(row)
                print("density", json.dumps(row), flush=True)

        # the walk it replaces
        if a.walk_bits > 0:
            hi, T = (1 << a.walk_bits) - 1, zero_bits(16)
            t_enum, (count, _, _) = timed(lambda: hits(GENESIS, 0, hi, T))
            listed = ctx.search_header_hits(GENESIS, 0, hi, T, cap)[1]

            def walk():
                got, lo = [], 0
                while lo <= hi:
                    found, h, n = ctx.search_header(GENESIS, lo, hi, T)
                    if not found:
                        break
                    got.append((h, n))
                    lo = n + 1
                return got

            t_walk, got = timed(walk)
            assert got == listed and len(got) == count
            res["walk"] = {"nonce_hi": hi, "hits": count, "enumeration_ms": t_enum, "walk_ms": t_walk,
                           "walk_calls": count + 1, "ratio": t_walk / t_enum, "rounds": 1}
            print("walk", json.dumps(res["walk"]), flush=True)

        # back to back: four headers (ntime rolled), one call each
        T = zero_bits(24)
        headers = [with_ntime(GENESIS, header_ntime(GENESIS) + r) for r in range(4)]

        def four():
            return [hits(h, *full, T)[0] for h in headers]

        ms, _ = alternate({"single": lambda: hits(GENESIS, *full, T), "four": four},
                          a.rounds, a.warmup)
        s = summary(ms)
        res["back_to_back"] = dict(s, four_over_4x_single=s["four"]["median_ms"] / (4 * s["single"]["median_ms"]))
        print("back_to_back", json.dumps(res["back_to_back"]), flush=True)

        parent_ab(a, ctx, header0, res)

    with open(os.path.join(a.out, "bench_header_hits.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    c = res["control"]["ratio"]
    lines = ["# bm_search_header_hits_gpu on one MI355X", "",
             f"`tools/bench_header_hits.py`: medians of {a.rounds} rounds after {a.warmup} warm-up, the variants of a "
             "comparison alternating in one process.  Raw figures: `bench_header_hits.json`.", "",
             f"* control, `search_header` at target 0 against itself over 2^32 nonces: "
             f"{res['control']['a']['median_ms']:.1f} ms, per-round ratio {c['median']:.4f} [{c['min']:.4f}, {c['max']:.4f}]"]
    for z in (32, 24):
        r = res["sparse"][f"ratio_{z}"]
        lines.append(f"* `search_header_hits` at {z} zero bits ({res['sparse'][f'count_{z}']} hits) over `search_header` "
                     f"at target 0: {r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]")
    for row in res["density"]:
        lines.append(f"* {row['zero_bits']} zero bits over [0, {row['nonce_hi']}]: {row['count']} hits, {row['stored']} "
                     f"stored; with entries {row['entries']['median_ms']:.1f} ms, {row['ratio_entries']['median']:.3f} of "
                     f"the header search's {row['header_t0']['median_ms']:.1f} ms; count mode "
                     f"{row['count_mode']['median_ms']:.1f} ms, "
                     f"{row['ratio_count']['median']:.3f}")
    if "walk" in res:
        w = res["walk"]
        lines.append(f"* the walk at 16 zero bits over [0, {w['nonce_hi']}]: {w['walk_calls']} `search_header` calls, "
                     f"{w['walk_ms'] / 1e3:.2f} s, against one enumeration call of {w['enumeration_ms']:.1f} ms: "
                     f"{w['ratio']:.0f} times (one round)")
    b = res["back_to_back"]
    lines.append(f"* four calls back to back (ntime rolled, 24 zero bits): {b['four']['median_ms']:.1f} ms, "
                 f"{b['four_over_4x_single']:.4f} of four times the single call's {b['single']['median_ms']:.1f} ms")
    if "parent" in res:
        for k in ("header", "c2"):
            r = res["parent"]["ratio_" + k]
            lines.append(f"* unchanged path `{k}`, this tree over the parent commit: {r['median']:.4f} "
                         f"[{r['min']:.4f}, {r['max']:.4f}] (`ab_parent.log`)")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
