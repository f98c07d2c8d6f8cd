#!/usr/bin/env python3
"""Measure bm_search_header_versions_hits_gpu on one GPU (DESIGN.md section 4,
"Version-rolling share enumeration"): medians of --rounds rounds after
--warmup, the variants alternating inside each round (their order reversed
every second round).  The genesis header under 4 rolled versions over
[0, 2^32-1] throughout.

  sparse   references, each twice (the second is the control: its per-round
           ratio to the first is the noise band):
             scan / scan_b   search_header_versions at target 0, the full scan
                             of the first-hit kernel
             four / four_b   four search_header_hits calls at 32 zero bits, one
                             per version: what a caller does without this call
           and the new call at 32 and 24 zero bits (z32, z24)
  dense    the new call at 16 and 12 zero bits, storing (cap =
           BM_MAX_HEADER_HITS) and counting (cap = 0), beside scan: the host's
           per-hit cost.  A count above the cap stores nothing (all or nothing)
  caps     the new call at 24 zero bits under group caps 1, 2 and 4
  parent   (--parent-lib) bm_search_header_versions_gpu and bm_search_gpu (C2)
           of this tree's library against another build's, alternating

The new call is timed through the C ABI into a buffer allocated once, so the
figures hold the library's work and not the Python binding's list building.
Writes profiles/header_versions_hits/bench_header_versions_hits.json and
README.md (and ab_parent.log with --parent-lib)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from distributed_bitcoin_minter_amd import _lib  # noqa: E402
from bench_header_hits import GENESIS, U32, RawLib, alternate, ratios, summary, zero_bits  # noqa: E402
from bench_header_versions import CAPS, context_with_cap, with_version  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "header_versions_hits")
NVER = 4
PAIRS = NVER * 2 ** 32


class ParentLib(RawLib):
    """RawLib with the parent's bm_search_header_versions_gpu."""

    def __init__(self, path):
        super().__init__(path)
        vp, P, u32 = ctypes.c_void_p, ctypes.POINTER, ctypes.c_uint32
        self.lib.bm_search_header_versions_gpu.argtypes = [vp, ctypes.c_char_p, P(u32), ctypes.c_size_t, u32, u32,
                                                           ctypes.c_char_p, P(_lib.HeaderVersionsResult)]

    def search_header_versions(self, header, versions, lo, hi, target):
        r = _lib.HeaderVersionsResult()
        arr = (ctypes.c_uint32 * len(versions))(*versions)
        _lib.check(self.lib.bm_search_header_versions_gpu(self.h, header, arr, len(versions), lo, hi,
                                                          target.to_bytes(32, "big"), ctypes.byref(r)),
                   "bm_search_header_versions_gpu")
        return bool(r.found), int.from_bytes(bytes(r.hash), "big"), r.nonce, r.version_index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libbtcminer.so of the parent commit, for the A/B")
    ap.add_argument("--only-parent", action="store_true",
                    help="the parent A/B only, added to the figures --out already holds")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    versions = _lib.roll_versions(int.from_bytes(GENESIS[:4], "little"), NVER)
    headers = [with_version(GENESIS, v) for v in versions]
    full = (0, U32)
    res = {"rounds": a.rounds, "warmup": a.warmup, "header": "genesis", "versions": versions}
    if a.only_parent:
        with open(os.path.join(a.out, "bench_header_versions_hits.json")) as f:
            res = json.load(f)
    ctxs = {cap: context_with_cap(cap) for cap in CAPS}
    base = ctxs[4]
    max_cap = _lib.BM_MAX_HEADER_HITS
    buf = (_lib.HeaderVersionHit * max_cap)()
    arr = (ctypes.c_uint32 * NVER)(*versions)

    def new_call(ctx, z, cap):
        """(count, stored, best (hash, nonce, index), first and last stored (nonce, index))"""
        r = _lib.HeaderVersionsHitsResult()
        _lib.check(ctx._lib.bm_search_header_versions_hits_gpu(ctx.handle, GENESIS, arr, NVER, *full,
                                                               zero_bits(z).to_bytes(32, "big"), buf if cap else None,
                                                               cap, ctypes.byref(r)),
                   "bm_search_header_versions_hits_gpu")
        ends = [(buf[k].nonce, buf[k].version_index) for k in ((0, r.stored - 1) if r.stored else ())]
        return r.count, r.stored, (int.from_bytes(bytes(r.hash), "big"), r.nonce, r.version_index), ends

    def four(z):
        got = [base.search_header_hits(h, *full, zero_bits(z), 65536) for h in headers]
        return sum(c for c, _, _ in got), sorted((n, i) for i, (_, hits, _) in enumerate(got) for _, n in hits)

    try:
        scan = lambda: base.search_header_versions(GENESIS, versions, *full, 0)  # noqa: E731
        if not a.only_parent:
            # ---- sparse: parity with the first-hit kernel's full scan ----
            ms, last = alternate({"scan": scan, "scan_b": scan, "four": lambda: four(32), "four_b": lambda: four(32),
                                  "z32": lambda: new_call(base, 32, 65536), "z24": lambda: new_call(base, 24, 65536)},
                                 a.rounds, a.warmup)
            assert last["z32"][2] == last["z24"][2] == last["scan"][1:], last  # the best share is the target-0 answer
            assert last["z32"][0] == last["z32"][1] == last["four"][0] and last["z32"][3] == [last["four"][1][0],
                                                                                           last["four"][1][-1]]
            row = dict(summary(ms), control_scan=ratios(ms, "scan_b", "scan"), control_four=ratios(ms, "four_b", "four"),
                       counts={"z32": last["z32"][0], "z24": last["z24"][0]})
            for k in ("z32", "z24"):
                row[f"ratio_{k}_scan"] = ratios(ms, k, "scan")
                row[f"ratio_{k}_four"] = ratios(ms, k, "four")
            for k in ("scan", "four", "z32", "z24"):
                row[f"ghs_{k}"] = PAIRS / row[k]["median_ms"] / 1e6
            res["sparse"] = row
            print("sparse", json.dumps(row), flush=True)

            # ---- dense: the host's per-hit cost ----
            variants = {"scan": scan}
            for z in (16, 12):
                variants[f"z{z}_stored"] = (lambda z: lambda: new_call(base, z, max_cap))(z)
                variants[f"z{z}_count"] = (lambda z: lambda: new_call(base, z, 0))(z)
            ms, last = alternate(variants, a.rounds, a.warmup)
            row = dict(summary(ms))
            for z in (16, 12):
                st, ct = last[f"z{z}_stored"], last[f"z{z}_count"]
                assert st[0] == ct[0] and ct[1] == 0 and st[1] == (st[0] if st[0] <= max_cap else 0)
                row[f"z{z}"] = {"count": st[0], "stored": st[1], "ratio_stored_scan": ratios(ms, f"z{z}_stored", "scan"),
                                "ratio_count_scan": ratios(ms, f"z{z}_count", "scan")}
                if st[1]:
                    row[f"z{z}"]["us_per_stored_hit"] = (row[f"z{z}_stored"]["median_ms"] -
                                                         row[f"z{z}_count"]["median_ms"]) * 1e3 / st[1]
            res["dense"] = row
            print("dense", json.dumps(row), flush=True)

            # ---- group caps at 24 zero bits ----
            ms, last = alternate({f"cap{c}": (lambda x: lambda: new_call(x, 24, 65536))(ctxs[c]) for c in CAPS},
                                 a.rounds, a.warmup)
            assert all(last[f"cap{c}"] == last["cap4"] for c in CAPS)
            row = dict(summary(ms))
            for c in CAPS:
                row[f"ghs_cap{c}"] = PAIRS / row[f"cap{c}"]["median_ms"] / 1e6
                row[f"ratio_cap{c}"] = ratios(ms, f"cap{c}", "cap4")
            res["caps"] = row
            print("caps", json.dumps(row), flush=True)

        if a.parent_lib:
            old = ParentLib(a.parent_lib)
            try:
                msg = b"bradfitz"
                # a pair per pass: next to the 600 ms scans the 80 ms C2 call's time depends on which
                # of them ran right before it, which is not the same for the two libraries
                ms, last = alternate({"versions_new": scan,
                                      "versions_parent": lambda: old.search_header_versions(GENESIS, versions, *full, 0)},
                                     a.rounds, a.warmup)
                ms2, last2 = alternate({"c2_new": lambda: base.search(msg, *full),
                                        "c2_parent": lambda: old.search(msg, *full)}, a.rounds, a.warmup)
                ms.update(ms2)
                last.update(last2)
                assert last["versions_new"] == last["versions_parent"] and last["c2_new"] == last["c2_parent"]
                res["parent"] = dict(summary(ms), ratio_versions=ratios(ms, "versions_new", "versions_parent"),
                                     ratio_c2=ratios(ms, "c2_new", "c2_parent"))
            finally:
                old.close()
            with open(os.path.join(a.out, "ab_parent.log"), "w") as f:
                f.write("this tree's library against the parent commit's, alternating in one process, "
                        f"{a.rounds} rounds after {a.warmup} warm-up; per-round new / parent\n")
                for k in ("versions", "c2"):
                    r = res["parent"]["ratio_" + k]
                    f.write(f"{k}: new {res['parent'][k + '_new']['median_ms']:.2f} ms, parent "
                            f"{res['parent'][k + '_parent']['median_ms']:.2f} ms, ratio median {r['median']:.4f} "
                            f"[{r['min']:.4f}, {r['max']:.4f}]\n")
            print("parent", json.dumps(res["parent"]), flush=True)
    finally:
        for c in ctxs.values():
            c.close()

    with open(os.path.join(a.out, "bench_header_versions_hits.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")

    def band(r):
        return f"{r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]"

    s, d, c = res["sparse"], res["dense"], res["caps"]
    lines = ["# header_versions_hits_kernel on one MI355X", "",
             f"`tools/bench_header_versions_hits.py`: the genesis header under {NVER} rolled versions over [0, 2^32-1]; "
             f"medians of {a.rounds} rounds after {a.warmup} warm-up, the variants alternating in one process.  A ratio "
             "is per round (below 1: faster), given as median [min, max].  Raw figures: "
             "`bench_header_versions_hits.json`.", "",
             f"* `search_header_versions` at target 0 (the first-hit kernel's full scan): {s['scan']['median_ms']:.1f} ms "
             f"({s['ghs_scan']:.2f} GH/s); control ratio {band(s['control_scan'])}",
             f"* four `search_header_hits` calls at 32 zero bits: {s['four']['median_ms']:.1f} ms "
             f"({s['ghs_four']:.2f} GH/s); control ratio {band(s['control_four'])}"]
    for k in ("z32", "z24"):
        lines.append(f"* the new call at {k[1:]} zero bits ({s['counts'][k]} hits): {s[k]['median_ms']:.1f} ms "
                     f"({s['ghs_' + k]:.2f} GH/s); over the scan {band(s[f'ratio_{k}_scan'])}, over the four calls "
                     f"{band(s[f'ratio_{k}_four'])}")
    for z in (16, 12):
        r = d[f"z{z}"]
        lines.append(f"* {z} zero bits, {r['count']} hits, {r['stored']} stored: storing "
                     f"{d[f'z{z}_stored']['median_ms']:.1f} ms, over the scan {band(r['ratio_stored_scan'])}; counting "
                     f"{d[f'z{z}_count']['median_ms']:.1f} ms, over the scan {band(r['ratio_count_scan'])}"
                     + (f"; {r['us_per_stored_hit']:.3f} us per stored hit" if "us_per_stored_hit" in r else ""))
    for cap in CAPS:
        lines.append(f"* group cap {cap} at 24 zero bits: {c[f'cap{cap}']['median_ms']:.1f} ms "
                     f"({c[f'ghs_cap{cap}']:.2f} GH/s), over cap 4 {band(c[f'ratio_cap{cap}'])}")
    if "parent" in res:
        for k in ("versions", "c2"):
            lines.append(f"* unchanged path `{k}`, this tree over the parent commit: "
                         f"{band(res['parent']['ratio_' + k])} (`ab_parent.log`)")
    lines.append("* not measured: the shader clock, PMC counters, more than one GPU")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
