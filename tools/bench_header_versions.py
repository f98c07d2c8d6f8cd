#!/usr/bin/env python3
"""Measure bm_search_header_versions_gpu on one GPU (DESIGN.md section 4,
"Version rolling"): medians of --rounds rounds after --warmup, the variants
alternating inside each round (their order reversed every second round).

  scan     the genesis header under 4 rolled versions, target 0 (a full scan of
           [0, 2^32-1] for each):
             four     four back-to-back search_header calls, one per version
                      (the parent's code path: the baseline)
             four_b   the same again: the control, its per-round ratio to
                      `four` is the noise band
             cap1/2/4 one search_header_versions call under each group cap
  found    the same at the header's own bits (early exit)
  parent   (--parent-lib) bm_search_header_gpu and bm_search_gpu (C2) of this
           tree's library against another build's, alternating

The group cap is read when a context is made, so each cap has a context of its
own, all in this one process.  Writes profiles/header_versions/
bench_header_versions.json and README.md (and ab_parent.log with --parent-lib)."""
import argparse
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from distributed_bitcoin_minter_amd import _lib  # noqa: E402
from bench_header_hits import GENESIS, U32, RawLib, alternate, ratios, summary  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "header_versions")
CAPS = (1, 2, 4)


def with_version(header, v):
    return struct.pack("<I", v) + header[4:]


def context_with_cap(cap):
    old = os.environ.get("BTCMINER_HEADER_GROUP")
    os.environ["BTCMINER_HEADER_GROUP"] = str(cap)
    try:
        return _lib.Context(num_gpus=1)
    finally:
        if old is None:
            del os.environ["BTCMINER_HEADER_GROUP"]
        else:
            os.environ["BTCMINER_HEADER_GROUP"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nver", type=int, default=4)
    ap.add_argument("--parent-lib", default=None, help="libbtcminer.so of the parent commit, for the A/B")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    versions = _lib.roll_versions(int.from_bytes(GENESIS[:4], "little"), a.nver)
    headers = [with_version(GENESIS, v) for v in versions]
    own_target = _lib.bits_to_target(int.from_bytes(GENESIS[72:76], "little"))
    full = (0, U32)
    res = {"rounds": a.rounds, "warmup": a.warmup, "header": "genesis", "versions": versions}
    ctxs = {cap: context_with_cap(cap) for cap in CAPS}
    base = ctxs[4]
    try:
        def four(target):
            """One search_header per version; the answer a versions call must give."""
            got = [base.search_header(h, *full, target) for h in headers]
            if any(f for f, _, _ in got):
                n, i = min((n, i) for i, (f, _, n) in enumerate(got) if f)
                return True, got[i][1], n, i
            _, n, i = min((h >> 192, n, i) for i, (_, h, n) in enumerate(got))
            return False, got[i][1], n, i

        for name, target in (("scan", 0), ("found", own_target)):
            variants = {"four": lambda: four(target), "four_b": lambda: four(target)}
            for cap in CAPS:
                variants[f"cap{cap}"] = (lambda c: lambda: c.search_header_versions(GENESIS, versions, *full, target))(
                    ctxs[cap])
            ms, last = alternate(variants, a.rounds, a.warmup)
            assert all(last[k] == last["four"] for k in variants), last
            row = dict(summary(ms), control=ratios(ms, "four_b", "four"),
                       answer=[last["cap4"][0], last["cap4"][2], last["cap4"][3]])
            for cap in CAPS:
                row[f"ratio_cap{cap}"] = ratios(ms, f"cap{cap}", "four")
                if target == 0:
                    row[f"ghs_cap{cap}"] = a.nver * 2 ** 32 / row[f"cap{cap}"]["median_ms"] / 1e6
            if target == 0:
                row["ghs_four"] = a.nver * 2 ** 32 / row["four"]["median_ms"] / 1e6
            res[name] = row
            print(name, json.dumps(row), flush=True)

        if a.parent_lib:
            old = RawLib(a.parent_lib)
            try:
                msg = b"bradfitz"
                ms, last = alternate({"header_new": lambda: base.search_header(GENESIS, *full, 0),
                                      "header_parent": lambda: old.search_header(GENESIS, *full, 0),
                                      "c2_new": lambda: base.search(msg, *full),
                                      "c2_parent": lambda: old.search(msg, *full)}, a.rounds, a.warmup)
                assert last["header_new"] == last["header_parent"] and last["c2_new"] == last["c2_parent"]
                res["parent"] = dict(summary(ms), ratio_header=ratios(ms, "header_new", "header_parent"),
                                     ratio_c2=ratios(ms, "c2_new", "c2_parent"))
            finally:
                old.close()
            with open(os.path.join(a.out, "ab_parent.log"), "w") as f:
                f.write("this tree's library against the parent commit's, alternating in one process, "
                        f"{a.rounds} rounds after {a.warmup} warm-up; per-round new / parent\n")
                for k in ("header", "c2"):
                    r = res["parent"]["ratio_" + k]
                    f.write(f"{k}: new {res['parent'][k + '_new']['median_ms']:.2f} ms, parent "
                            f"{res['parent'][k + '_parent']['median_ms']:.2f} ms, ratio median {r['median']:.4f} "
                            f"[{r['min']:.4f}, {r['max']:.4f}]\n")
            print("parent", json.dumps(res["parent"]), flush=True)
    finally:
        for c in ctxs.values():
            c.close()

    with open(os.path.join(a.out, "bench_header_versions.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    lines = ["# header_versions_kernel on one MI355X", "",
             f"`tools/bench_header_versions.py`: the genesis header under {a.nver} rolled versions over [0, 2^32-1]; "
             f"medians of {a.rounds} rounds after {a.warmup} warm-up, the variants alternating in one process.  A ratio "
             "is per round, time over the time of four back-to-back `search_header` calls (below 1: faster).  Raw "
             "figures: `bench_header_versions.json`.", ""]
    for name, what in (("scan", "target 0, a full scan"), ("found", "the header's own bits")):
        row = res[name]
        c = row["control"]
        lines.append(f"* {what}: four `search_header` calls {row['four']['median_ms']:.1f} ms"
                     + (f" ({row['ghs_four']:.2f} GH/s)" if "ghs_four" in row else "")
                     + f"; control ratio {c['median']:.4f} [{c['min']:.4f}, {c['max']:.4f}]")
        for cap in CAPS:
            r = row[f"ratio_cap{cap}"]
            lines.append(f"  * one versions call, group cap {cap}: {row[f'cap{cap}']['median_ms']:.1f} ms"
                         + (f" ({row[f'ghs_cap{cap}']:.2f} GH/s)" if f"ghs_cap{cap}" in row else "")
                         + f", ratio {r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]")
    if "parent" in res:
        for k in ("header", "c2"):
            r = res["parent"]["ratio_" + k]
            lines.append(f"* unchanged path `{k}`, this tree over the parent commit: {r['median']:.4f} "
                         f"[{r['min']:.4f}, {r['max']:.4f}] (`ab_parent.log`)")
    lines.append("* not measured: the shader clock, PMC counters, more than one GPU")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
