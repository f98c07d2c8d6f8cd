#!/usr/bin/env python3
"""Measure bm_search_job_shares_gpu on one GPU ("Stratum
jobs"): medians of --rounds rounds after --warmup, the variants alternating
inside each round (their order reversed every second round).  The genesis job
(tests/golden/stratum_genesis_job.json) under 4 extranonce2 values x 4 rolled
versions over [0, 2^32-1] at 32 zero bits throughout.

  job              one bm_search_job_shares_gpu call over the 4 extranonce2 values
  direct/direct_b  the same 4 headers (built beforehand) through 4
                   bm_search_header_versions_hits_gpu calls: what a caller of the
                   parent commit does, the yardstick; direct_b is the control: its
                   per-round ratio to direct is the noise band
  host             bm_job_header alone, per header (through ctypes, so an upper
                   bound): the one piece of host work the job call adds per
                   header besides the merge, which is the residual of job - direct

Every call is timed through the C ABI into a buffer allocated once.  Writes
profiles/job/bench_job.json and README.md."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from distributed_bitcoin_minter_amd import Context, Job, _lib  # noqa: E402
from bench_header_hits import U32, alternate, ratios, summary, zero_bits  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "job")
NVER = 4
EN2 = (28, 31)
ZBITS = 32
CAP = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(ROOT, "tests", "golden", "stratum_genesis_job.json")) as f:
        spec = json.load(f)
    job = Job.from_notify(spec["notify"], spec["extranonce1"], spec["extranonce2_size"])
    versions = _lib.roll_versions(job.version, NVER)
    arr = (ctypes.c_uint32 * NVER)(*versions)
    target = zero_bits(ZBITS).to_bytes(32, "big")
    headers = [job.header(e) for e in range(EN2[0], EN2[1] + 1)]
    nheaders = len(headers)
    pairs = nheaders * NVER * 2 ** 32
    job_buf = (_lib.JobShare * CAP)()
    hit_buf = (_lib.HeaderVersionHit * CAP)()

    with Context(num_gpus=1) as ctx:
        def job_call():
            r = _lib.JobSharesResult()
            _lib.check(ctx._lib.bm_search_job_shares_gpu(ctx.handle, ctypes.byref(job.struct), job.ntime, *EN2, arr, NVER,
                                                         0, U32, target, job_buf, CAP, ctypes.byref(r)),
                       "bm_search_job_shares_gpu")
            shares = [(int.from_bytes(bytes(s.hash), "big"), s.extranonce2, s.nonce, s.version_index)
                      for s in job_buf[:r.stored]]
            return r.count, shares, (int.from_bytes(bytes(r.hash), "big"), r.extranonce2, r.nonce, r.version_index)

        def direct():
            count, shares, bests = 0, [], []
            for e, header in zip(range(EN2[0], EN2[1] + 1), headers):
                r = _lib.HeaderVersionsHitsResult()
                _lib.check(ctx._lib.bm_search_header_versions_hits_gpu(ctx.handle, header, arr, NVER, 0, U32, target,
                                                                       hit_buf, CAP, ctypes.byref(r)),
                           "bm_search_header_versions_hits_gpu")
                count += r.count
                shares += [(int.from_bytes(bytes(s.hash), "big"), e, s.nonce, s.version_index) for s in hit_buf[:r.stored]]
                bests.append((int.from_bytes(bytes(r.hash), "big"), e, r.nonce, r.version_index))
            return count, shares, min(bests, key=lambda s: (s[0] >> 192, s[1], s[2], s[3]))

        ms, last = alternate({"job": job_call, "direct": direct, "direct_b": direct}, a.rounds, a.warmup)
        assert last["job"] == last["direct"] == last["direct_b"], last

    # the host's header build alone (pure CPU)
    out = (ctypes.c_uint8 * 80)()
    f = _lib.load().bm_job_header
    reps = 20000
    t = time.perf_counter()
    for k in range(reps):
        f(ctypes.byref(job.struct), EN2[0] + k % nheaders, job.ntime, job.version, out)
    header_us = (time.perf_counter() - t) * 1e6 / reps

    row = dict(summary(ms), control=ratios(ms, "direct_b", "direct"), ratio_job_direct=ratios(ms, "job", "direct"),
               count=last["job"][0], headers=nheaders, versions=versions, header_build_us=header_us)
    for k in ("job", "direct"):
        row[f"ghs_{k}"] = pairs / row[k]["median_ms"] / 1e6
    row["excess_ms"] = row["job"]["median_ms"] - row["direct"]["median_ms"]
    res = {"rounds": a.rounds, "warmup": a.warmup, "job": "genesis", "extranonce2": list(EN2), "zero_bits": ZBITS,
           "result": row}
    with open(os.path.join(a.out, "bench_job.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")

    def band(r):
        return f"{r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]"

    inside = row["control"]["min"] <= row["ratio_job_direct"]["median"] <= row["control"]["max"]
    lines = ["# bm_search_job_shares_gpu on one MI355X", "",
             f"`tools/bench_job.py`: the genesis job under extranonce2 {EN2[0]}..{EN2[1]} x {NVER} rolled versions over "
             f"[0, 2^32-1] at {ZBITS} zero bits ({row['count']} shares); medians of {a.rounds} rounds after {a.warmup} "
             "warm-up, the variants alternating in one process.  A ratio is per round (below 1: faster), given as "
             "median [min, max].  Raw figures: `bench_job.json`.", "",
             f"* one job call: {row['job']['median_ms']:.1f} ms ({row['ghs_job']:.2f} GH/s)",
             f"* the same {nheaders} headers through {nheaders} `bm_search_header_versions_hits_gpu` calls: "
             f"{row['direct']['median_ms']:.1f} ms ({row['ghs_direct']:.2f} GH/s); control ratio {band(row['control'])}",
             f"* the job call over the direct calls: {band(row['ratio_job_direct'])}: "
             + ("inside" if inside else "OUTSIDE") + " the control's band; median difference "
             f"{row['excess_ms']:+.3f} ms",
             f"* `bm_job_header` alone: {header_us:.2f} us per header through ctypes ({nheaders} per call); the merge "
             "is what is left of the difference",
             "* not measured: the shader clock, PMC counters, more than one GPU"]
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
