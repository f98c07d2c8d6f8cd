#!/usr/bin/env python3
"""Measure bm_jobs_verify_gpu on one GPU ("Share verification
over several jobs"), tools/bench_pool_verify.py's method and workload: medians of
--rounds rounds after --warmup, the variants alternating inside each round (their
order reversed every second round), every call through the C ABI into buffers
allocated once.  n = 2^17 random valid submissions over 2^12 sessions and J = 1, 8,
64 synthetic jobs (a 12-entry branch and a 250-byte coinbase each, all different),
the jobs assigned at random:

  jobs/jobs_b  (a) one bm_jobs_verify_gpu call; jobs_b is the control: its
               per-round ratio to jobs is the noise band
  per_job      (b) the parent's way: the submissions grouped by job beforehand,
               then J bm_pool_verify_gpu calls.  Only the calls are timed, which
               favours this variant
  pool         (c) at J = 1, bm_pool_verify_gpu on the same batch: what the grouping
               stage and the indirection cost when there is nothing to group
  set          (d) at J = 8, bm_share_set_verify_jobs on an empty 2^22 set (cleared
               before every call, outside the timer)

and, on the host alone (tools/jobs_verify_host_time.cpp, built here with g++), what
the grouping and the tripwire's per-job entries take at J = 64.  The verdict bytes
of (a), (b), (c) and (d) are compared every round.  Writes
profiles/jobs_verify/bench_jobs_verify.json and README.md."""
import argparse
import ctypes
import json
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from distributed_bitcoin_minter_amd import Context, Job, ShareSet, _lib  # noqa: E402
from bench_header_hits import ratios, summary, timed, zero_bits  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "jobs_verify")
N = 1 << 17
S = 1 << 12
JOBS = (1, 8, 64)
SET_J = 8
SET_CAPACITY = 1 << 22
ZBITS = 8
SIZE1, SIZE2 = 4, 8
SUBMIT = np.dtype([("extranonce2", "<u8"), ("ntime", "<u4"), ("nonce", "<u4"), ("version", "<u4"), ("session", "<u4")])
JOBS_SUBMIT = np.dtype([("extranonce2", "<u8"), ("ntime", "<u4"), ("nonce", "<u4"), ("version", "<u4"), ("session", "<u4"),
                        ("job", "<u4"), ("reserved", "<u4")])
SESSION = np.dtype([("extranonce1", "u1", 8), ("target", "u1", 32)])


def make_job(rng):
    """bench_pool_verify.py's job shape with pieces of its own."""
    return Job(rng.randbytes(100), rng.randbytes(SIZE1), SIZE2, rng.randbytes(250 - 112), [rng.randbytes(32) for _ in range(12)],
               rng.randbytes(32), 0x20000000, 0x1d00ffff, 0x60000000)


def host_times(out_dir):
    """The grouping and the per-job tripwire entries on the host alone, at J = 64."""
    csrc = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "jobs_verify_host_time")
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "jobs_verify_host_time.cpp"), os.path.join(csrc, "bm_job.cpp"),
                               "-o", exe])
        text = subprocess.run([exe, str(N), str(JOBS[-1]), "12"], capture_output=True, text=True, check=True,
                              timeout=300).stdout
    with open(os.path.join(out_dir, "host_time.json"), "w") as fh:
        fh.write(text)
    return json.loads(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    host = host_times(a.out)
    target = zero_bits(ZBITS).to_bytes(32, "big")
    lib = _lib.load()
    rows = []
    with Context(num_gpus=1) as ctx:
        for J in JOBS:
            rng = random.Random(100 + J)
            rs = np.random.RandomState(J)
            jobs = [make_job(rng) for _ in range(J)]
            jarr, _keep = _lib._jobs_array(jobs)
            ses = np.zeros(S, dtype=SESSION)
            ses["extranonce1"][:, :SIZE1] = rs.randint(0, 256, (S, SIZE1))
            ses["target"][:] = list(target)
            subs = np.zeros(N, dtype=JOBS_SUBMIT)
            subs["extranonce2"] = rs.randint(0, 1 << 62, N, dtype=np.uint64)
            for k in ("ntime", "nonce", "version"):
                subs[k] = rs.randint(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
            subs["session"] = rs.randint(0, S, N).astype(np.uint32)
            subs["job"] = rs.randint(0, J, N).astype(np.uint32)       # assigned at random
            ses_c = (_lib.PoolSessionStruct * S).from_buffer(ses)
            subs_c = (_lib.JobsSubmit * N).from_buffer(subs)
            jobs_v = (_lib.JobVerdict * N)()

            # (b): grouped beforehand (a stable sort by job), one job and one slice of the arrays per call
            order = np.argsort(subs["job"], kind="stable")
            grouped = np.zeros(N, dtype=SUBMIT)
            for k in SUBMIT.names:
                grouped[k] = subs[k][order]
            grouped_c = (_lib.PoolSubmit * N).from_buffer(grouped)
            bounds = np.searchsorted(subs["job"][order], np.arange(J + 1))
            per_v = (_lib.JobVerdict * N)()
            sub_ptr, ver_ptr = ctypes.addressof(grouped_c), ctypes.addressof(per_v)
            slices = [(ctypes.cast(sub_ptr + 24 * int(lo), ctypes.POINTER(_lib.PoolSubmit)),
                       ctypes.cast(ver_ptr + 40 * int(lo), ctypes.POINTER(_lib.JobVerdict)), int(hi - lo))
                      for lo, hi in zip(bounds[:-1], bounds[1:])]

            def one_call():
                r = _lib.PoolVerifyResult()
                _lib.check(lib.bm_jobs_verify_gpu(ctx.handle, jarr, J, ses_c, S, subs_c, N, jobs_v, ctypes.byref(r)),
                           "bm_jobs_verify_gpu")
                return r.n, r.shares, r.blocks, r.invalid, r.ntime

            def per_job():
                tot = [0, 0, 0, 0, 0]
                r = _lib.PoolVerifyResult()
                for j, (sp, vp, cnt) in zip(jobs, slices):
                    if cnt == 0:
                        continue
                    _lib.check(lib.bm_pool_verify_gpu(ctx.handle, ctypes.byref(j.struct), ses_c, S, sp, cnt, 0, 0xFFFFFFFF, vp,
                                                      ctypes.byref(r)), "bm_pool_verify_gpu")
                    for i, v in enumerate((r.n, r.shares, r.blocks, r.invalid, r.ntime)):
                        tot[i] += v
                return tuple(tot)

            variants = {"jobs": one_call, "per_job": per_job, "jobs_b": one_call}
            checks = []
            a_bytes = np.frombuffer(jobs_v, dtype=np.uint8).reshape(N, 40)
            b_bytes = np.frombuffer(per_v, dtype=np.uint8).reshape(N, 40)
            checks.append(lambda: np.array_equal(a_bytes[order], b_bytes))
            share_set = None
            if J == 1:  # (c): the single-job entry on the same batch, in the caller's order
                plain = np.zeros(N, dtype=SUBMIT)
                for k in SUBMIT.names:
                    plain[k] = subs[k]
                plain_c = (_lib.PoolSubmit * N).from_buffer(plain)
                pool_v = (_lib.JobVerdict * N)()

                def pool():
                    r = _lib.PoolVerifyResult()
                    _lib.check(lib.bm_pool_verify_gpu(ctx.handle, ctypes.byref(jobs[0].struct), ses_c, S, plain_c, N, 0,
                                                      0xFFFFFFFF, pool_v, ctypes.byref(r)), "bm_pool_verify_gpu")
                    return r.n, r.shares, r.blocks, r.invalid, r.ntime

                variants = {"jobs": one_call, "pool": pool, "per_job": per_job, "jobs_b": one_call}
                checks.append(lambda: bytes(pool_v) == bytes(jobs_v))
            if J == SET_J:  # (d): the share set over the same call, on an empty set
                share_set = ShareSet(ctx, SET_CAPACITY)
                set_v = (_lib.JobVerdict * N)()

                def with_set():
                    r = _lib.ShareSetResult()
                    _lib.check(lib.bm_share_set_verify_jobs(share_set.handle, jarr, J, ses_c, S, subs_c, N, set_v,
                                                            ctypes.byref(r)), "bm_share_set_verify_jobs")
                    assert r.duplicates == 0 and r.recorded == r.shares, (r.duplicates, r.recorded, r.shares)
                    return r.n, r.shares, r.blocks, r.invalid, r.ntime

                variants = {"jobs": one_call, "set": with_set, "per_job": per_job, "jobs_b": one_call}
                checks.append(lambda: bytes(set_v) == bytes(jobs_v))

            ms = {k: [] for k in variants}
            last = {}
            for r in range(a.warmup + a.rounds):
                for k, f in (list(variants.items()) if r % 2 == 0 else reversed(list(variants.items()))):
                    if k == "set":
                        share_set.clear()  # an empty set every time, outside the timer
                    t, last[k] = timed(f)
                    if r >= a.warmup:
                        ms[k].append(t)
                assert all(c() for c in checks), (J, r)
                assert len(set(last.values())) == 1, last
            if share_set is not None:
                share_set.close()
            row = dict(summary(ms), J=J, n=N, sessions=S, shares=last["jobs"][1], rounds_compared=a.warmup + a.rounds,
                       control=ratios(ms, "jobs_b", "jobs"), ratio_jobs_per_job=ratios(ms, "jobs", "per_job"))
            if "pool" in ms:
                row["ratio_jobs_pool"] = ratios(ms, "jobs", "pool")
            if "set" in ms:
                row["ratio_set_jobs"] = ratios(ms, "set", "jobs")
            for k in ("jobs", "per_job"):
                row[f"submissions_per_s_{k}"] = N / row[k]["median_ms"] * 1e3
            rows.append(row)
            print(J, " ".join("%s %.3f ms" % (k, row[k]["median_ms"]) for k in ms), flush=True)

    res = {"rounds": a.rounds, "warmup": a.warmup, "zero_bits": ZBITS, "n": N, "sessions": S, "jobs": list(JOBS),
           "results": rows, "host_alone": host}
    with open(os.path.join(a.out, "bench_jobs_verify.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")

    def band(r):
        return f"{r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]"

    lines = ["# bm_jobs_verify_gpu on one MI355X", "",
             f"`tools/bench_jobs_verify.py`: n = 2^17 random valid submissions over 2^12 sessions and J synthetic jobs (a "
             f"12-entry branch and a 250-byte coinbase each), the jobs assigned at random, a target of {ZBITS} zero bits; "
             f"medians of {a.rounds} rounds after {a.warmup} warm-up, the variants alternating in one process, every call "
             "through the C ABI into buffers allocated once.  (a) is one `bm_jobs_verify_gpu` call; (b) is the submissions "
             "grouped by job beforehand and J `bm_pool_verify_gpu` calls, the calls alone timed.  A ratio is per round "
             "(below 1: the one call is faster), given as median [min, max]; the control is (a) against itself.  The verdict "
             "bytes of all variants were compared in every round.  Raw figures: `bench_jobs_verify.json`, `host_time.json`.",
             "", "| J | (a) one call ms | submissions/s (a) | (b) J calls ms | submissions/s (b) | (a) / (b) | control |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['J']} | {r['jobs']['median_ms']:.3f} | {r['submissions_per_s_jobs']:.3e} | "
                     f"{r['per_job']['median_ms']:.3f} | {r['submissions_per_s_per_job']:.3e} | "
                     f"{band(r['ratio_jobs_per_job'])} | {band(r['control'])} |")
    one, eight = rows[0], [r for r in rows if r["J"] == SET_J][0]
    lines += ["", f"* (c) at J = 1, `bm_pool_verify_gpu` on the same batch: {one['pool']['median_ms']:.3f} ms; (a) / (c) "
                  f"{band(one['ratio_jobs_pool'])}, control {band(one['control'])}",
              f"* (d) at J = {SET_J}, `bm_share_set_verify_jobs` on an empty 2^22 set: {eight['set']['median_ms']:.3f} ms; "
              f"(d) / (a) {band(eight['ratio_set_jobs'])}, control {band(eight['control'])}",
              f"* on the host alone at J = {host['jobs']}: the grouping (count, block table, scatter) "
              f"{host['grouping']['median_ms']:.3f} ms [{host['grouping']['min_ms']:.3f}, {host['grouping']['max_ms']:.3f}] over "
              f"{host['blocks']} workgroups; the tripwire's per-job entries "
              f"{host['tripwire_per_job']['median_ms']:.3f} ms [{host['tripwire_per_job']['min_ms']:.3f}, "
              f"{host['tripwire_per_job']['max_ms']:.3f}]",
              "* every figure of the table is a whole call, copies and host work included",
              "* not measured: the kernel's own time, the shader clock, PMC counters, more than one GPU"]
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
