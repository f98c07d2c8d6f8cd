#!/usr/bin/env python3
"""Measure bm_job_verify_gpu on one GPU ("Share
verification"): medians of --rounds rounds after --warmup, the variants
alternating inside each round (their order reversed every second round).  n =
2^10, 2^14, 2^17, 2^20 random valid submissions of two jobs:

  genesis    tests/golden/stratum_genesis_job.json: no branch, a 204-byte coinbase
  deep       a synthetic job of random bytes: a 12-entry branch, a 250-byte coinbase

  gpu/gpu_b  bm_job_verify_gpu; gpu_b is the control: its per-round ratio to gpu
             is the noise band
  cpu        bm_job_verify_cpu on one thread: what a caller without the kernel runs

Every call is timed through the C ABI into buffers allocated once; the two
entries' verdicts are compared byte for byte at every size.  At n = 2^20 the
kernel's plain compressions per second (nb + 1 + 3 * depth + 3 per submission)
stand beside header_hash_kernel's (2 per nonce, through bm_header_hash_gpu at
the same n): both are whole calls, copies included.  Writes
profiles/verify/bench_verify.json and README.md."""
import argparse
import ctypes
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from distributed_bitcoin_minter_amd import Context, Job, _lib  # noqa: E402
from bench_header_hits import alternate, ratios, summary, zero_bits  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "verify")
SIZES = (1 << 10, 1 << 14, 1 << 17, 1 << 20)
ZBITS = 8
SUBMIT = np.dtype([("extranonce2", "<u8"), ("ntime", "<u4"), ("nonce", "<u4"), ("version", "<u4"), ("reserved", "<u4")])


def jobs():
    with open(os.path.join(ROOT, "tests", "golden", "stratum_genesis_job.json")) as f:
        spec = json.load(f)
    genesis = Job.from_notify(spec["notify"], spec["extranonce1"], spec["extranonce2_size"])
    rng = random.Random(12)
    deep = Job(rng.randbytes(100), rng.randbytes(4), 8, rng.randbytes(250 - 112), [rng.randbytes(32) for _ in range(12)],
               rng.randbytes(32), 0x20000000, 0x1d00ffff, 0x60000000)
    return {"genesis": genesis, "deep": deep}


def compressions(job):
    """Per submission on the device: the tail's blocks, the coinbase's second
    hash, three per branch entry, three for the header."""
    pos = len(job.coinb1) + len(job.extranonce1)
    total = pos + job.extranonce2_size + len(job.coinb2)
    nb = (total + 9 + 63) // 64 - pos // 64
    return nb + 1 + 3 * len(job.branch) + 3


def submissions(job, n, seed):
    rs = np.random.RandomState(seed)
    a = np.zeros(n, dtype=SUBMIT)
    a["extranonce2"] = rs.randint(0, 1 << 62, n, dtype=np.uint64) & np.uint64((1 << (8 * job.extranonce2_size)) - 1)
    for k in ("ntime", "nonce", "version"):
        a[k] = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return (_lib.JobSubmit * n).from_buffer(a), a  # (the array keeps the buffer alive)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    target = zero_bits(ZBITS).to_bytes(32, "big")
    lib = _lib.load()
    rows = []
    with Context(num_gpus=1) as ctx:
        for name, job in jobs().items():
            per = compressions(job)
            for n in SIZES:
                subs, keep = submissions(job, n, n)
                gpu_v, cpu_v = (_lib.JobVerdict * n)(), (_lib.JobVerdict * n)()

                def gpu():
                    r = _lib.JobVerifyResult()
                    _lib.check(lib.bm_job_verify_gpu(ctx.handle, ctypes.byref(job.struct), target, subs, n, gpu_v,
                                                     ctypes.byref(r)), "bm_job_verify_gpu")
                    return r.n, r.shares, r.blocks, r.invalid

                def cpu():
                    r = _lib.JobVerifyResult()
                    _lib.check(lib.bm_job_verify_cpu(ctypes.byref(job.struct), target, subs, n, cpu_v, ctypes.byref(r)),
                               "bm_job_verify_cpu")
                    return r.n, r.shares, r.blocks, r.invalid

                ms, last = alternate({"gpu": gpu, "cpu": cpu, "gpu_b": gpu}, a.rounds, a.warmup)
                assert last["gpu"] == last["cpu"] == last["gpu_b"], last
                assert bytes(gpu_v) == bytes(cpu_v), (name, n)
                row = dict(summary(ms), job=name, n=n, compressions_per_submission=per, shares=last["gpu"][1],
                           control=ratios(ms, "gpu_b", "gpu"), ratio_gpu_cpu=ratios(ms, "gpu", "cpu"))
                for k in ("gpu", "cpu"):
                    row[f"submissions_per_s_{k}"] = n / row[k]["median_ms"] * 1e3
                row["compressions_per_s_gpu"] = per * row["submissions_per_s_gpu"]
                rows.append(row)
                print(name, n, "gpu %.3f ms" % row["gpu"]["median_ms"], "cpu %.3f ms" % row["cpu"]["median_ms"], flush=True)

        # the plain-compression yardstick: header_hash_kernel through its own call, two compressions per nonce
        n = SIZES[-1]
        header = jobs()["genesis"].header(29)
        nonces = (ctypes.c_uint32 * n)(*range(n))
        hashes = (ctypes.c_uint8 * (32 * n))()

        def header_hash():
            _lib.check(lib.bm_header_hash_gpu(ctx.handle, header, nonces, n, hashes), "bm_header_hash_gpu")
            return bytes(hashes[:32])

        ms, _ = alternate({"header_hash": header_hash, "header_hash_b": header_hash}, a.rounds, a.warmup)
        yard = dict(summary(ms), n=n, control=ratios(ms, "header_hash_b", "header_hash"))
        yard["compressions_per_s"] = 2 * n / yard["header_hash"]["median_ms"] * 1e3

    res = {"rounds": a.rounds, "warmup": a.warmup, "zero_bits": ZBITS, "sizes": list(SIZES), "results": rows,
           "header_hash": yard}
    with open(os.path.join(a.out, "bench_verify.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")

    def band(r):
        return f"{r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]"

    lines = ["# bm_job_verify_gpu on one MI355X", "",
             f"`tools/bench_verify.py`: random valid submissions against a target of {ZBITS} zero bits; medians of "
             f"{a.rounds} rounds after {a.warmup} warm-up, the variants alternating in one process, every call through "
             "the C ABI into buffers allocated once.  `cpu` is `bm_job_verify_cpu` on one thread.  A ratio is per round "
             "(below 1: the GPU call is faster), given as median [min, max]; the control is the GPU call against "
             "itself.  Raw figures: `bench_verify.json`.", "",
             "| job | compressions / submission | n | GPU call ms | submissions/s GPU | CPU call ms | submissions/s CPU "
             "| GPU / CPU | control |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['job']} | {r['compressions_per_submission']} | {r['n']} | {r['gpu']['median_ms']:.3f} | "
                     f"{r['submissions_per_s_gpu']:.3e} | {r['cpu']['median_ms']:.3f} | {r['submissions_per_s_cpu']:.3e} | "
                     f"{band(r['ratio_gpu_cpu'])} | {band(r['control'])} |")
    lines.append("")
    for name in ("genesis", "deep"):
        wins = [r["n"] for r in rows if r["job"] == name and r["ratio_gpu_cpu"]["max"] < 1]
        big = next(r for r in rows if r["job"] == name and r["n"] == SIZES[-1])
        lines.append(f"* {name}: the smallest measured n at which the GPU call wins in every round: "
                     + (str(min(wins)) if wins else "none") + f"; at n = 2^20 {big['compressions_per_s_gpu']:.3e} "
                     "compressions/s through the whole call")
    lines += [f"* the yardstick, `bm_header_hash_gpu` at n = 2^20 (header_hash_kernel, 2 compressions per nonce, 4 bytes "
              f"in and 32 out per nonce): {yard['header_hash']['median_ms']:.3f} ms, {yard['compressions_per_s']:.3e} "
              f"compressions/s through the whole call; control {band(yard['control'])}",
              "* both rates include the call's copies and host work; the kernels alone were not timed",
              "* not measured: the shader clock, PMC counters, more than one GPU"]
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
