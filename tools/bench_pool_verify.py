#!/usr/bin/env python3
"""Measure bm_pool_verify_gpu on one GPU ("Share
verification across sessions"), tools/bench_verify.py's method: medians of
--rounds rounds after --warmup, the variants alternating inside each round (their
order reversed every second round), every call through the C ABI into buffers
allocated once.  The synthetic job (a 12-entry branch, a 250-byte coinbase), n =
2^17 random valid submissions spread evenly over S sessions, S = 1, 2^6, 2^12:

  pool/pool_b  (a) one bm_pool_verify_gpu call; pool_b is the control: its
               per-round ratio to pool is the noise band
  per_session  (b) the parent's way: the submissions grouped by session
               beforehand, then S bm_job_verify_gpu calls, each with its
               session's extranonce1 and target.  Only the calls are timed, which
               favours this variant
  (c)          at S = 1, (a) over (b): what the generality costs
  cpu          (d) one thread on bm_pool_verify_cpu at n = 2^14, for scale

The verdict bytes of (a) and (b) are compared every round.  Writes
profiles/pool_verify/bench_pool_verify.json and README.md."""
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

OUT = os.path.join(ROOT, "profiles", "pool_verify")
N = 1 << 17
N_CPU = 1 << 14
SESSIONS = (1, 1 << 6, 1 << 12)
ZBITS = 8
SIZE1, SIZE2 = 4, 8
SUBMIT = np.dtype([("extranonce2", "<u8"), ("ntime", "<u4"), ("nonce", "<u4"), ("version", "<u4"), ("session", "<u4")])
SESSION = np.dtype([("extranonce1", "u1", 8), ("target", "u1", 32)])


def parts():
    """The synthetic job's pieces: bench_verify.py's `deep` job (its extranonce1 is session 0's)."""
    rng = random.Random(12)
    return dict(coinb1=rng.randbytes(100), en1=rng.randbytes(SIZE1), coinb2=rng.randbytes(250 - 112),
                branch=[rng.randbytes(32) for _ in range(12)], prevhash=rng.randbytes(32))


def job_with(p, en1):
    return Job(p["coinb1"], en1, SIZE2, p["coinb2"], p["branch"], p["prevhash"], 0x20000000, 0x1d00ffff, 0x60000000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    target = zero_bits(ZBITS).to_bytes(32, "big")
    lib = _lib.load()
    p = parts()
    rows = []
    with Context(num_gpus=1) as ctx:
        for S in SESSIONS:
            rs = np.random.RandomState(S)
            ses = np.zeros(S, dtype=SESSION)
            ses["extranonce1"][:, :SIZE1] = rs.randint(0, 256, (S, SIZE1))
            ses["extranonce1"][0, :SIZE1] = list(p["en1"])
            ses["target"][:] = list(target)
            subs = np.zeros(N, dtype=SUBMIT)
            subs["extranonce2"] = rs.randint(0, 1 << 62, N, dtype=np.uint64)
            for k in ("ntime", "nonce", "version"):
                subs[k] = rs.randint(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
            subs["session"] = np.arange(N, dtype=np.uint32) % S      # spread evenly, adjacent lanes in different sessions
            ses_c = (_lib.PoolSessionStruct * S).from_buffer(ses)
            subs_c = (_lib.PoolSubmit * N).from_buffer(subs)
            pool_v = (_lib.JobVerdict * N)()
            job = job_with(p, p["en1"])

            # (b): grouped beforehand (a stable sort by session), one job and one slice of the arrays per session
            order = np.argsort(subs["session"], kind="stable")
            grouped = np.ascontiguousarray(subs[order])
            grouped["session"] = 0                                     # bm_job_submit_t's reserved
            grouped_c = (_lib.JobSubmit * N).from_buffer(grouped)
            bounds = np.searchsorted(subs["session"][order], np.arange(S + 1))
            jobs = [job_with(p, bytes(ses["extranonce1"][s, :SIZE1])) for s in range(S)]
            per_v = (_lib.JobVerdict * N)()
            sub_ptr, ver_ptr = ctypes.addressof(grouped_c), ctypes.addressof(per_v)
            slices = [(ctypes.cast(sub_ptr + 24 * int(lo), ctypes.POINTER(_lib.JobSubmit)),
                       ctypes.cast(ver_ptr + 40 * int(lo), ctypes.POINTER(_lib.JobVerdict)), int(hi - lo))
                      for lo, hi in zip(bounds[:-1], bounds[1:])]

            def pool():
                r = _lib.PoolVerifyResult()
                _lib.check(lib.bm_pool_verify_gpu(ctx.handle, ctypes.byref(job.struct), ses_c, S, subs_c, N, 0, 0xFFFFFFFF,
                                                  pool_v, ctypes.byref(r)), "bm_pool_verify_gpu")
                return r.n, r.shares, r.blocks, r.invalid

            def per_session():
                tot = [0, 0, 0, 0]
                r = _lib.JobVerifyResult()
                for j, (sp, vp, cnt) in zip(jobs, slices):
                    _lib.check(lib.bm_job_verify_gpu(ctx.handle, ctypes.byref(j.struct), target, sp, cnt, vp,
                                                     ctypes.byref(r)), "bm_job_verify_gpu")
                    for i, v in enumerate((r.n, r.shares, r.blocks, r.invalid)):
                        tot[i] += v
                return tuple(tot)

            # alternate()'s loop, one round at a time, so that the verdict bytes are compared after every round
            # (outside the timed calls)
            ms = {k: [] for k in ("pool", "per_session", "pool_b")}
            a_bytes = np.frombuffer(pool_v, dtype=np.uint8).reshape(N, 40)
            b_bytes = np.frombuffer(per_v, dtype=np.uint8).reshape(N, 40)
            for r in range(a.warmup + a.rounds):
                one, last = alternate({"pool": pool, "per_session": per_session, "pool_b": pool} if r % 2 == 0 else
                                      {"pool_b": pool, "per_session": per_session, "pool": pool}, 1, 0)
                assert np.array_equal(a_bytes[order], b_bytes), (S, r)
                assert last["pool"] == last["per_session"] == last["pool_b"], last
                if r >= a.warmup:
                    for k in ms:
                        ms[k] += one[k]
            row = dict(summary(ms), sessions=S, n=N, shares=last["pool"][1], rounds_compared=a.warmup + a.rounds,
                       control=ratios(ms, "pool_b", "pool"), ratio_pool_per_session=ratios(ms, "pool", "per_session"))
            for k in ("pool", "per_session"):
                row[f"submissions_per_s_{k}"] = N / row[k]["median_ms"] * 1e3
            rows.append(row)
            print(S, "pool %.3f ms" % row["pool"]["median_ms"], "per_session %.3f ms" % row["per_session"]["median_ms"],
                  flush=True)

        # (d): one CPU thread, for scale, against the GPU call at the same n
        S = SESSIONS[1]
        rs = np.random.RandomState(7)
        ses = np.zeros(S, dtype=SESSION)
        ses["extranonce1"][:, :SIZE1] = rs.randint(0, 256, (S, SIZE1))
        ses["target"][:] = list(target)
        subs = np.zeros(N_CPU, dtype=SUBMIT)
        subs["extranonce2"] = rs.randint(0, 1 << 62, N_CPU, dtype=np.uint64)
        for k in ("ntime", "nonce", "version"):
            subs[k] = rs.randint(0, 1 << 32, N_CPU, dtype=np.uint64).astype(np.uint32)
        subs["session"] = np.arange(N_CPU, dtype=np.uint32) % S
        ses_c = (_lib.PoolSessionStruct * S).from_buffer(ses)
        subs_c = (_lib.PoolSubmit * N_CPU).from_buffer(subs)
        gpu_v, cpu_v = (_lib.JobVerdict * N_CPU)(), (_lib.JobVerdict * N_CPU)()
        job = job_with(p, p["en1"])

        def gpu():
            r = _lib.PoolVerifyResult()
            _lib.check(lib.bm_pool_verify_gpu(ctx.handle, ctypes.byref(job.struct), ses_c, S, subs_c, N_CPU, 0, 0xFFFFFFFF,
                                              gpu_v, ctypes.byref(r)), "bm_pool_verify_gpu")
            return bytes(r)

        def cpu():
            r = _lib.PoolVerifyResult()
            _lib.check(lib.bm_pool_verify_cpu(ctypes.byref(job.struct), ses_c, S, subs_c, N_CPU, 0, 0xFFFFFFFF, cpu_v,
                                              ctypes.byref(r)), "bm_pool_verify_cpu")
            return bytes(r)

        ms, last = alternate({"gpu": gpu, "cpu": cpu, "gpu_b": gpu}, a.rounds, a.warmup)
        assert last["gpu"] == last["cpu"] and bytes(gpu_v) == bytes(cpu_v)
        scale = dict(summary(ms), sessions=S, n=N_CPU, control=ratios(ms, "gpu_b", "gpu"), ratio_gpu_cpu=ratios(ms, "gpu", "cpu"))

    res = {"rounds": a.rounds, "warmup": a.warmup, "zero_bits": ZBITS, "n": N, "sessions": list(SESSIONS), "results": rows,
           "cpu_scale": scale}
    with open(os.path.join(a.out, "bench_pool_verify.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")

    def band(r):
        return f"{r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]"

    lines = ["# bm_pool_verify_gpu on one MI355X", "",
             f"`tools/bench_pool_verify.py`: the synthetic job (a 12-entry branch, a 250-byte coinbase), n = 2^17 random "
             f"valid submissions spread evenly over S sessions, a target of {ZBITS} zero bits; medians of {a.rounds} rounds "
             f"after {a.warmup} warm-up, the variants alternating in one process, every call through the C ABI into buffers "
             "allocated once.  (a) is one `bm_pool_verify_gpu` call; (b) is the submissions grouped by session beforehand "
             "and S `bm_job_verify_gpu` calls, the calls alone timed.  A ratio is per round (below 1: the one call is "
             "faster), given as median [min, max]; the control is (a) against itself.  The verdict bytes of (a) and (b) "
             "were compared in every round.  Raw figures: `bench_pool_verify.json`.", "",
             "| S | (a) one call ms | submissions/s (a) | (b) S calls ms | submissions/s (b) | (a) / (b) | control |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['sessions']} | {r['pool']['median_ms']:.3f} | {r['submissions_per_s_pool']:.3e} | "
                     f"{r['per_session']['median_ms']:.3f} | {r['submissions_per_s_per_session']:.3e} | "
                     f"{band(r['ratio_pool_per_session'])} | {band(r['control'])} |")
    lines += ["", f"* (c) what the generality costs: the S = 1 row's (a) / (b), {band(rows[0]['ratio_pool_per_session'])}",
              f"* (d) one CPU thread on `bm_pool_verify_cpu` at n = 2^14 over {scale['sessions']} sessions: "
              f"{scale['cpu']['median_ms']:.3f} ms against {scale['gpu']['median_ms']:.3f} ms for the GPU call; GPU / CPU "
              f"{band(scale['ratio_gpu_cpu'])}, control {band(scale['control'])}",
              "* every figure is a whole call, copies and host work included",
              "* not measured: the kernel's own time, the shader clock, PMC counters, more than one GPU"]
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
