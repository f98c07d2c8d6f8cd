#!/usr/bin/env python3
"""Measure bm_share_set_verify on one GPU ("Duplicate-share
detection"), tools/bench_pool_verify.py's method and workload: medians of --rounds
rounds after --warmup, the variants alternating inside each round (their order
reversed every second round), every call through the C ABI into buffers allocated
once.  The synthetic job (a 12-entry branch, a 250-byte coinbase), n = 2^17 valid
submissions over S = 2^12 sessions whose target lets every hash through, a set of
capacity 2^22.  Every round has a batch of its own, so that its shares are all new
to both sets:

  verify/verify_b  bm_pool_verify_gpu alone; verify_b is the control: its per-round
                   ratio to verify is the noise band
  set_empty        (a, b) bm_share_set_verify on a set cleared before the call (the
                   clear is not timed): what detection costs on top of verification
  set_filled       (b) the same on a set that holds 2^21 other hashes (and the
                   earlier rounds' batches)
  host_way         (c) the parent's way: bm_pool_verify_gpu, then the library's CPU
                   set step over the returned hashes on this thread
                   (host::share_set_apply, built from tools/share_set_host_insert.cpp);
                   both parts are timed, and the second one alone (host_insert)
  one_slot         (d) the worst contention: 2^17 copies of one submission, every
                   lane on one slot, on a cleared set; against verify_same, the plain
                   call on that batch

The verdicts of set_empty, set_filled and host_way are compared with verify's every
round (no duplicate among all-new shares).  Writes
profiles/share_set/bench_share_set.json and README.md."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from distributed_bitcoin_minter_amd import Context, _lib  # noqa: E402
from bench_header_hits import ratios, summary, timed  # noqa: E402
from bench_pool_verify import SESSION, SIZE1, SUBMIT, job_with, parts  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "share_set")
N = 1 << 17
S = 1 << 12
CAPACITY = 1 << 22
PREFILL = 1 << 21
CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")


def batch(seed):
    """(numpy array, ctypes view) of N random valid submissions spread evenly over the sessions."""
    rs = np.random.RandomState(seed)
    subs = np.zeros(N, dtype=SUBMIT)
    subs["extranonce2"] = rs.randint(0, 1 << 62, N, dtype=np.uint64)
    for k in ("ntime", "nonce", "version"):
        subs[k] = rs.randint(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    subs["session"] = np.arange(N, dtype=np.uint32) % S
    return subs, (_lib.PoolSubmit * N).from_buffer(subs)


def build_helper(d):
    so = os.path.join(d, "share_set_host_insert.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "share_set_host_insert.cpp"), "-o", so])
    helper = ctypes.CDLL(so)
    helper.bench_share_set_apply.argtypes = [ctypes.c_void_p, ctypes.POINTER(_lib.JobVerdict), ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_uint64)]
    helper.bench_share_set_apply.restype = ctypes.c_int
    return helper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    total = a.warmup + a.rounds
    assert PREFILL + total * N <= CAPACITY, "the filled set must hold every round's batch"
    lib = _lib.load()
    p = parts()
    job = job_with(p, p["en1"])
    rs = np.random.RandomState(S)
    ses = np.zeros(S, dtype=SESSION)
    ses["extranonce1"][:, :SIZE1] = rs.randint(0, 256, (S, SIZE1))
    ses["target"][:] = 0xFF                                   # every hash is a share: every lane goes through the set
    ses_c = (_lib.PoolSessionStruct * S).from_buffer(ses)
    W = (0, 0xFFFFFFFF)
    j = ctypes.byref(job.struct)
    bufs = {k: (_lib.JobVerdict * N)() for k in ("verify", "set_empty", "set_filled", "host_way", "one_slot")}
    views = {k: np.frombuffer(v, dtype=np.uint8).reshape(N, 40) for k, v in bufs.items()}

    with tempfile.TemporaryDirectory() as tmp, Context(num_gpus=1) as ctx:
        helper = build_helper(tmp)
        h = lambda: ctypes.c_void_p()  # noqa: E731
        empty, filled, host = h(), h(), h()
        _lib.check(lib.bm_share_set_create(ctx.handle, CAPACITY, ctypes.byref(empty)), "bm_share_set_create")
        _lib.check(lib.bm_share_set_create(ctx.handle, CAPACITY, ctypes.byref(filled)), "bm_share_set_create")
        _lib.check(lib.bm_share_set_create_cpu(CAPACITY, ctypes.byref(host)), "bm_share_set_create_cpu")
        try:
            r = _lib.ShareSetResult()
            for k in range(PREFILL // N):                     # (untimed) 2^21 other hashes
                _subs, subs_c = batch(1000 + k)
                _lib.check(lib.bm_share_set_verify(filled, j, ses_c, S, subs_c, N, *W, bufs["set_filled"], ctypes.byref(r)),
                           "bm_share_set_verify")
                assert r.recorded == N and r.duplicates == 0, (k, r.recorded, r.duplicates)
            assert r.count == PREFILL
            hot = np.zeros(N, dtype=SUBMIT)
            hot[:] = batch(999)[0][0]                         # 2^17 copies of one submission
            hot_c = (_lib.PoolSubmit * N).from_buffer(hot)

            def verify(subs_c, key="verify"):
                def f():
                    pr = _lib.PoolVerifyResult()
                    _lib.check(lib.bm_pool_verify_gpu(ctx.handle, j, ses_c, S, subs_c, N, *W, bufs[key], ctypes.byref(pr)),
                               "bm_pool_verify_gpu")
                    return pr.shares
                return f

            def on_set(handle, subs_c, key):
                def f():
                    sr = _lib.ShareSetResult()
                    _lib.check(lib.bm_share_set_verify(handle, j, ses_c, S, subs_c, N, *W, bufs[key], ctypes.byref(sr)),
                               "bm_share_set_verify")
                    return sr.shares, sr.duplicates, sr.recorded
                return f

            host_part = []

            def host_way(subs_c):
                def f():
                    shares = verify(subs_c, "host_way")()
                    rec = ctypes.c_uint64(0)
                    t, rc = timed(lambda: helper.bench_share_set_apply(host, bufs["host_way"], N, ctypes.byref(rec)))
                    assert rc == 0
                    host_part.append(t)
                    return shares, rec.value
                return f

            names = ("verify", "set_empty", "set_filled", "host_way", "verify_b", "one_slot", "verify_same")
            ms = {k: [] for k in names + ("host_insert",)}
            for rnd in range(total):
                _subs, subs_c = batch(rnd)
                variants = {"verify": verify(subs_c), "set_empty": on_set(empty, subs_c, "set_empty"),
                            "set_filled": on_set(filled, subs_c, "set_filled"), "host_way": host_way(subs_c),
                            "verify_b": verify(subs_c), "one_slot": on_set(empty, hot_c, "one_slot"),
                            "verify_same": verify(hot_c, "one_slot")}
                order = list(names) if rnd % 2 == 0 else list(reversed(names))
                last, one = {}, {}
                for k in order:
                    if k in ("set_empty", "one_slot"):       # (untimed) these start from an empty set
                        _lib.check(lib.bm_share_set_clear(empty), "bm_share_set_clear")
                    if k == "host_way":
                        _lib.check(lib.bm_share_set_clear(host), "bm_share_set_clear")
                    one[k], last[k] = timed(variants[k])
                    if k == "one_slot":
                        flags = views["one_slot"][:, 32].copy()
                        assert last[k] == (N, N - 1, 1) and flags[0] & 16 == 0 and (flags[1:] & 16).all(), last[k]
                assert last["set_empty"] == last["set_filled"] == (N, 0, N) and last["host_way"] == (N, N), last
                for k in ("set_empty", "set_filled", "host_way"):
                    assert np.array_equal(views[k], views["verify"]), (k, rnd)
                if rnd >= a.warmup:
                    for k in names:
                        ms[k].append(one[k])
                    ms["host_insert"].append(host_part[-1])
        finally:
            for s in (empty, filled, host):
                lib.bm_share_set_destroy(s)

    row = dict(summary(ms), n=N, sessions=S, capacity=CAPACITY, prefill=PREFILL, rounds_compared=total,
               control=ratios(ms, "verify_b", "verify"),
               ratio_set_empty_verify=ratios(ms, "set_empty", "verify"),
               ratio_set_filled_verify=ratios(ms, "set_filled", "verify"),
               ratio_set_filled_set_empty=ratios(ms, "set_filled", "set_empty"),
               ratio_set_empty_host_way=ratios(ms, "set_empty", "host_way"),
               ratio_one_slot_verify_same=ratios(ms, "one_slot", "verify_same"))
    res = {"rounds": a.rounds, "warmup": a.warmup, "results": row}
    with open(os.path.join(a.out, "bench_share_set.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")

    def band(r):
        return f"{r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]"

    def med(k):
        return f"{row[k]['median_ms']:.3f}"

    lines = ["# bm_share_set_verify on one MI355X", "",
             f"`tools/bench_share_set.py`: the synthetic job (a 12-entry branch, a 250-byte coinbase), n = 2^17 valid "
             f"submissions over S = 2^12 sessions, every hash a share, a set of capacity 2^22; medians of {a.rounds} rounds "
             f"after {a.warmup} warm-up, the variants alternating in one process, every call through the C ABI into buffers "
             "allocated once; every round has a batch of its own, all new to both sets.  A ratio is per round, given as "
             "median [min, max]; the control is `bm_pool_verify_gpu` against itself.  The verdict bytes of every variant "
             "were compared with the plain call's in every round.  Raw figures: `bench_share_set.json`.", "",
             "| variant | median ms | ratio | per round |", "|---|---|---|---|",
             f"| `bm_pool_verify_gpu` alone | {med('verify')} | control | {band(row['control'])} |",
             f"| (a) `bm_share_set_verify`, empty set | {med('set_empty')} | to the plain call | "
             f"{band(row['ratio_set_empty_verify'])} |",
             f"| (b) the same, the set holding 2^21 hashes | {med('set_filled')} | to the plain call | "
             f"{band(row['ratio_set_filled_verify'])} |",
             f"| (b) filled against empty | | | {band(row['ratio_set_filled_set_empty'])} |",
             f"| (c) the plain call, then the CPU set step on one thread | {med('host_way')} (the step alone: "
             f"{med('host_insert')}) | (a) to (c) | {band(row['ratio_set_empty_host_way'])} |",
             f"| (d) 2^17 copies of one submission, every lane on one slot | {med('one_slot')} | to the plain call on that "
             f"batch ({med('verify_same')} ms) | {band(row['ratio_one_slot_verify_same'])} |", "",
             "* every figure is a whole call, copies and host work included; a set is cleared outside the timed call",
             "* (d) is atomic-bound by design (one word takes 2^17 atomics), like dense hit enumeration",
             "* not measured: the kernels' own times, the shader clock, PMC counters, more than one GPU"]
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
