#!/usr/bin/env python3
"""Measure bm_ledger_verify_jobs on one GPU ("Share
accounting"), tools/bench_jobs_verify.py's method: medians of --rounds rounds after
--warmup, the variants alternating inside each round (their order reversed every
second round), every call through the C ABI into buffers allocated once.  n = 2^17
random submissions that are all accepted, over 2^12 sessions and J = 8 synthetic jobs
(a 12-entry branch and a 250-byte coinbase each), a 2^22 share set cleared outside the
timer before every call, and a ledger cleared outside the timer likewise:

  ledger_pR  (a) one bm_ledger_verify_jobs call at R = 0, 1, 4, 64 peel rounds;
             ledger_b is the control: (a) at 4 rounds again, its per-round ratio to
             ledger_p4 is the noise band
  host_way   (b) the parent's way: bm_share_set_verify_jobs, then the CPU ledger's
             crediting loop on this thread over the returned verdicts
             (tools/ledger_host_credit.cpp); host_credit is that loop alone
  set        (c) bm_share_set_verify_jobs alone: (a) / (c) is what the ledger adds

under four account maps: the identity (2^12 rows), 64 accounts uniform, a skewed map
(half of all submissions on one account, the rest over 2^12) and one account for
everything.  The verdict bytes and the ledger rows of all variants are compared
every round.  Writes profiles/ledger/bench_ledger.json and README.md."""
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
from distributed_bitcoin_minter_amd import Context, Ledger, ShareSet, _lib  # noqa: E402
from bench_header_hits import ratios, summary, timed  # noqa: E402
from bench_jobs_verify import JOBS_SUBMIT, SESSION, SIZE1, make_job  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ledger")
CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")
N = 1 << 17
S = 1 << 12
J = 8
SET_CAPACITY = 1 << 22
PEELS = (0, 1, 4, 64)
MAPS = ("identity", "uniform64", "skewed", "one")


def build_helper(d):
    so = os.path.join(d, "ledger_host_credit.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "ledger_host_credit.cpp"), "-o", so])
    helper = ctypes.CDLL(so)
    helper.bench_ledger_credit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]
    helper.bench_ledger_credit.restype = None
    return helper


def account_map(kind, rs, sessions_of_subs):
    """(rows, accounts[] by session).  The skewed map gives one account to sessions
    that carry half of all submissions: the sessions are sorted by load and taken
    until they hold half."""
    if kind == "identity":
        return S, np.arange(S, dtype=np.uint32)
    if kind == "uniform64":
        return 64, rs.randint(0, 64, S).astype(np.uint32)
    if kind == "one":
        return 1, np.zeros(S, dtype=np.uint32)
    load = np.bincount(sessions_of_subs, minlength=S)
    order = rs.permutation(S)
    acc = np.arange(S, dtype=np.uint32)
    acc[order[np.cumsum(load[order]) <= N // 2]] = 0
    return S, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lib = _lib.load()
    rows_out = []
    with tempfile.TemporaryDirectory() as d, Context(num_gpus=1) as ctx:
        helper = build_helper(d)
        rng = random.Random(108)
        rs = np.random.RandomState(8)
        jobs = [make_job(rng) for _ in range(J)]
        jarr, _keep = _lib._jobs_array(jobs)
        ses = np.zeros(S, dtype=SESSION)
        ses["extranonce1"][:, :SIZE1] = rs.randint(0, 256, (S, SIZE1))
        ses["target"][:] = 0xFF   # every submission is accepted
        subs = np.zeros(N, dtype=JOBS_SUBMIT)
        subs["extranonce2"] = rs.randint(0, 1 << 62, N, dtype=np.uint64)
        for k in ("ntime", "nonce", "version"):
            subs[k] = rs.randint(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
        subs["session"] = rs.randint(0, S, N).astype(np.uint32)
        subs["job"] = rs.randint(0, J, N).astype(np.uint32)
        weights = rs.randint(1, 1 << 62, S, dtype=np.uint64)
        ses_c = (_lib.PoolSessionStruct * S).from_buffer(ses)
        subs_c = (_lib.JobsSubmit * N).from_buffer(subs)
        wgt_c = (ctypes.c_uint64 * S).from_buffer(weights)
        with ShareSet(ctx, SET_CAPACITY) as share_set:
            for kind in MAPS:
                nrows, accounts = account_map(kind, rs, subs["session"])
                acc_c = (ctypes.c_uint32 * S).from_buffer(accounts)
                top = int(np.bincount(accounts[subs["session"]], minlength=nrows).max())
                ledgers = {p: Ledger(ctx, nrows) for p in PEELS}
                for p, led in ledgers.items():
                    led.set_peel(p)
                verdicts = {k: (_lib.JobVerdict * N)() for k in [f"ledger_p{p}" for p in PEELS] + ["host_way", "set"]}
                verdicts["ledger_b"] = verdicts["ledger_p4"]
                host_rows = np.zeros((nrows, 8), dtype=np.uint64)
                host_part = []

                def on_ledger(p, name):
                    def f():
                        r = _lib.LedgerResult()
                        _lib.check(lib.bm_ledger_verify_jobs(ledgers[p].handle, share_set.handle, jarr, J, ses_c, S, acc_c, wgt_c,
                                                             subs_c, N, verdicts[name], ctypes.byref(r)), "bm_ledger_verify_jobs")
                        assert r.credited == N and r.duplicates == 0, (r.credited, r.duplicates)
                        return r.n, r.shares, r.blocks, r.invalid, r.ntime
                    return f

                def set_alone(name):
                    def f():
                        r = _lib.ShareSetResult()
                        _lib.check(lib.bm_share_set_verify_jobs(share_set.handle, jarr, J, ses_c, S, subs_c, N, verdicts[name],
                                                                ctypes.byref(r)), "bm_share_set_verify_jobs")
                        return r.n, r.shares, r.blocks, r.invalid, r.ntime
                    return f

                def host_way():
                    got = set_alone("host_way")()
                    t, _ = timed(lambda: helper.bench_ledger_credit(ctypes.addressof(subs_c), ctypes.addressof(verdicts["host_way"]),
                                                                    N, S, ctypes.addressof(acc_c), ctypes.addressof(wgt_c),
                                                                    host_rows.ctypes.data))
                    host_part.append(t)
                    return got

                variants = {f"ledger_p{p}": on_ledger(p, f"ledger_p{p}") for p in PEELS}
                variants.update({"host_way": host_way, "set": set_alone("set"), "ledger_b": on_ledger(4, "ledger_b")})
                ms = {k: [] for k in list(variants) + ["host_credit"]}
                last = {}
                for r in range(a.warmup + a.rounds):
                    host_rows[:, :7] = 0
                    host_rows[:, 7] = np.uint64(0xFFFFFFFFFFFFFFFF)
                    for k, f in (list(variants.items()) if r % 2 == 0 else reversed(list(variants.items()))):
                        share_set.clear()  # an empty set every time, outside the timer
                        if k.startswith("ledger"):  # and an empty ledger
                            ledgers[4 if k == "ledger_b" else int(k[8:])].clear()
                        t, last[k] = timed(f)
                        if r >= a.warmup:
                            ms[k].append(t)
                    if r >= a.warmup:
                        ms["host_credit"].append(host_part[-1])
                    assert len(set(last.values())) == 1, last
                    want = bytes(verdicts["set"])
                    assert all(bytes(v) == want for v in verdicts.values()), (kind, r)
                    tables = [np.frombuffer(led.read(), dtype=np.uint64).reshape(nrows, 8) for led in ledgers.values()]
                    assert all(np.array_equal(t, host_rows) for t in tables), (kind, r)
                for led in ledgers.values():
                    led.close()
                row = dict(summary(ms), map=kind, rows=nrows, n=N, sessions=S, jobs=J, largest_account=top,
                           rounds_compared=a.warmup + a.rounds, control=ratios(ms, "ledger_b", "ledger_p4"),
                           ratio_host_way_set=ratios(ms, "host_way", "set"))
                for p in PEELS:
                    row[f"ratio_p{p}_set"] = ratios(ms, f"ledger_p{p}", "set")
                    row[f"ratio_p{p}_host_way"] = ratios(ms, f"ledger_p{p}", "host_way")
                rows_out.append(row)
                print(kind, " ".join("%s %.3f ms" % (k, row[k]["median_ms"]) for k in ms), flush=True)

    res = {"rounds": a.rounds, "warmup": a.warmup, "n": N, "sessions": S, "jobs": J, "set_capacity": SET_CAPACITY,
           "peels": list(PEELS), "results": rows_out}
    with open(os.path.join(a.out, "bench_ledger.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")

    def band(r):
        return f"{r['median']:.3f} [{r['min']:.3f}, {r['max']:.3f}]"

    lines = ["# bm_ledger_verify_jobs on one MI355X", "",
             f"`tools/bench_ledger.py`: n = 2^17 random submissions, all accepted, over 2^12 sessions and {J} synthetic jobs (a "
             f"12-entry branch and a 250-byte coinbase each), a 2^22 share set and the ledger cleared outside the timer before "
             f"every call; medians of {a.rounds} rounds after {a.warmup} warm-up, the variants alternating in one process, every "
             "call through the C ABI into buffers allocated once.  (a) is one `bm_ledger_verify_jobs` call at 0, 1, 4 and 64 "
             "peel rounds; (b) is `bm_share_set_verify_jobs` and then the CPU ledger's crediting loop on one host thread; (c) is "
             "`bm_share_set_verify_jobs` alone.  A ratio is per round, given as median [min, max]; the control is (a) at 4 "
             "rounds against itself.  The verdict bytes and the ledger rows of all variants were compared in every round.  Raw "
             "figures: `bench_ledger.json`.", "",
             "| map | rows | largest account | (c) set alone ms | (b) host way ms (its loop alone) | (a) ms at 0 / 1 / 4 / 64 |"
             " (a)/(c) at 0 | at 1 | at 4 | at 64 | control |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows_out:
        lines.append(f"| {r['map']} | {r['rows']} | {r['largest_account']} | {r['set']['median_ms']:.3f} | "
                     f"{r['host_way']['median_ms']:.3f} ({r['host_credit']['median_ms']:.3f}) | "
                     + " / ".join(f"{r[f'ledger_p{p}']['median_ms']:.3f}" for p in PEELS) + " | "
                     + " | ".join(band(r[f"ratio_p{p}_set"]) for p in PEELS) + f" | {band(r['control'])} |")
    lines += ["", "* every figure is a whole call, copies and host work included; the set and the ledger are cleared outside the "
                  "timed call",
              "* not measured: the kernel's own time, the shader clock, PMC counters, more than one GPU"]
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
