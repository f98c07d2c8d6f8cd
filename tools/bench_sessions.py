#!/usr/bin/env python3
"""Measure the session table on one GPU ("Sessions"),
tools/bench_ledger.py's method: medians of --rounds rounds after --warmup, the
variants alternating inside each round (their order reversed every second round),
every call through the C ABI into buffers allocated once, every figure a whole call.

verify   n = 2^17 submissions that are (nearly all) accepted, over J = 8 synthetic jobs,
         a 2^22 share set and a ledger, both cleared outside the timer before every
         call, at S = 2^12, 2^16 and 2^20 sessions of difficulty 2^-32:
           table     bm_sessions_verify_jobs on a device table of S slots
           arrays    bm_ledger_verify_jobs on the arrays bm_sessions_get returned
           arrays_b  the control: arrays again; its per-round ratio to arrays is the noise band
         and `one`: table with all 2^17 submissions on one session, the tally's worst
         case.  Verdicts, results and ledger rows of the variants are compared every round.
retarget S = 2^12, 2^16 and 2^20 open sessions, about 1% and 100% of them changing (the
         others' windows are not over), the table set again outside the timer before
         every call:
           device    bm_sessions_retarget on the device table
           cpu       the same call on a CPU table, one thread
           host      the host's part of the device call alone (the ordering by session, the recheck of
                     every target, the list applied to the mirror: tools/sessions_host_share.cpp)
         The change lists and results of device and cpu are compared every round.

--rehearse runs the same code on CPU objects at small sizes and writes nothing: it
checks the script, and measures nothing.  Writes profiles/sessions/bench_sessions.json
and README.md."""
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
from distributed_bitcoin_minter_amd import Context, Ledger, SessionTable, ShareSet, VardiffPolicy, _lib  # noqa: E402
from bench_header_hits import ratios, summary, timed  # noqa: E402
from bench_jobs_verify import JOBS_SUBMIT, SIZE1, make_job  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "sessions")
CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")
J = 8
ROWS = 64
INIT = np.dtype([("extranonce1", "u1", 8), ("difficulty_fx", "<u8"), ("account", "<u4"), ("reserved", "<u4")])
CHANGE = np.dtype([("session", "<u4"), ("reserved", "<u4"), ("old_fx", "<u8"), ("new_fx", "<u8"), ("target", "u1", 32)])


def build_helper(d):
    so = os.path.join(d, "sessions_host_share.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "sessions_host_share.cpp"), os.path.join(CSRC, "bm_job.cpp"), "-o", so])
    helper = ctypes.CDLL(so)
    helper.bench_sessions_host_share.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p]
    helper.bench_sessions_host_share.restype = ctypes.c_int
    return helper


def alternate(variants, rounds, warmup, before, after_round):
    ms = {k: [] for k in variants}
    last = {}
    for r in range(warmup + rounds):
        for k, f in (list(variants.items()) if r % 2 == 0 else reversed(list(variants.items()))):
            before(k)
            t, last[k] = timed(f)
            if r >= warmup:
                ms[k].append(t)
        after_round(last)
    return ms


def set_table(lib, table, init, now_ms):
    _lib.check(lib.bm_sessions_set(table.handle, None, len(init), init.ctypes.data_as(ctypes.POINTER(_lib.SessionInit)), now_ms),
               "bm_sessions_set")


def bench_verify(a, lib, make, S, n, rs, jarr, one):
    make_table, make_ledger, make_set, set_capacity = make
    init = np.zeros(S, dtype=INIT)
    init["extranonce1"][:, :SIZE1] = rs.randint(0, 256, (S, SIZE1))
    init["difficulty_fx"] = 1  # the target 0xffff << 240: all but about 2^-16 of the hashes are accepted
    init["account"] = rs.randint(0, ROWS, S)
    subs = np.zeros(n, dtype=JOBS_SUBMIT)
    subs["extranonce2"] = rs.randint(0, 1 << 62, n, dtype=np.uint64)
    for k in ("ntime", "nonce", "version"):
        subs[k] = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    subs["session"] = 0 if one else rs.randint(0, S, n).astype(np.uint32)
    subs["job"] = rs.randint(0, J, n).astype(np.uint32)
    subs_c = (_lib.JobsSubmit * n).from_buffer(subs)
    with make_table(S) as table, make_set(set_capacity) as share_set:
        set_table(lib, table, init, 0)
        ses_c, acc, wgt = table.get()
        acc_c, wgt_c = (ctypes.c_uint32 * S)(*acc), (ctypes.c_uint64 * S)(*wgt)
        names = ("table", "arrays", "arrays_b")
        ledgers = {k: make_ledger(ROWS) for k in names}
        verdicts = {k: (_lib.JobVerdict * n)() for k in names}
        results = {}

        def through_table():
            r = _lib.LedgerResult()
            _lib.check(lib.bm_sessions_verify_jobs(table.handle, ledgers["table"].handle, share_set.handle, jarr, J, subs_c, n,
                                                   verdicts["table"], ctypes.byref(r)), "bm_sessions_verify_jobs")
            results["table"] = bytes(r)
            return r.credited

        def through_arrays(name):
            def f():
                r = _lib.LedgerResult()
                _lib.check(lib.bm_ledger_verify_jobs(ledgers[name].handle, share_set.handle, jarr, J, ses_c, S, acc_c, wgt_c, subs_c,
                                                     n, verdicts[name], ctypes.byref(r)), "bm_ledger_verify_jobs")
                results[name] = bytes(r)
                return r.credited
            return f

        variants = {"table": through_table, "arrays": through_arrays("arrays"), "arrays_b": through_arrays("arrays_b")}
        tallied = [0]

        def before(k):
            share_set.clear()  # an empty set and an empty ledger every time, outside the timer
            ledgers[k].clear()

        def after_round(last):
            assert len(set(last.values())) == 1 and n - 64 <= last["table"] <= n, last
            assert len(set(results.values())) == 1
            want = bytes(verdicts["arrays"])
            assert all(bytes(v) == want for v in verdicts.values())
            rows = [bytes(led.read()) for led in ledgers.values()]
            assert rows[0] == rows[1] == rows[2]
            tallied[0] += last["table"]

        ms = alternate(variants, a.rounds, a.warmup, before, after_round)
        state = np.frombuffer(table.state(), dtype=np.uint64).reshape(S, 4)
        assert int(state[:, 2].sum()) == tallied[0], "the tally over all rounds"
        for led in ledgers.values():
            led.close()
    return dict(summary(ms), sessions=S, n=n, one_session=one, bytes_not_copied=52 * S,
                ratio_table_arrays=ratios(ms, "table", "arrays"), control=ratios(ms, "arrays_b", "arrays"))


def bench_retarget(a, lib, make, helper, S, part, rs):
    make_table = make[0]
    policy = VardiffPolicy(target_ms=1000, window_ms=5000, band_permille=0).struct
    now = 6000
    init = np.zeros(S, dtype=INIT)
    init["extranonce1"][:] = rs.randint(0, 256, (S, 8))
    init["difficulty_fx"] = rs.randint(1 << 20, 1 << 40, S, dtype=np.uint64)
    init["account"] = rs.randint(0, ROWS, S)
    # the slots that change were set at 0 (a window of 6000 with no share: a quarter of the difficulty); the others
    # at 5000, and their window is not over
    due = rs.permutation(S)[:max(1, S * part // 100)]
    first = np.zeros(S, dtype=bool)
    first[due] = True
    with make_table(S) as dev, SessionTable.cpu(S) as cpu:
        changes = {k: np.zeros(len(due), dtype=CHANGE) for k in ("device", "cpu")}
        results = {}

        def reset(table):
            set_table(lib, table, init, 5000)
            idx = np.ascontiguousarray(due.astype(np.uint32))
            sub = np.ascontiguousarray(init[due])
            _lib.check(lib.bm_sessions_set(table.handle, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(due),
                                           sub.ctypes.data_as(ctypes.POINTER(_lib.SessionInit)), 0), "bm_sessions_set")

        def on(table, name):
            def f():
                r = _lib.VardiffResult()
                _lib.check(lib.bm_sessions_retarget(table.handle, now, ctypes.byref(policy),
                                                    changes[name].ctypes.data_as(ctypes.POINTER(_lib.VardiffChange)), len(due),
                                                    ctypes.byref(r)), "bm_sessions_retarget")
                results[name] = r.as_tuple()
                return r.changed
            return f

        ses_c, _, wgt = cpu.get(0, S)
        mirror_ses = np.frombuffer(ses_c, dtype=np.uint8).copy()
        scratch, ordered = np.zeros(len(due), dtype=CHANGE), np.zeros(len(due), dtype=CHANGE)
        mirror_wgt = np.zeros(S, dtype=np.uint64)

        def host():
            return helper.bench_sessions_host_share(scratch.ctypes.data, len(due), S, ordered.ctypes.data, mirror_ses.ctypes.data,
                                                    mirror_wgt.ctypes.data)

        variants = {"device": on(dev, "device"), "cpu": on(cpu, "cpu"), "host": host}

        def before(k):
            if k == "host":  # the list as the device may return it, unordered: shuffled; the mirror as before the call
                scratch[:] = changes["cpu"][rs.permutation(len(due))]
                mirror_wgt[:] = init["difficulty_fx"]
            else:
                reset(dev if k == "device" else cpu)

        def after_round(last):
            assert last["device"] == last["cpu"] == len(due) and last["host"] == 0, last
            assert results["device"] == results["cpu"] == (S, len(due), len(due), 0, len(due))
            assert changes["device"].tobytes() == changes["cpu"].tobytes()

        reset(cpu)
        on(cpu, "cpu")()  # the host variant's first list
        ms = alternate(variants, a.rounds, a.warmup, before, after_round)
        assert bytes(dev.get(0, S)[0]) == bytes(cpu.get(0, S)[0]) and bytes(dev.state(0, S)) == bytes(cpu.state(0, S))
    return dict(summary(ms), sessions=S, changing=len(due), ratio_device_cpu=ratios(ms, "device", "cpu"),
                host_share=ratios(ms, "host", "device"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--rehearse", action="store_true", help="CPU objects at small sizes: checks the script, measures nothing")
    a = ap.parse_args()
    lib = _lib.load()
    sizes, n, set_capacity = ((1 << 12, 1 << 16, 1 << 20), 1 << 17, 1 << 22) if not a.rehearse else ((1 << 6, 1 << 8), 1 << 9, 1 << 12)
    rng = random.Random(109)
    rs = np.random.RandomState(9)
    jobs = [make_job(rng) for _ in range(J)]
    jarr, _keep = _lib._jobs_array(jobs)
    verify, retarget = [], []
    with tempfile.TemporaryDirectory() as d:
        helper = build_helper(d)
        ctx = None if a.rehearse else Context(num_gpus=1)
        try:
            if a.rehearse:
                make = (SessionTable.cpu, Ledger.cpu, ShareSet.cpu, set_capacity)
            else:
                make = (lambda c: SessionTable(ctx, c), lambda r: Ledger(ctx, r), lambda c: ShareSet(ctx, c), set_capacity)
            for S in sizes:
                verify.append(bench_verify(a, lib, make, S, n, rs, jarr, False))
                print("verify", S, " ".join("%s %.3f ms" % (k, verify[-1][k]["median_ms"]) for k in ("table", "arrays", "arrays_b")),
                      flush=True)
            verify.append(bench_verify(a, lib, make, sizes[0], n, rs, jarr, True))
            print("verify one session", " ".join("%s %.3f ms" % (k, verify[-1][k]["median_ms"]) for k in ("table", "arrays")),
                  flush=True)
            for S in sizes:
                for part in (1, 100):
                    retarget.append(bench_retarget(a, lib, make, helper, S, part, rs))
                    print("retarget", S, part, " ".join("%s %.3f ms" % (k, retarget[-1][k]["median_ms"])
                                                       for k in ("device", "cpu", "host")), flush=True)
        finally:
            if ctx is not None:
                ctx.close()
    if a.rehearse:
        print("rehearsal ok: nothing measured, nothing written")
        return 0
    os.makedirs(a.out, exist_ok=True)
    res = {"rounds": a.rounds, "warmup": a.warmup, "n": n, "jobs": J, "set_capacity": set_capacity, "ledger_rows": ROWS,
           "verify": verify, "retarget": retarget}
    with open(os.path.join(a.out, "bench_sessions.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")

    def band(r):
        return f"{r['median']:.3f} [{r['min']:.3f}, {r['max']:.3f}]"

    lines = ["# The session table on one MI355X", "",
             f"`tools/bench_sessions.py`: medians of {a.rounds} rounds after {a.warmup} warm-up, the variants alternating in one "
             "process, every call through the C ABI into buffers allocated once; every figure is a whole call, copies and host "
             "work included.  A ratio is per round, given as median [min, max].  Raw figures: `bench_sessions.json`.", "",
             "## Verify", "",
             f"n = 2^17 submissions, all but about 2^-16 of them accepted, over {J} synthetic jobs (a 12-entry branch and a 250-byte "
             f"coinbase each), a 2^22 share set and a {ROWS}-row ledger, both cleared outside the timer before every call.  `table` "
             "is `bm_sessions_verify_jobs` on a device table; `arrays` is `bm_ledger_verify_jobs` on the arrays `bm_sessions_get` "
             "returned (52 bytes per session staged and copied up in every call); the control is `arrays` against itself.  The "
             "verdicts, the results and the ledger's rows of the variants were compared in every round, the table's tally at the end.",
             "", "| sessions | bytes per call not copied | arrays ms | table ms | table / arrays | control |", "|---|---|---|---|---|---|"]
    for r in verify:
        what = f"{r['sessions']}" + (" (all submissions on one session)" if r["one_session"] else "")
        lines.append(f"| {what} | {r['bytes_not_copied']} | {r['arrays']['median_ms']:.3f} | {r['table']['median_ms']:.3f} | "
                     f"{band(r['ratio_table_arrays'])} | {band(r['control'])} |")
    lines += ["", "## Retarget", "",
              "S open sessions; the changing ones have a window of 6 s without a share (a quarter of the difficulty), the others' "
              "windows are not over; the table is set again outside the timer before every call.  `device` is "
              "`bm_sessions_retarget` on the device table (two passes, two copies down, the host's ordering, recheck and mirror "
              "update), `cpu` the same call on a CPU table on one thread, `host` the host's part of the device call alone.  The "
              "change lists and the results of device and cpu were compared in every round, the tables at the end.", "",
              "| sessions | changing | cpu ms | device ms | device / cpu | host part ms | host part / device |", "|---|---|---|---|---|---|---|"]
    for r in retarget:
        lines.append(f"| {r['sessions']} | {r['changing']} | {r['cpu']['median_ms']:.3f} | {r['device']['median_ms']:.3f} | "
                     f"{band(r['ratio_device_cpu'])} | {r['host']['median_ms']:.3f} | {band(r['host_share'])} |")
    lines += ["", "* not measured: the kernels' own times, the shader clock, PMC counters, more than one GPU, a table next to "
                  "searches on the same device, bm_sessions_set (it runs outside the timers here)"]
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
