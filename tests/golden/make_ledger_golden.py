#!/usr/bin/env python3
"""Writes the fixtures of the pool_ledger command line (tests/test_pool_ledger_cli.py
and the README's example), with hashlib only.  The jobs are the two live jobs of
the pool_jobs fixtures (stratum_genesis_job.json, stratum_second_job.json).

  stratum_ledger_sessions.json  satoshi.1 at difficulty 1, and two accounts of easy
                                workers: farm.1 at 2^-20 and farm.2 at 2^-18 (one
                                account at two difficulties) and solo.1 at 2^-20
  stratum_ledger_submits.txt    the genesis block, shares of the second job found
                                here, a duplicate, an above-target share, a share
                                with a late ntime, an unknown job id and a line that
                                is no submission
  stratum_ledger_expected.json  what pool_ledger prints for them: plain, with
                                --dedup, with --dedup --by-worker and with
                                --ntime-slack 60

    python3 tests/golden/make_ledger_golden.py
"""
import json
import os

from make_jobs_golden import DIFF1, header_hash, params, text

HERE = os.path.dirname(os.path.abspath(__file__))
WORKERS = {"satoshi.1": ("ffff", 1), "farm.1": ("0002", 2.0 ** -20), "farm.2": ("0003", 2.0 ** -18),
           "solo.1": ("0004", 2.0 ** -20)}


def line_of(jobs, workers, p, slack, seen):
    """(pool_ledger's line, the class it counts in or None, hash) for params p;
    seen: the hashes recorded so far (None: no share set)."""
    if p[1] not in jobs:
        return "Reject job " + text(p), None, None
    job = jobs[p[1]]
    en1, target = workers[p[0]]
    ntime, nonce = int(p[3], 16), int(p[4], 16)
    version = int(job["notify"][5], 16) & ~int(job["version_mask"], 16) | int(p[5], 16)
    h = header_hash(job, en1, int(p[2], 16), ntime, nonce, version)
    job_ntime = int(job["notify"][7], 16)
    nbits = int(job["notify"][6], 16)
    block = h <= (nbits & 0xffffff) << (8 * ((nbits >> 24) - 3))
    eligible = block or h <= target
    duplicate = False
    if seen is not None and eligible:  # the set does not look at the window
        duplicate = h in seen
        seen.add(h)
    if slack is not None and not job_ntime <= ntime <= job_ntime + slack:
        return "Reject ntime " + text(p), "ntime", h
    if duplicate:
        return "Reject duplicate " + text(p), "duplicate", h
    if block:
        return "Block %s %064x" % (text(p), h), "block", h
    if eligible:
        return "Accept %s %064x" % (text(p), h), "accepted", h
    return "Reject above-target " + text(p), "above", h


def expected(jobs, workers, lines, slack, dedup, by_worker):
    seen = set() if dedup else None
    out, tallies = [], {}
    for w in WORKERS:
        tallies.setdefault(w if by_worker else w.split(".")[0], dict(accepted=0, block=0, above=0, ntime=0, duplicate=0,
                                                                     work=0, best=None))
    for raw in lines:
        if not isinstance(raw, list):
            out.append("Reject malformed " + raw)
            continue
        ln, cls, h = line_of(jobs, workers, raw, slack, seen)
        out.append(ln)
        if cls is None:
            continue
        t = tallies[raw[0] if by_worker else raw[0].split(".")[0]]
        if cls in ("accepted", "block"):
            t["accepted"] += 1
            t["block"] += cls == "block"
            t["work"] += max(1, int(WORKERS[raw[0]][1] * 2 ** 32))
            t["best"] = h >> 192 if t["best"] is None else min(t["best"], h >> 192)
        else:
            t[cls] += 1
    accepted = sum(1 for ln in out if not ln.startswith("Reject"))
    blocks = sum(1 for ln in out if ln.startswith("Block"))
    closing = "Verified %d Accepted %d Blocks %d Rejected %d" % (len(out), accepted, blocks, len(out) - accepted)
    if dedup:
        closing += " Duplicates %d" % sum(1 for ln in out if ln.startswith("Reject duplicate"))
    out.append(closing)
    for name in sorted(tallies):
        t = tallies[name]
        rejected = t["above"] + t["ntime"] + t["duplicate"]
        out.append("Account %s Accepted %d Blocks %d Rejected %d AboveTarget %d Ntime %d Duplicate %d Extranonce2 0 Work %d Best %s"
                   % (name, t["accepted"], t["block"], rejected, t["above"], t["ntime"], t["duplicate"], t["work"],
                      "-" if t["best"] is None else "%016x" % t["best"]))
    return out


def main():
    jobs = {}
    for name in ("stratum_genesis_job.json", "stratum_second_job.json"):
        with open(os.path.join(HERE, name)) as f:
            job = json.load(f)
        jobs[job["notify"][0]] = job
    genesis, second = jobs["genesis"], jobs["second"]
    sessions = {"workers": {w: {"extranonce1": en1, "difficulty": d} for w, (en1, d) in WORKERS.items()}}
    workers = {w: (bytes.fromhex(en1), int(DIFF1 / d)) for w, (en1, d) in WORKERS.items()}
    ntime2 = int(second["notify"][7], 16)

    def find(worker, extranonce2, ntime, good=True):
        """The first nonce from 0 that meets (good) or misses the worker's target."""
        en1, target = workers[worker]
        nonce = 0
        while (header_hash(second, en1, extranonce2, ntime, nonce, 1) <= target) != good:
            nonce += 1
        return params(worker, second, extranonce2, ntime, nonce)

    a1, a2 = find("farm.1", 0, ntime2), find("farm.1", 1, ntime2)
    b1 = find("farm.2", 0, ntime2)
    c1 = find("solo.1", 0, ntime2)
    late = find("solo.1", 1, ntime2 + 100)
    above = find("farm.2", 2, ntime2, good=False)
    block = params("satoshi.1", genesis, 29, int(genesis["notify"][7], 16), 2083236893)
    unknown = params("farm.1", second, 0, ntime2, int(a1[4], 16), "third")
    lines = [a1, block, b1, a1, above, unknown, c1, "hello", a2, late, b1]
    expect = {"plain": expected(jobs, workers, lines, None, False, False),
              "dedup": expected(jobs, workers, lines, None, True, False),
              "dedup_by_worker": expected(jobs, workers, lines, None, True, True),
              "slack60": expected(jobs, workers, lines, 60, True, False)}

    def dump(name, obj):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(obj, f, indent=1)
            f.write("\n")

    dump("stratum_ledger_sessions.json", sessions)
    dump("stratum_ledger_expected.json", expect)
    with open(os.path.join(HERE, "stratum_ledger_submits.txt"), "w") as f:
        f.write("".join((text(p) if isinstance(p, list) else p) + "\n" for p in lines))


if __name__ == "__main__":
    main()
