#!/usr/bin/env python3
"""Writes the fixtures of the pool_jobs command line (tests/test_pool_jobs_cli.py and
the README's example), with hashlib only:

  stratum_second_job.json     a second live job beside stratum_genesis_job.json: the
                              genesis job with another id, a later ntime and a
                              one-entry synthetic merkle branch
  stratum_jobs_sessions.json  stratum_genesis_sessions.json's workers and easy.1, at
                              difficulty 2^-20 (a target of 12 zero bits)
  stratum_jobs_submits.txt    the genesis submission and shares of the second job
                              found here at about 12 zero bits, in a mixed order, with
                              a repeat, an unknown job id, a share sent under the
                              other job's id and a share with a late ntime
  stratum_jobs_expected.json  what pool_jobs prints for them: plain, with
                              --ntime-slack 60, and with --dedup

    python3 tests/golden/make_jobs_golden.py
"""
import hashlib
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
DIFF1 = 0xffff << 208
EASY = 2.0 ** -20


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def header_hash(job, extranonce1, extranonce2, ntime, nonce, version):
    n = job["notify"]
    coinbase = (bytes.fromhex(n[2]) + extranonce1 + extranonce2.to_bytes(job["extranonce2_size"], "big")
                + bytes.fromhex(n[3]))
    root = sha256d(coinbase)
    for entry in n[4]:
        root = sha256d(root + bytes.fromhex(entry))
    swapped = bytes.fromhex(n[1])
    prevhash = b"".join(swapped[4 * w:4 * w + 4][::-1] for w in range(8))
    header = (struct.pack("<I", version) + prevhash + root
              + struct.pack("<III", ntime, int(n[6], 16), nonce))
    return int.from_bytes(sha256d(header), "little")


def params(worker, job, extranonce2, ntime, nonce, job_id=None):
    return [worker, job_id or job["notify"][0], "%0*x" % (2 * job["extranonce2_size"], extranonce2), "%08x" % ntime,
            "%08x" % nonce, "00000000"]


def text(p):
    return json.dumps(p, separators=(",", ":"))


def classify(jobs, workers, p, slack):
    """pool_jobs' line for well-formed params of a known worker, without a share set."""
    if p[1] not in jobs:
        return "Reject job " + text(p)
    job = jobs[p[1]]
    en1, target = workers[p[0]]
    ntime, nonce = int(p[3], 16), int(p[4], 16)
    version = int(job["notify"][5], 16) & ~int(job["version_mask"], 16) | int(p[5], 16)
    h = header_hash(job, en1, int(p[2], 16), ntime, nonce, version)
    job_ntime = int(job["notify"][7], 16)
    if slack is not None and not job_ntime <= ntime <= job_ntime + slack:
        return "Reject ntime " + text(p)
    nbits = int(job["notify"][6], 16)
    block_target = (nbits & 0xffffff) << (8 * ((nbits >> 24) - 3))
    if h <= block_target:
        return "Block %s %064x" % (text(p), h)
    if h <= target:
        return "Accept %s %064x" % (text(p), h)
    return "Reject above-target " + text(p)


def main():
    with open(os.path.join(HERE, "stratum_genesis_job.json")) as f:
        genesis = json.load(f)
    with open(os.path.join(HERE, "stratum_genesis_sessions.json")) as f:
        sessions = json.load(f)
    second = json.loads(json.dumps(genesis))
    second["notify"][0] = "second"
    second["notify"][4] = [hashlib.sha256(b"a transaction that arrived after the first job").hexdigest()]
    second["notify"][7] = "%08x" % (int(genesis["notify"][7], 16) + 30)
    second["notify"][8] = False
    sessions["workers"]["easy.1"] = {"extranonce1": "0002", "difficulty": EASY}
    workers = {name: (bytes.fromhex(w["extranonce1"]), int(DIFF1 / w["difficulty"]))
               for name, w in sessions["workers"].items()}
    assert workers["easy.1"][1] == 0xffff << 228
    jobs = {"genesis": genesis, "second": second}

    # shares of the second job under easy.1: the first nonces from 0 that meet its target
    en1, target = workers["easy.1"]
    ntime2 = int(second["notify"][7], 16)
    found = []
    for extranonce2, ntime in ((0, ntime2), (1, ntime2), (2, ntime2 + 100)):
        nonce = 0
        while header_hash(second, en1, extranonce2, ntime, nonce, 1) > target:
            nonce += 1
        found.append(params("easy.1", second, extranonce2, ntime, nonce))
    block = params("satoshi.1", genesis, 29, int(genesis["notify"][7], 16), 2083236893)
    lines = [found[0], block, found[1], found[0], params("easy.1", second, 0, ntime2, int(found[0][4], 16), "third"),
             params("easy.1", second, 0, ntime2, int(found[0][4], 16), "genesis"), found[2], block]
    expected = {}
    for key, slack in (("plain", None), ("slack60", 60)):
        out = [classify(jobs, workers, p, slack) for p in lines]
        accepted = sum(1 for ln in out if not ln.startswith("Reject"))
        blocks = sum(1 for ln in out if ln.startswith("Block"))
        expected[key] = out + ["Verified %d Accepted %d Blocks %d Rejected %d" % (len(out), accepted, blocks, len(out) - accepted)]
    seen, out, dups = set(), [], 0
    for ln in expected["plain"][:-1]:
        if not ln.startswith("Reject") and ln.split()[-1] in seen:
            ln, dups = "Reject duplicate " + ln.split()[1], dups + 1
        elif not ln.startswith("Reject"):
            seen.add(ln.split()[-1])
        out.append(ln)
    accepted = sum(1 for ln in out if not ln.startswith("Reject"))
    blocks = sum(1 for ln in out if ln.startswith("Block"))
    expected["dedup"] = out + ["Verified %d Accepted %d Blocks %d Rejected %d Duplicates %d"
                               % (len(out), accepted, blocks, len(out) - accepted, dups)]
    expected["readme"] = [expected["plain"][1], expected["plain"][0], "Verified 2 Accepted 2 Blocks 1 Rejected 0"]

    def dump(name, obj):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(obj, f, indent=1)
            f.write("\n")

    dump("stratum_second_job.json", second)
    dump("stratum_jobs_sessions.json", sessions)
    dump("stratum_jobs_expected.json", expected)
    with open(os.path.join(HERE, "stratum_jobs_submits.txt"), "w") as f:
        f.write("".join(text(p) + "\n" for p in lines))


if __name__ == "__main__":
    main()
