"""The ledger's host code under sanitizers (no GPU): tools/ledger_check.cpp, a
stand-alone program over csrc/bm_ledger.cpp, csrc/bm_share_set.cpp and
csrc/bm_job.cpp, built with ASan and UBSan and run on the CPU."""
import os
import subprocess
import tempfile

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")


def test_ledger_host_code_under_sanitizers():
    """The CPU ledger on exactly-sized heap buffers for `sessions`, `accounts`,
    `weights`, `submits`, `verdicts` and the rows read back, against
    bm_jobs_verify_cpu plus a std::map; the argument checks with canaries; drain,
    clear and the wrap-around of `work`."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ledger_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "ledger_check.cpp"), os.path.join(CSRC, "bm_ledger.cpp"),
                               os.path.join(CSRC, "bm_share_set.cpp"), os.path.join(CSRC, "bm_job.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("ledger check ok")
