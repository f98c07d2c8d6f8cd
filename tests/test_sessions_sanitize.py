"""The session table's host code under sanitizers (no GPU): tools/sessions_check.cpp, a
stand-alone program over csrc/bm_sessions.cpp, csrc/bm_ledger.cpp, csrc/bm_share_set.cpp
and csrc/bm_job.cpp, built with ASan and UBSan and run on the CPU."""
import os
import subprocess
import tempfile

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")


def test_sessions_host_code_under_sanitizers():
    """bm_target_from_difficulty_fx and the kernels' multiword arithmetic (compiled for
    the host) against a 128-bit restatement; the CPU table on exactly-sized heap buffers
    for `index`, `init`, the arrays of bm_sessions_get, `submits`, `verdicts` and
    `changes`, against bm_ledger_verify_jobs on the arrays it returned and the rule
    restated; BM_EFULL one entry short; the argument checks with canaries."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sessions_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "sessions_check.cpp"), os.path.join(CSRC, "bm_sessions.cpp"),
                               os.path.join(CSRC, "bm_ledger.cpp"), os.path.join(CSRC, "bm_share_set.cpp"),
                               os.path.join(CSRC, "bm_job.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("sessions check ok")
