"""The Stratum job layer's host code under sanitizers (no GPU): tools/job_check.cpp,
a stand-alone program over csrc/bm_job.hpp and csrc/bm_job.cpp, built with ASan
and UBSan and run on the CPU."""
import os
import subprocess
import tempfile

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")


def test_job_host_code_under_sanitizers():
    """bm_job_header on exactly-sized heap buffers around the block edges and at
    the limit, the refusals, the share merge on synthetic per-header results and
    bm_target_from_difficulty at its edges."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "job_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "job_check.cpp"), os.path.join(CSRC, "bm_job.cpp"),
                               "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("job check ok")
