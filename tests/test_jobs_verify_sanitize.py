"""The host code of verification over several jobs under sanitizers (no GPU):
tools/jobs_verify_check.cpp, a stand-alone program over csrc/bm_job.hpp and
csrc/bm_job.cpp, built with ASan and UBSan and run on the CPU."""
import os
import subprocess
import tempfile

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")


def test_jobs_verify_host_code_under_sanitizers():
    """bm_jobs_verify_cpu on exactly-sized heap buffers for the jobs, `sessions`,
    `submits` and `verdicts` against bm_pool_verify_cpu per submission; the counting
    sort, the block table and the scatter into an exactly-sized stage over 0, 1, 3, 5
    and 64 jobs and the batch sizes around a workgroup; the descriptors' offsets;
    the tripwire's entries; the refusals with canaries."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "jobs_verify_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "jobs_verify_check.cpp"), os.path.join(CSRC, "bm_job.cpp"),
                               "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("jobs verify check ok")
