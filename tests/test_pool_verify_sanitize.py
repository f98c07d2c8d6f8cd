"""The pool verifier's host code under sanitizers (no GPU): tools/pool_verify_check.cpp,
a stand-alone program over csrc/bm_job.hpp and csrc/bm_job.cpp, built with ASan
and UBSan and run on the CPU."""
import os
import subprocess
import tempfile

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc")


def test_pool_verify_host_code_under_sanitizers():
    """field_words over every (size1, size2, boff) against its bytes; the tail
    template and the field's five words replayed against bm_job_header over the
    edge layouts (the field against word and block edges, every padding edge, the
    coinbase limit); bm_pool_verify_cpu on exactly-sized heap buffers for
    `sessions`, `submits` and `verdicts`; INVALID entries; the refusals with
    canaries."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pool_verify_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "pool_verify_check.cpp"), os.path.join(CSRC, "bm_job.cpp"),
                               "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("pool verify check ok")
