"""The built jobs_verify_kernel's resources (no GPU): the unit's resource remarks."""
import os

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc", "build")


def test_kernel_resources():
    """No scratch, no spills, no LDS: the job's descriptor stays in scalar registers."""
    path = os.path.join(BUILD, "bm_jobs_verify_inst.res")
    if not os.path.exists(path):
        pytest.skip("device assembly not built (make -C distributed_bitcoin_minter_amd/csrc)")
    with open(path) as f:
        res = f.read()
    assert "jobs_verify_kernel" in res
    for line in ("ScratchSize [bytes/lane]: 0", "SGPRs Spill: 0", "VGPRs Spill: 0", "LDS Size [bytes/block]: 0"):
        assert res.count(line) == 1, (line, res[-1500:])
