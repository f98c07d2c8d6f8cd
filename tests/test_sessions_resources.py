"""The built session-table kernels' resources (no GPU): the unit's resource remarks."""
import os

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "distributed_bitcoin_minter_amd", "csrc", "build")
KERNELS = ("sessions_set_kernel", "sessions_tally_kernel", "sessions_retarget_kernel")


def test_kernel_resources():
    """No scratch, no spills and no LDS, in any of the three kernels."""
    path = os.path.join(BUILD, "bm_sessions_inst.res")
    if not os.path.exists(path):
        pytest.skip("device assembly not built (make -C distributed_bitcoin_minter_amd/csrc)")
    with open(path) as f:
        res = f.read()
    for kernel in KERNELS:
        assert kernel in res, kernel
    assert res.count("Function Name:") == len(KERNELS)
    for line in ("ScratchSize [bytes/lane]: 0", "SGPRs Spill: 0", "VGPRs Spill: 0", "LDS Size [bytes/block]: 0"):
        assert res.count(line) == len(KERNELS), (line, res[-1500:])
